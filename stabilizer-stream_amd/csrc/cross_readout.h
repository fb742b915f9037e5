// cross_readout.h -- the bank read-out of the pair and matrix objects (psdcxr_*, include/psdcascade_crossread.h): the job table, the
// argument rules, and what cross_stitch_kernel and cross_band_kernel (cross_readout.hip) compute for one element and one thread.
// The band walk, its reduction order and the two f32 factors of a job are those of bank_readout.h.  Host and device:
// tests/host/cross_readout_check.cpp runs these on the CPU.
#pragma once
#include "bank_readout.h"

#include <limits>

namespace psdk {

constexpr uint32_t XREAD_MAX_ROWS = 16;  // accumulator rows of a stage the stitch kernel takes (m * m of a matrix object, m <= 4)
constexpr uint32_t XREAD_PAIR_ROWS = 4;  // xx, yy, re xy, im xy
constexpr uint32_t XREAD_THREADS = BANK_STITCH_THREADS;

// one included stage of one selected unit: output elements [start, start + bins_end - bins_start) of each of the unit's rows come
// from bins [bins_start, bins_end) of the stage's f64 accumulator `src`, laid out [rows][bins]
struct CrossReadJob {
    const double *src;
    uint32_t row, start; // the selected unit's index in the call, the first output element
    uint32_t bins_start, bins_end;
    float gsc, rbw;
    uint32_t rows, bins;
};
static_assert(sizeof(CrossReadJob) == 40, "the job table is copied to the device as it is");

// where a pair call's rows go (any may be null: not wanted); row i of an output starts at i * stride elements (pairs of them for
// sxy and transfer, which hold (re, im) a bin)
struct CrossPairOut {
    float *sxx, *syy, *sxy, *freq;
    double *coherence, *transfer;
    size_t stride;
    bool any() const { return sxx || syy || sxy || freq || coherence || transfer; }
};

// what a job type derived from CrossReadJob takes from its Break beyond the fields below (carrier_readout.h: the count); nothing here.
// (cross_row_jobs calls this unqualified on a dependent type: an overload for a derived job, declared later beside that type in
// namespace psdk, is found by argument-dependent lookup at instantiation)
template <class B>
inline void cross_job_break(CrossReadJob &, const B &)
{
}

// The jobs of one unit from its Breaks, as bank_row_jobs makes them (Break i belongs to stage n_breaks - 1 - i).  Jobs: a vector
// of CrossReadJob or of a type derived from it.
template <class B, class Jobs, class Src, class Gain>
inline BankRow cross_row_jobs(const B *breaks, size_t n_breaks, uint32_t row, uint32_t rows, uint32_t bins, Jobs &jobs, Src src_of, Gain gain_of)
{
    BankRow r{(uint32_t)jobs.size(), 0, 0, 0};
    for (size_t i = 0; i < n_breaks; ++i) {
        const B &b = breaks[i];
        if (!b.include || b.bins_end <= b.bins_start)
            continue;
        const uint32_t stage = (uint32_t)(n_breaks - 1 - i);
        typename Jobs::value_type j;
        cross_job_break(j, b);
        j.src = src_of(stage);
        j.row = row;
        j.start = (uint32_t)b.start;
        j.bins_start = (uint32_t)b.bins_start;
        j.bins_end = (uint32_t)b.bins_end;
        j.gsc = bank_gsc(gain_of(stage), b.decimation);
        j.rbw = bank_rbw(b.fft_size, b.decimation);
        j.rows = rows;
        j.bins = bins;
        jobs.push_back(j);
        ++r.njobs;
        r.len = j.start + (j.bins_end - j.bins_start);
    }
    return r;
}

// the accumulator of row r at bin k, and its stitched value: the f32 cast and the one f32 multiply of psdc_cross_csd / psdc_csm_csd
PSDK_BR_HD inline double cross_acc(const CrossReadJob &j, uint32_t r, uint32_t k) { return j.src[(size_t)r * j.bins + k]; }
PSDK_BR_HD inline float cross_scaled(double acc, float gsc) { return (float)acc * gsc; }
PSDK_BR_HD inline float cross_val(const CrossReadJob &j, uint32_t r, uint32_t k) { return cross_scaled(cross_acc(j, r, k), j.gsc); }

// coherence and H1 of one bin from its four f64 accumulators (the scale cancels: no f32 rounding enters)
PSDK_BR_HD inline double cross_coherence(double xx, double yy, double re, double im)
{
    const double den = xx * yy;
    return den != 0 ? (re * re + im * im) / den : std::numeric_limits<double>::quiet_NaN();
}
PSDK_BR_HD inline void cross_transfer(double xx, double re, double im, double out[2])
{
    out[0] = xx != 0 ? re / xx : std::numeric_limits<double>::quiet_NaN();
    out[1] = xx != 0 ? im / xx : std::numeric_limits<double>::quiet_NaN();
}

// what one thread of the pair form of cross_stitch_kernel does for element i of job j: the four values stay in registers
PSDK_BR_HD inline void cross_pair_element(const CrossReadJob &j, uint32_t i, const CrossPairOut &o)
{
    const uint32_t k = j.bins_start + i;
    const size_t e = (size_t)j.row * o.stride + j.start + i;
    const double xx = cross_acc(j, 0, k), yy = cross_acc(j, 1, k), re = cross_acc(j, 2, k), im = cross_acc(j, 3, k);
    if (o.sxx)
        o.sxx[e] = cross_scaled(xx, j.gsc);
    if (o.syy)
        o.syy[e] = cross_scaled(yy, j.gsc);
    if (o.sxy) {
        o.sxy[2 * e] = cross_scaled(re, j.gsc);
        o.sxy[2 * e + 1] = cross_scaled(im, j.gsc);
    }
    if (o.freq)
        o.freq[e] = bank_freq(j, k);
    if (o.coherence)
        o.coherence[e] = cross_coherence(xx, yy, re, im);
    if (o.transfer)
        cross_transfer(xx, re, im, o.transfer + 2 * e);
}

// ... and of the matrix form: out is [units][j.rows][stride] (may be null), freq [units][stride] (may be null)
PSDK_BR_HD inline void cross_rows_element(const CrossReadJob &j, uint32_t i, float *out, float *freq, size_t stride)
{
    const uint32_t k = j.bins_start + i;
    if (out)
        for (uint32_t r = 0; r < j.rows; ++r)
            out[((size_t)j.row * j.rows + r) * stride + j.start + i] = cross_val(j, r, k);
    if (freq)
        freq[(size_t)j.row * stride + j.start + i] = bank_freq(j, k);
}

// the band sums of a pair: bank_readout.h's walk over the four stitched rows; acc and out are [4][BANK_MAX_BANDS]
PSDK_BR_HD inline void cross_band_thread(const CrossReadJob *jobs, uint32_t nj, uint32_t L, uint32_t t, uint32_t T, const BankBands &bands,
                                         double (*acc)[BANK_MAX_BANDS])
{
    bank_band_walk<XREAD_PAIR_ROWS>(
        jobs, nj, L, t, T, bands, [](const CrossReadJob &j, uint32_t r, uint32_t k) { return cross_val(j, r, k); }, acc);
}
inline void cross_band_pair_host(const CrossReadJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, double (*out)[BANK_MAX_BANDS])
{
    bank_band_rows_host<XREAD_PAIR_ROWS>(
        jobs, nj, L, bands, [](const CrossReadJob &j, uint32_t r, uint32_t k) { return cross_val(j, r, k); }, out);
}

// The argument rules that need no object (the texts of include/psdcascade_crossread.h); nullptr: the arguments are good.
inline const char *cross_read_layout_refusal(const void *lens, const void *n_breaks, const void *breaks)
{
    if (!lens)
        return "null lens";
    if (breaks && !n_breaks)
        return "breaks without n_breaks";
    return nullptr;
}
// bands: [n_bands][2] = (lo, hi) on the host; *bb is filled when the arguments are good
inline const char *cross_read_band_refusal(const float *bands, uint32_t n_bands, const void *band_out, bool any_row_output, BankBands *bb)
{
    if (n_bands > BANK_MAX_BANDS)
        return "more than 8 bands";
    if (n_bands && !bands)
        return "n_bands without a band list";
    if ((n_bands != 0) != (band_out != nullptr))
        return n_bands ? "bands without a band output" : "a band output without bands";
    if (!any_row_output && !band_out)
        return "no output";
    bb->n = n_bands;
    for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b) {
        bb->lo[b] = b < n_bands ? bands[2 * b] : 0.0f;
        bb->hi[b] = b < n_bands ? bands[2 * b + 1] : 0.0f;
        if (b < n_bands && !(bb->lo[b] <= bb->hi[b])) // (false for a NaN on either side)
            return "a band with NaN or lo > hi";
    }
    return nullptr;
}

// cross_readout.hip (a host build of cross_runtime.cpp has inline stand-ins).  Jobs of at most max_bins bins each.
#if defined(__HIPCC__)
hipError_t launch_cross_stitch_pair(const CrossReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const CrossPairOut &out, hipStream_t s);
hipError_t launch_cross_stitch_rows(const CrossReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, float *d_rows, float *d_freq, size_t stride,
                                    hipStream_t s);
// one workgroup a selected pair; d_out is [n_units][bands.n][4] f64
hipError_t launch_cross_band(const CrossReadJob *d_jobs, const BankRow *d_units, uint32_t n_units, const BankBands &bands, double *d_out,
                             hipStream_t s);
#endif

} // namespace psdk
