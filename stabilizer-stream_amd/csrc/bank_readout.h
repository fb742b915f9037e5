// bank_readout.h -- the bank read-out (psdcr_*, include/psdcascade_readout.h): the job table, and what bank_stitch_kernel and
// bank_band_kernel (bank_readout.hip) compute for one element and one thread.  Host and device: tests/host/bank_readout_check.cpp
// runs these on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#if defined(__HIPCC__)
#define PSDK_BR_HD __host__ __device__
#else
#define PSDK_BR_HD
#endif
// The f64 product of the band sums stands next to an addition.  Nothing in this header keeps a compiler from fusing the two: the
// device TU (bank_readout.hip) is built with -ffp-contract=off (csrc/Makefile), which is what makes the product round on its own
// there (hipcc's __dmul_rn is a plain product that contracts like any other); a host build has no fused multiply-add to contract
// into unless it is asked for one.

namespace psdk {

constexpr uint32_t BANK_MAX_BANDS = 8;    // PSDCR_MAX_BANDS
constexpr uint32_t BANK_MAX_ROWS = 65536; // PSDCR_MAX_ROWS
constexpr uint32_t BANK_STITCH_THREADS = 256;
constexpr uint32_t BANK_BAND_THREADS = 256; // four wavefronts: the band sums' order is defined for this number
constexpr uint32_t BANK_WAVE = 64;

// one included stage of one selected row: output elements [start, start + bins_end - bins_start) of row `row` come from bins
// [bins_start, bins_end) of the accumulator row `src`
struct BankJob {
    const float *src;
    uint32_t row, start;
    uint32_t bins_start, bins_end;
    float gsc, rbw;
};
static_assert(sizeof(BankJob) == 32, "the job table is copied to the device as it is");

// one selected row: its jobs [job0, job0 + njobs) in output order (deepest stage first, contiguous from element 0) and its length
struct BankRow {
    uint32_t job0, njobs;
    uint32_t len, _pad;
};
static_assert(sizeof(BankRow) == 16, "the row table is copied to the device as it is");

struct BankBands {
    float lo[BANK_MAX_BANDS], hi[BANK_MAX_BANDS];
    uint32_t n;
};

// the two f32 factors of a job, as PsdCascade::psd (gain: PsdStage::gain of the stage, in f32) and Break::rbw form them
inline float bank_gsc(float gain, uint64_t decimation) { return 1.0f / (gain * (float)decimation); }
inline float bank_rbw(uint64_t fft_size, uint64_t decimation) { return 1.0f / (float)(fft_size * decimation); }

// The jobs of one row from its Breaks (deepest stage first, as the stitch writes them; B is psdc_break): Break i belongs to stage
// n_breaks - 1 - i, whose accumulator row and gain the two callables give.  Appends to `jobs`, returns the row's record.
template <class B, class Jobs, class Src, class Gain>
inline BankRow bank_row_jobs(const B *breaks, size_t n_breaks, uint32_t row, Jobs &jobs, Src src_of, Gain gain_of)
{
    BankRow r{(uint32_t)jobs.size(), 0, 0, 0};
    for (size_t i = 0; i < n_breaks; ++i) {
        const B &b = breaks[i];
        if (!b.include || b.bins_end <= b.bins_start)
            continue;
        const uint32_t stage = (uint32_t)(n_breaks - 1 - i);
        BankJob j;
        j.src = src_of(stage);
        j.row = row;
        j.start = (uint32_t)b.start;
        j.bins_start = (uint32_t)b.bins_start;
        j.bins_end = (uint32_t)b.bins_end;
        j.gsc = bank_gsc(gain_of(stage), b.decimation);
        j.rbw = bank_rbw(b.fft_size, b.decimation);
        jobs.push_back(j);
        ++r.njobs;
        r.len = j.start + (j.bins_end - j.bins_start);
    }
    return r;
}

// one f32 multiply an element each: the bytes of psdc_psd and psdc_frequencies
PSDK_BR_HD inline float bank_psd(const BankJob &j, uint32_t k) { return j.src[k] * j.gsc; }
template <class Job>
PSDK_BR_HD inline float bank_freq(const Job &j, uint32_t k) { return (float)k * j.rbw; }

// What thread t of T adds up for one unit of R stitched rows that share their jobs (a PSD row: R = 1; the four rows of a pair,
// cross_readout.h): the trapezoids t_e of the elements e = t, t + T, ... < L of each row r, each into the bands that hold f[e].
// p[e] = val(job, r, bin) and f[e] come from the jobs (the rows themselves are not read); p[-1] = f[-1] = 0.
template <uint32_t R, class Job, class Val>
PSDK_BR_HD inline void bank_band_walk(const Job *jobs, uint32_t nj, uint32_t L, uint32_t t, uint32_t T, const BankBands &bands, Val val,
                                      double (*acc)[BANK_MAX_BANDS])
{
    uint32_t ji = 0;
    for (uint32_t e = t; e < L; e += T) {
        while (ji + 1 < nj && e >= jobs[ji + 1].start)
            ++ji;
        const Job &j = jobs[ji];
        const uint32_t k = j.bins_start + (e - j.start);
        const Job *q = nullptr; // the job and bin of element e - 1
        uint32_t kq = 0;
        if (e > j.start) {
            q = &j;
            kq = k - 1;
        } else if (ji > 0) {
            q = &jobs[ji - 1];
            kq = q->bins_end - 1;
        }
        const float f = bank_freq(j, k), f1 = q ? bank_freq(*q, kq) : 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t r = 0; r < R; ++r) {
            // (val yields the stitched f32 value, or an f64 that was never cast to f32: carrier_readout.h; float to double is exact)
            const double p = val(j, r, k), p1 = q ? (double)val(*q, r, kq) : 0.0;
            const double tk = (0.5 * (p + p1)) * ((double)f - (double)f1); // rounded on its own: see the top
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
                if (b < bands.n && bands.lo[b] <= f && f <= bands.hi[b])
                    acc[r][b] += tk;
        }
    }
}

PSDK_BR_HD inline void bank_band_thread(const BankJob *jobs, uint32_t nj, uint32_t L, uint32_t t, uint32_t T, const BankBands &bands,
                                        double acc[BANK_MAX_BANDS])
{
    bank_band_walk<1>(
        jobs, nj, L, t, T, bands, [](const BankJob &j, uint32_t, uint32_t k) { return bank_psd(j, k); },
        reinterpret_cast<double(*)[BANK_MAX_BANDS]>(acc));
}

// The band sums of one unit as bank_band_kernel / cross_band_kernel form them, on the host: BANK_BAND_THREADS threads, then within
// each wavefront the tree v[l] += v[l + off] for off = 32, 16 ... 1 (lane 0 holds the wavefront's sum), then the wavefronts in order.
template <uint32_t R, class Job, class Val>
inline void bank_band_rows_host(const Job *jobs, uint32_t nj, uint32_t L, const BankBands &bands, Val val, double (*out)[BANK_MAX_BANDS])
{
    static double acc[BANK_BAND_THREADS][R][BANK_MAX_BANDS];
    for (uint32_t t = 0; t < BANK_BAND_THREADS; ++t) {
        for (uint32_t r = 0; r < R; ++r)
            for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
                acc[t][r][b] = 0.0;
        bank_band_walk<R>(jobs, nj, L, t, BANK_BAND_THREADS, bands, val, acc[t]);
    }
    for (uint32_t r = 0; r < R; ++r)
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b) {
            double sum = 0.0;
            for (uint32_t w = 0; w < BANK_BAND_THREADS / BANK_WAVE; ++w) {
                double v[BANK_WAVE];
                for (uint32_t l = 0; l < BANK_WAVE; ++l)
                    v[l] = acc[w * BANK_WAVE + l][r][b];
                for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
                    for (uint32_t l = 0; l < off; ++l)
                        v[l] += v[l + off];
                sum = w ? sum + v[0] : v[0];
            }
            out[r][b] = sum;
        }
}

inline void bank_band_row_host(const BankJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, double out[BANK_MAX_BANDS])
{
    bank_band_rows_host<1>(
        jobs, nj, L, bands, [](const BankJob &j, uint32_t, uint32_t k) { return bank_psd(j, k); },
        reinterpret_cast<double(*)[BANK_MAX_BANDS]>(out));
}

#if defined(__HIPCC__)
// bank_readout.hip.  Jobs of at most max_bins bins each; psd and freq rows of `stride` floats (either may be null)
hipError_t launch_bank_stitch(const BankJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, float *d_psd, float *d_freq, size_t stride,
                              hipStream_t s);
// one workgroup a row; d_out is [n_rows][bands.n] f64
hipError_t launch_bank_band(const BankJob *d_jobs, const BankRow *d_rows, uint32_t n_rows, const BankBands &bands, double *d_out,
                            hipStream_t s);
#endif

} // namespace psdk
