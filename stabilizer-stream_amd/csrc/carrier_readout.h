// carrier_readout.h -- the bank read-out of the six single-channel carrier kinds (psdczr_*, include/psdcascade_carrierread.h: the
// zoom, IQ, zoom / IQ spectral kurtosis and zoom / IQ AM/PM objects): the job and unit tables, the argument rules, and what
// carrier_stitch_kernel and carrier_band_kernel (carrier_readout.hip) compute for one element and one thread.  The jobs, the two
// f32 factors, the band walk and its reduction order are those of cross_readout.h / bank_readout.h.  Host and device:
// tests/host/carrier_readout_check.cpp runs these on the CPU, and cross_runtime.cpp's host read-outs call sk_estimate.
// Every f64 product here stands next to a sum: the device TU is built with -ffp-contract=off (csrc/Makefile), as bank_readout.hip.
#pragma once
#include "cross_readout.h"

#include <cmath>
#include <limits>

namespace psdk {

constexpr uint32_t CREAD_SIDE_ROWS = 2; // upper, lower: rows 0 and 1 of all six kinds
constexpr uint32_t CREAD_ROWS = 4;      // SK kinds: S1 up, S1 lo, S2 up, S2 lo; AM/PM kinds: upper, lower, comp re, comp im
constexpr int CREAD_SIDES = 0, CREAD_SK = 1, CREAD_AMPM = 2; // the modes of carrier_stitch_kernel

// a CrossReadJob that also carries the count its Break reports (what sk_estimate takes on the host)
struct CarrierReadJob : CrossReadJob {
    uint32_t count, _pad;
};
static_assert(sizeof(CrossReadJob) == 40 && sizeof(CarrierReadJob) == 48, "the job table is copied to the device as it is");
// cross_row_jobs (cross_readout.h) finds this overload by argument-dependent lookup when it is instantiated for a vector of
// CarrierReadJob: it must stay in namespace psdk beside the type and keep (CarrierReadJob &, const B &), or the no-op for
// CrossReadJob is taken silently and SK gets an unset count (tests/host/carrier_readout_check.cpp asserts the counts)
template <class B>
inline void cross_job_break(CarrierReadJob &j, const B &b)
{
    j.count = b.count;
    j._pad = 0;
}

// one selected channel of an AM/PM call: where its carrier comes from
struct CarrierUnit {
    const double *src0; // stage 0's accumulator [4][bins] (null: the channel has no stage)
    double n2p;         // (double)n * (double)n * (double)power, power the object's f32 window power
    double P, ur, ui;   // given != 0: the carrier's power and u = A^2 / |A|^2 from the host
    uint32_t count0;    // the count stage 0 reports
    uint32_t given;
    uint32_t bins, _pad;
};
static_assert(sizeof(CarrierUnit) == 56, "the unit table is copied to the device as it is");

// where a call's rows go (any may be null: not wanted); row i of an output starts at i * stride elements (pairs of them for
// s_ampm, which holds (re, im) a bin); carrier is [units][4] = power, u re, u im, lock
struct CarrierOut {
    float *upper, *lower, *freq;
    double *sk_upper, *sk_lower;
    double *s_am, *s_pm, *s_ampm;
    double *carrier;
    size_t stride;
    bool any_row() const { return upper || lower || freq || sk_upper || sk_lower || s_am || s_pm || s_ampm; }
};

// SK of one bin from its moments (include/psdcascade.h, "spectral kurtosis cascade"): NaN below two averages and without power
PSDK_BR_HD inline double sk_estimate(uint32_t count, double s1, double s2)
{
    if (count < 2 || s1 == 0.0)
        return std::numeric_limits<double>::quiet_NaN();
    const double m = (double)count;
    return (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0);
}

// the carrier of a channel: power, u, lock.  Given: the host's P and u, lock NaN.  Else from the raw accumulators of bin 0 of
// stage 0 (carrier_from_rows of the Python package); no average there, or comp[0] == 0: (0, NaN, NaN, NaN)
struct Carrier {
    double P, ur, ui, lock;
};
// LOCK: with the lock, which only the record wants (a second square root, a division and two loads that the per-bin split and
// the band walk, which call this once a thread, do without)
template <bool LOCK = true>
PSDK_BR_HD inline Carrier carrier_of(const CarrierUnit &u)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (u.given)
        return {u.P, u.ur, u.ui, nan};
    if (!u.src0 || u.count0 < 1)
        return {0.0, nan, nan, nan};
    const double cr0 = u.src0[2 * (size_t)u.bins], ci0 = u.src0[3 * (size_t)u.bins];
    const double mag = sqrt(cr0 * cr0 + ci0 * ci0);
    if (!(mag > 0.0))
        return {0.0, nan, nan, nan};
    return {mag / ((double)u.count0 * u.n2p), cr0 / mag, ci0 / mag, LOCK ? mag / sqrt(u.src0[0] * u.src0[u.bins]) : nan};
}
// the power the AM/PM split divides by: NaN for a channel without a carrier, so that every one of its AM/PM values is NaN
PSDK_BR_HD inline double carrier_split_power(const Carrier &c) { return c.ur == c.ur ? c.P : c.ur; }

// the AM/PM split of one bin from its four f64 accumulators, the job's f32 scale and the carrier (P: carrier_split_power):
// out = s_am, s_pm, re s_ampm, im s_ampm
PSDK_BR_HD inline void ampm_split(double U, double L, double CR, double CI, float gsc, double P, double ur, double ui, double out[4])
{
    const double g = (double)gsc;
    const double Us = U * g, Ls = L * g, cr = CR * g, ci = CI * g;
    const double Dr = cr * ur + ci * ui, Di = ci * ur - cr * ui, mean = 0.5 * (Us + Ls);
    out[0] = (mean + Dr) / (2.0 * P);
    out[1] = (mean - Dr) / (2.0 * P);
    out[2] = Di / (2.0 * P);
    out[3] = (Ls - Us) / (4.0 * P);
}

// what one thread of carrier_stitch_kernel<MODE> does for element i of job j: two or four f64 loads, every requested output
template <int MODE>
PSDK_BR_HD inline void carrier_element(const CarrierReadJob &j, uint32_t i, const CarrierOut &o, const CarrierUnit *units)
{
    const uint32_t k = j.bins_start + i;
    const size_t e = (size_t)j.row * o.stride + j.start + i;
    const double U = cross_acc(j, 0, k), L = cross_acc(j, 1, k);
    if (o.upper)
        o.upper[e] = cross_scaled(U, j.gsc);
    if (o.lower)
        o.lower[e] = cross_scaled(L, j.gsc);
    if (o.freq)
        o.freq[e] = bank_freq(j, k);
    if (MODE == CREAD_SK) {
        if (o.sk_upper)
            o.sk_upper[e] = sk_estimate(j.count, U, cross_acc(j, 2, k));
        if (o.sk_lower)
            o.sk_lower[e] = sk_estimate(j.count, L, cross_acc(j, 3, k));
    }
    if (MODE == CREAD_AMPM && (o.s_am || o.s_pm || o.s_ampm)) {
        const Carrier c = carrier_of<false>(units[j.row]);
        double s[4];
        ampm_split(U, L, cross_acc(j, 2, k), cross_acc(j, 3, k), j.gsc, carrier_split_power(c), c.ur, c.ui, s);
        if (o.s_am)
            o.s_am[e] = s[0];
        if (o.s_pm)
            o.s_pm[e] = s[1];
        if (o.s_ampm) {
            o.s_ampm[2 * e] = s[2];
            o.s_ampm[2 * e + 1] = s[3];
        }
    }
}
// ... and one thread of the blocks behind the tiles for selected unit `unit`: its carrier record
PSDK_BR_HD inline void carrier_record(const CarrierUnit *units, uint32_t unit, double *carrier)
{
    const Carrier c = carrier_of(units[unit]);
    carrier[4 * (size_t)unit] = c.P;
    carrier[4 * (size_t)unit + 1] = c.ur;
    carrier[4 * (size_t)unit + 2] = c.ui;
    carrier[4 * (size_t)unit + 3] = c.lock;
}

// The values the band sums integrate.  Sides (R = 2): the stitched f32 rows upper and lower.  AM/PM (R = 4): those two, then s_am
// and s_pm of the same bin in f64, without an f32 cast.
struct CarrierSideVal {
    PSDK_BR_HD double operator()(const CarrierReadJob &j, uint32_t r, uint32_t k) const { return (double)cross_val(j, r, k); }
};
struct CarrierAmPmVal {
    double P, ur, ui;
    PSDK_BR_HD double operator()(const CarrierReadJob &j, uint32_t r, uint32_t k) const
    {
        if (r < CREAD_SIDE_ROWS)
            return (double)cross_val(j, r, k);
        double s[4];
        ampm_split(cross_acc(j, 0, k), cross_acc(j, 1, k), cross_acc(j, 2, k), cross_acc(j, 3, k), j.gsc, P, ur, ui, s);
        return s[r - CREAD_SIDE_ROWS];
    }
};
PSDK_BR_HD inline CarrierAmPmVal carrier_ampm_val(const CarrierUnit &u)
{
    const Carrier c = carrier_of<false>(u);
    return {carrier_split_power(c), c.ur, c.ui};
}

// the band sums of one channel as carrier_band_kernel<R> forms them, on the host; out is [R][BANK_MAX_BANDS]
inline void carrier_band_sides_host(const CarrierReadJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, double (*out)[BANK_MAX_BANDS])
{
    bank_band_rows_host<CREAD_SIDE_ROWS>(jobs, nj, L, bands, CarrierSideVal{}, out);
}
inline void carrier_band_ampm_host(const CarrierReadJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, const CarrierUnit &u,
                                   double (*out)[BANK_MAX_BANDS])
{
    bank_band_rows_host<CREAD_ROWS>(jobs, nj, L, bands, carrier_ampm_val(u), out);
}

// A given carrier amplitude A = (re, im) as the unit table takes it: P = re^2 + im^2 and u = (A A) / P in f64.  nullptr: good.
inline const char *carrier_given(double re, double im, CarrierUnit *u)
{
    const double P = re * re + im * im;
    if (!std::isfinite(re) || !std::isfinite(im) || !std::isfinite(P) || !(P > 0.0))
        return "a given carrier amplitude must be finite and not 0";
    u->P = P;
    u->ur = (re * re - im * im) / P;
    u->ui = (2.0 * (re * im)) / P;
    u->given = 1;
    return nullptr;
}

// carrier_readout.hip (a host build of cross_runtime.cpp has inline stand-ins).  Jobs of at most max_bins bins each; d_units is
// read in AM/PM mode alone, n_units carrier records are written when out.carrier is given.
#if defined(__HIPCC__)
hipError_t launch_carrier_stitch(int mode, const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const CarrierOut &out,
                                 const CarrierUnit *d_units, uint32_t n_units, hipStream_t s);
// one workgroup a selected channel; d_out is [n_units][bands.n][rows] f64, rows = 2 (sides) or 4 (AM/PM: d_cunits is read)
hipError_t launch_carrier_band(uint32_t rows, const CarrierReadJob *d_jobs, const BankRow *d_units, const CarrierUnit *d_cunits, uint32_t n_units,
                               const BankBands &bands, double *d_out, hipStream_t s);
#endif

} // namespace psdk
