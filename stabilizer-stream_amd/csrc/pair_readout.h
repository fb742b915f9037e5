// pair_readout.h -- the bank read-out of the four pair carrier kinds (psdcpr_*, include/ext/psdcascade_pairread.h: the zoom cross, IQ
// cross and zoom / IQ AM/PM cross objects, 8 or 12 f64 rows a stage): the unit table, the argument rules, and what
// pair_stitch_kernel and pair_band_kernel (pair_readout.hip) compute for one element and one thread.  The jobs (CarrierReadJob),
// the two f32 factors, the band walk and its reduction order are those of carrier_readout.h / cross_readout.h / bank_readout.h.
// Host and device: tests/host/pair_readout_check.cpp runs these on the CPU.
// Every f64 product here stands next to a sum: the device TU is built with -ffp-contract=off (csrc/Makefile), as bank_readout.hip.
#pragma once
#include "carrier_readout.h"

#include <cmath>
#include <limits>

namespace psdk {

constexpr uint32_t PREAD_CSD_ROWS = 8;  // S_aa up, lo; S_bb up, lo; Re S_ab up, lo; Im S_ab up, lo
constexpr uint32_t PREAD_ROWS = 12;     // those, then Re cab, Im cab, Re cba, Im cba
constexpr uint32_t PREAD_BAND_ROWS = 8; // columns of a band sum in either mode
constexpr uint32_t PREAD_BAND_KERNEL_ROWS = 8; // rows a workgroup of pair_band_kernel takes (8 or 4: DESIGN.md section 4.7)
constexpr int PREAD_CSD = 0, PREAD_AMPM = 1; // the modes of pair_stitch_kernel
constexpr uint32_t PREAD_RECORD = 7;    // p_ab, re w, im w, re q, im q, lock_w, lock_q

// one selected pair of an AM/PM call: where its carriers come from
struct PairUnit {
    const double *src0;        // stage 0's accumulator [12][bins] (null: the pair has no stage)
    double n2p;                // (double)n * (double)n * (double)power, power the object's f32 window power
    double P, wr, wi, qr, qi;  // given != 0: p_ab and the unit phasors w, q from the host
    uint32_t count0;           // the count stage 0 reports
    uint32_t given;
    uint32_t bins, _pad;
};
static_assert(sizeof(PairUnit) == 72, "the unit table is copied to the device as it is");

// where a CSD call's rows go (any may be null: not wanted); row i of an output starts at i * stride elements (pairs of them for
// sab_*, h1_*, which hold (re, im) a bin)
struct PairCsdOut {
    float *saa_up, *saa_lo, *sbb_up, *sbb_lo, *sab_up, *sab_lo, *freq;
    double *coh_up, *coh_lo, *h1_up, *h1_lo;
    size_t stride;
    bool any_row() const { return saa_up || saa_lo || sbb_up || sbb_lo || sab_up || sab_lo || freq || coh_up || coh_lo || h1_up || h1_lo; }
};
// ... and an AM/PM call's: all but freq are (re, im) a bin; carrier is [units][PREAD_RECORD]
struct PairAmPmOut {
    float *freq;
    double *cab, *cba, *s_am, *s_pm, *s_am_pm, *s_pm_am;
    double *carrier;
    size_t stride;
    PSDK_BR_HD bool split() const { return s_am || s_pm || s_am_pm || s_pm_am; }
    bool any_row() const { return freq || cab || cba || split(); }
};

// the carriers of a pair.  Given: the host's P, w, q, locks NaN.  Else from the raw accumulators of bin 0 of stage 0
// (carriers_from_rows of the Python package); no average there, or sab_up[0] == 0 or cab[0] == 0: (0, NaN x 6)
struct PairCarrier {
    double P, wr, wi, qr, qi, lock_w, lock_q;
};
// LOCK: with the locks, which only the record wants (two more square roots, two divisions and three loads)
template <bool LOCK = true>
PSDK_BR_HD inline PairCarrier pair_carrier_of(const PairUnit &u)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (u.given)
        return {u.P, u.wr, u.wi, u.qr, u.qi, nan, nan};
    if (!u.src0 || u.count0 < 1)
        return {0.0, nan, nan, nan, nan, nan, nan};
    const size_t B = u.bins;
    const double ur = u.src0[4 * B], ui = u.src0[6 * B], cr = u.src0[8 * B], ci = u.src0[9 * B];
    const double mu = sqrt(ur * ur + ui * ui), mc = sqrt(cr * cr + ci * ci);
    if (!(mu > 0.0) || !(mc > 0.0))
        return {0.0, nan, nan, nan, nan, nan, nan};
    return {mu / ((double)u.count0 * u.n2p), ur / mu, ui / mu, cr / mc, ci / mc,
            LOCK ? mu / sqrt(u.src0[0] * u.src0[2 * B]) : nan, LOCK ? mc / sqrt(u.src0[0] * u.src0[3 * B]) : nan};
}

// what the per-bin split takes of the carriers: P is NaN for a pair without carriers, so that every one of its AM/PM values is NaN
struct PairSplit {
    double P, wr, wi, qr, qi;
};
PSDK_BR_HD inline PairSplit pair_split_of(const PairUnit &u)
{
    const PairCarrier c = pair_carrier_of<false>(u);
    return {c.wr == c.wr ? c.P : c.wr, c.wr, c.wi, c.qr, c.qi};
}

// The AM/PM cross split of one bin from its eight f64 accumulators a[] = rows 4 ... 11 at the bin, the job's f32 scale and the
// carriers: out = (re, im) of s_am, s_pm, s_am_pm, s_pm_am (am_pm_cross_from_sidebands of the Python package in real operations)
PSDK_BR_HD inline void pair_ampm_split(const double a[8], float gsc, const PairSplit &c, double out[8])
{
    const double g = (double)gsc;
    const double Ur = a[0] * g, Lr = a[1] * g, Ui = a[2] * g, Li = a[3] * g;
    const double Cr = a[4] * g, Ci = a[5] * g, Br = a[6] * g, Bi = a[7] * g;
    const double t1r = Ur * c.wr + Ui * c.wi, t1i = Ui * c.wr - Ur * c.wi;
    const double t2r = Cr * c.qr + Ci * c.qi, t2i = Cr * c.qi - Ci * c.qr;
    const double t3r = Br * c.qr + Bi * c.qi, t3i = Bi * c.qr - Br * c.qi;
    const double t4r = Lr * c.wr + Li * c.wi, t4i = Lr * c.wi - Li * c.wr;
    const double d = 4.0 * c.P;
    out[0] = (((t1r + t2r) + t3r) + t4r) / d;
    out[1] = (((t1i + t2i) + t3i) + t4i) / d;
    out[2] = (((t1r - t2r) - t3r) + t4r) / d;
    out[3] = (((t1i - t2i) - t3i) + t4i) / d;
    const double xr = ((t1r - t2r) + t3r) - t4r, xi = ((t1i - t2i) + t3i) - t4i;
    const double yr = ((t1r + t2r) - t3r) - t4r, yi = ((t1i + t2i) - t3i) - t4i;
    out[4] = xi / d;
    out[5] = -xr / d;
    out[6] = -yi / d;
    out[7] = yr / d;
}
// rows 4 ... 11 of bin k of a 12-row job, in row order
PSDK_BR_HD inline void pair_cross_rows(const CarrierReadJob &j, uint32_t k, double a[8])
{
    for (uint32_t r = 0; r < 8; ++r)
        a[r] = cross_acc(j, 4 + r, k);
}

// what one thread of pair_stitch_kernel<PREAD_CSD> does for element i of job j: the rows its outputs need, every requested output
PSDK_BR_HD inline void pair_csd_element(const CarrierReadJob &j, uint32_t i, const PairCsdOut &o)
{
    const uint32_t k = j.bins_start + i;
    const size_t e = (size_t)j.row * o.stride + j.start + i;
    const bool up = o.coh_up || o.h1_up, lo = o.coh_lo || o.h1_lo;
    double aa_u = 0, aa_l = 0, bb_u = 0, bb_l = 0, re_u = 0, re_l = 0, im_u = 0, im_l = 0;
    if (o.saa_up || up)
        aa_u = cross_acc(j, 0, k);
    if (o.saa_lo || lo)
        aa_l = cross_acc(j, 1, k);
    if (o.sbb_up || o.coh_up)
        bb_u = cross_acc(j, 2, k);
    if (o.sbb_lo || o.coh_lo)
        bb_l = cross_acc(j, 3, k);
    if (o.sab_up || up) {
        re_u = cross_acc(j, 4, k);
        im_u = cross_acc(j, 6, k);
    }
    if (o.sab_lo || lo) {
        re_l = cross_acc(j, 5, k);
        im_l = cross_acc(j, 7, k);
    }
    if (o.saa_up)
        o.saa_up[e] = cross_scaled(aa_u, j.gsc);
    if (o.saa_lo)
        o.saa_lo[e] = cross_scaled(aa_l, j.gsc);
    if (o.sbb_up)
        o.sbb_up[e] = cross_scaled(bb_u, j.gsc);
    if (o.sbb_lo)
        o.sbb_lo[e] = cross_scaled(bb_l, j.gsc);
    if (o.sab_up) {
        o.sab_up[2 * e] = cross_scaled(re_u, j.gsc);
        o.sab_up[2 * e + 1] = cross_scaled(im_u, j.gsc);
    }
    if (o.sab_lo) {
        o.sab_lo[2 * e] = cross_scaled(re_l, j.gsc);
        o.sab_lo[2 * e + 1] = cross_scaled(im_l, j.gsc);
    }
    if (o.freq)
        o.freq[e] = bank_freq(j, k);
    if (o.coh_up)
        o.coh_up[e] = cross_coherence(aa_u, bb_u, re_u, im_u);
    if (o.coh_lo)
        o.coh_lo[e] = cross_coherence(aa_l, bb_l, re_l, im_l);
    if (o.h1_up)
        cross_transfer(aa_u, re_u, im_u, o.h1_up + 2 * e);
    if (o.h1_lo)
        cross_transfer(aa_l, re_l, im_l, o.h1_lo + 2 * e);
}

// ... and of pair_stitch_kernel<PREAD_AMPM>: cab / cba alone need four loads, the split all eight of rows 4 ... 11
PSDK_BR_HD inline void pair_ampm_element(const CarrierReadJob &j, uint32_t i, const PairAmPmOut &o, const PairUnit *units)
{
    const uint32_t k = j.bins_start + i;
    const size_t e = (size_t)j.row * o.stride + j.start + i;
    const double g = (double)j.gsc;
    if (o.freq)
        o.freq[e] = bank_freq(j, k);
    if (o.split()) {
        double a[8], s[8];
        pair_cross_rows(j, k, a);
        pair_ampm_split(a, j.gsc, pair_split_of(units[j.row]), s);
        if (o.cab) {
            o.cab[2 * e] = a[4] * g;
            o.cab[2 * e + 1] = a[5] * g;
        }
        if (o.cba) {
            o.cba[2 * e] = a[6] * g;
            o.cba[2 * e + 1] = a[7] * g;
        }
        if (o.s_am) {
            o.s_am[2 * e] = s[0];
            o.s_am[2 * e + 1] = s[1];
        }
        if (o.s_pm) {
            o.s_pm[2 * e] = s[2];
            o.s_pm[2 * e + 1] = s[3];
        }
        if (o.s_am_pm) {
            o.s_am_pm[2 * e] = s[4];
            o.s_am_pm[2 * e + 1] = s[5];
        }
        if (o.s_pm_am) {
            o.s_pm_am[2 * e] = s[6];
            o.s_pm_am[2 * e + 1] = s[7];
        }
        return;
    }
    if (o.cab) {
        o.cab[2 * e] = cross_acc(j, 8, k) * g;
        o.cab[2 * e + 1] = cross_acc(j, 9, k) * g;
    }
    if (o.cba) {
        o.cba[2 * e] = cross_acc(j, 10, k) * g;
        o.cba[2 * e + 1] = cross_acc(j, 11, k) * g;
    }
}
// ... and one thread of the blocks behind the tiles for selected pair `unit`: its carrier record
PSDK_BR_HD inline void pair_record(const PairUnit *units, uint32_t unit, double *carrier)
{
    const PairCarrier c = pair_carrier_of(units[unit]);
    double *r = carrier + PREAD_RECORD * (size_t)unit;
    r[0] = c.P;
    r[1] = c.wr;
    r[2] = c.wi;
    r[3] = c.qr;
    r[4] = c.qi;
    r[5] = c.lock_w;
    r[6] = c.lock_q;
}

// The values the band sums integrate; `row0` is the first of the R rows a workgroup takes (pair_band_kernel).  CSD: the stitched
// f32 rows 0 ... 7.  AM/PM: (re, im) of s_am, s_pm, s_am_pm, s_pm_am of the bin in f64, without an f32 cast.
struct PairCsdVal {
    uint32_t row0;
    PSDK_BR_HD double operator()(const CarrierReadJob &j, uint32_t r, uint32_t k) const { return (double)cross_val(j, row0 + r, k); }
};
struct PairAmPmVal {
    PairSplit c;
    uint32_t row0;
    PSDK_BR_HD double operator()(const CarrierReadJob &j, uint32_t r, uint32_t k) const
    {
        double a[8], s[8];
        pair_cross_rows(j, k, a);
        pair_ampm_split(a, j.gsc, c, s);
        return s[row0 + r];
    }
};

// the band sums of one pair as pair_band_kernel forms them, on the host; out is [PREAD_BAND_ROWS][BANK_MAX_BANDS]
inline void pair_band_csd_host(const CarrierReadJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, double (*out)[BANK_MAX_BANDS])
{
    bank_band_rows_host<PREAD_BAND_ROWS>(jobs, nj, L, bands, PairCsdVal{0}, out);
}
inline void pair_band_ampm_host(const CarrierReadJob *jobs, uint32_t nj, uint32_t L, const BankBands &bands, const PairUnit &u,
                                double (*out)[BANK_MAX_BANDS])
{
    bank_band_rows_host<PREAD_BAND_ROWS>(jobs, nj, L, bands, PairAmPmVal{pair_split_of(u), 0}, out);
}

// Given carriers c = (p_ab, re w, im w, re q, im q) as the unit table takes them: w and q divided by their magnitude, as
// am_pm_cross_from_sidebands does.  nullptr: good.
inline const char *pair_given(const double c[5], PairUnit *u)
{
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(c[i]))
            return "given carriers must be finite, with p_ab > 0 and w, q not 0";
    const double mw = std::hypot(c[1], c[2]), mq = std::hypot(c[3], c[4]);
    if (!(c[0] > 0.0) || !(mw > 0.0) || !(mq > 0.0) || !std::isfinite(mw) || !std::isfinite(mq))
        return "given carriers must be finite, with p_ab > 0 and w, q not 0";
    u->P = c[0];
    u->wr = c[1] / mw;
    u->wi = c[2] / mw;
    u->qr = c[3] / mq;
    u->qi = c[4] / mq;
    u->given = 1;
    return nullptr;
}

// pair_readout.hip (a host build of cross_runtime.cpp has inline stand-ins).  Jobs of at most max_bins bins each; d_units is read
// in AM/PM mode alone, n_units carrier records are written when out.carrier is given.
#if defined(__HIPCC__)
hipError_t launch_pair_stitch_csd(const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const PairCsdOut &out, hipStream_t s);
hipError_t launch_pair_stitch_ampm(const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const PairAmPmOut &out,
                                   const PairUnit *d_units, uint32_t n_units, hipStream_t s);
// d_out is [n_units][bands.n][8] f64; mode PREAD_AMPM reads d_punits
hipError_t launch_pair_band(int mode, const CarrierReadJob *d_jobs, const BankRow *d_units, const PairUnit *d_punits, uint32_t n_units,
                            const BankBands &bands, double *d_out, hipStream_t s);
#endif

} // namespace psdk
