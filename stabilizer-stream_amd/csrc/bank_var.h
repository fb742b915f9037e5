// bank_var.h -- the Var read-out (psdcv_*, include/psdcascade_var.h): what bank_var_kernel (bank_var.hip) computes for one
// element, one thread and one workgroup, and the order in which it adds.  Host and device: tests/host/bank_var_check.cpp runs
// these on the CPU.  The definition (limit, sine by an exact fold, term factor, trapezoid, sum) is the header's of include/.
//
// Every f64 product here stands next to another product or a sum; the device TU is built with -ffp-contract=off (BANK_FLAGS of
// csrc/Makefile), as bank_readout.hip is and for the same reason: each product rounds on its own.
#pragma once
#include "bank_readout.h"

#include <cmath>

namespace psdk {

constexpr uint32_t VAR_MAX_VARS = 4;    // PSDCV_MAX_VARS
constexpr uint32_t VAR_MAX_TAUS = 4096; // PSDCV_MAX_TAUS
constexpr int32_t VAR_MAX_EXP = 16;     // PSDCV_MAX_EXP
constexpr uint32_t VAR_THREADS = 256;   // four wavefronts: the order of the sum is defined for this number
constexpr uint32_t VAR_TAU_TILE = 4;    // taus a workgroup: 16 f64 sums a thread with four descriptors
constexpr double VAR_PI = 3.14159265358979323846;

// psdcv_var
struct VarDesc {
    int32_t x_exp, sinx_exp;
    float clip;
    uint32_t dc_cut;
};
static_assert(sizeof(VarDesc) == 16, "the descriptor table is copied to the device as it is");

// one caller row of the rows form
struct VarRow {
    const float *psd, *freq;
    uint32_t len, _pad;
};
static_assert(sizeof(VarRow) == 24, "the row table is copied to the device as it is");

// The element accessors.  at(e, &p, &f) is asked for non-decreasing e by one thread.
struct VarJobSrc { // a selected row of a bank: the accumulators through its jobs; nothing stitched is read
    const BankJob *jobs;
    uint32_t nj, len, ji;
    PSDK_BR_HD VarJobSrc(const BankJob *j, uint32_t n, uint32_t l) : jobs(j), nj(n), len(l), ji(0) {}
    PSDK_BR_HD void at(uint32_t e, float *p, float *f)
    {
        while (ji + 1 < nj && e >= jobs[ji + 1].start)
            ++ji;
        const BankJob &j = jobs[ji];
        const uint32_t k = j.bins_start + (e - j.start);
        *p = bank_psd(j, k);
        *f = bank_freq(j, k);
    }
};
struct VarRowSrc { // a caller row
    const float *psd, *freq;
    uint32_t len;
    PSDK_BR_HD VarRowSrc(const float *p, const float *f, uint32_t l) : psd(p), freq(f), len(l) {}
    PSDK_BR_HD void at(uint32_t e, float *p, float *f)
    {
        *p = psd[e];
        *f = freq[e];
    }
};

// sin(pi x) by the exact fold: r = fmod(x, 2.0) written as x - 2 trunc(x / 2) (the halving, the truncation, the doubling and the
// difference are all exact for a finite x, so this IS fmod), then r into [0, 0.5] with the sign kept aside.  The sine's argument
// lies in [0, pi/2] (for x >= 0): no large-argument reduction runs.
PSDK_BR_HD inline double var_sinpi(double x)
{
    double r = x - 2.0 * trunc(0.5 * x);
    bool neg = false;
    if (r > 1.0) {
        r -= 1.0;
        neg = true;
    }
    if (r > 0.5)
        r = 1.0 - r;
    const double s = sin(VAR_PI * r);
    return neg ? -s : s;
}

// square and multiply, 1 / r for a negative exponent (psdc_var_eval's, in f64)
PSDK_BR_HD inline double var_powi(double x, int32_t e)
{
    uint32_t u = (uint32_t)(e < 0 ? -e : e);
    double r = 1.0, b = x;
    while (u) {
        if (u & 1u)
            r *= b;
        b *= b;
        u >>= 1;
    }
    return e < 0 ? 1.0 / r : r;
}

// a[e] of every descriptor for one element and one tau: the sine and w once, shared by the descriptors
PSDK_BR_HD inline void var_terms(float p, float f, float tau, const VarDesc *vars, uint32_t nv, double a[VAR_MAX_VARS])
{
    const double fd = (double)f, x = fd * (double)tau, w = VAR_PI * x, s = var_sinpi(x);
    const double sy = ((double)p * fd) * fd;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
        a[v] = v < nv ? sy * (var_powi(s, vars[v].sinx_exp) * var_powi(w, vars[v].x_exp)) : 0.0;
}

// t[e], or +0.0 for an element outside [dc_cut, E); (a1, f1) belong to element e - 1 and are not looked at for e == dc_cut
PSDK_BR_HD inline double var_trapezoid(double a, double a1, float f, float f1, uint32_t e, uint32_t dc_cut, uint32_t E)
{
    if (e < dc_cut || e >= E)
        return 0.0;
    if (e == dc_cut)
        return (a + 0.0) * ((double)f - 0.0);
    return (a + a1) * ((double)f - (double)f1);
}

// The limit search of thread t of T: over its elements e = t, t + T, ... < L the first e >= dc_cut with !(f[e] <= lim), per
// descriptor and tau of the tile; `first` starts at L.  E is the smallest of these over the threads: the first violation ends the
// row wherever f steps back later.  (A job's f is monotone in the bin, so E is also the smallest per-job first violation; the
// search here asks nothing of f and so serves caller rows as well.)
template <class Src>
PSDK_BR_HD inline void var_limit_walk(Src src, uint32_t t, uint32_t T, const VarDesc *vars, uint32_t nv,
                                      const float (*lim)[VAR_TAU_TILE], uint32_t (*first)[VAR_TAU_TILE])
{
    for (uint32_t e = t; e < src.len; e += T) {
        float p, f;
        src.at(e, &p, &f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
                if (v < nv && e >= vars[v].dc_cut && !(f <= lim[v][j]) && e < first[v][j])
                    first[v][j] = e;
    }
}

// One tau tile of one row as bank_var_kernel forms it, on the host: the limits in f32, E per descriptor and tau, then round by
// round the VAR_THREADS threads (thread t on element round * VAR_THREADS + t, rounds while an element below the largest E is
// left), each adding its trapezoid into its own sum; then within each wavefront the tree v[l] += v[l + off] for off = 32, 16 ...
// 1, then the wavefronts in order.  tau[] holds the tile's VAR_TAU_TILE taus (a tile at the end repeats the last tau).
template <class Src>
inline void bank_var_tile_host(Src src, const VarDesc *vars, uint32_t nv, const float tau[VAR_TAU_TILE],
                               double (*out)[VAR_TAU_TILE])
{
    const uint32_t L = src.len;
    float lim[VAR_MAX_VARS][VAR_TAU_TILE];
    uint32_t E[VAR_MAX_VARS][VAR_TAU_TILE];
    uint32_t e_max = 0;
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
            lim[v][j] = v < nv ? vars[v].clip / tau[j] : 0.0f;
            E[v][j] = L;
        }
    var_limit_walk(src, 0, 1, vars, nv, lim, E);
    for (uint32_t v = 0; v < nv; ++v)
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
            if (E[v][j] > vars[v].dc_cut && E[v][j] > e_max)
                e_max = E[v][j];
    static double acc[VAR_THREADS][VAR_MAX_VARS][VAR_TAU_TILE];
    for (uint32_t t = 0; t < VAR_THREADS; ++t)
        for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
            for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
                acc[t][v][j] = 0.0;
    double a1[VAR_TAU_TILE][VAR_MAX_VARS] = {}; // of the element before
    float f1 = 0.0f;
    for (uint32_t e = 0; e < e_max; ++e) { // (element by element: thread e % VAR_THREADS in round e / VAR_THREADS)
        float p, f;
        src.at(e, &p, &f);
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
            double a[VAR_MAX_VARS];
            var_terms(p, f, tau[j], vars, nv, a);
            for (uint32_t v = 0; v < VAR_MAX_VARS; ++v) {
                acc[e % VAR_THREADS][v][j] += var_trapezoid(a[v], a1[j][v], f, f1, e, v < nv ? vars[v].dc_cut : 0, v < nv ? E[v][j] : 0);
                a1[j][v] = a[v];
            }
        }
        f1 = f;
    }
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
            double sum = 0.0;
            for (uint32_t w = 0; w < VAR_THREADS / BANK_WAVE; ++w) {
                double x[BANK_WAVE];
                for (uint32_t l = 0; l < BANK_WAVE; ++l)
                    x[l] = acc[w * BANK_WAVE + l][v][j];
                for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
                    for (uint32_t l = 0; l < off; ++l)
                        x[l] += x[l + off];
                sum = w ? sum + x[0] : x[0];
            }
            out[v][j] = sum;
        }
}

// A whole row on the host: out is [nv][nt]
template <class Src>
inline void bank_var_row_host(Src src, const VarDesc *vars, uint32_t nv, const float *taus, uint32_t nt, double *out)
{
    for (uint32_t j0 = 0; j0 < nt; j0 += VAR_TAU_TILE) {
        float tau[VAR_TAU_TILE];
        double r[VAR_MAX_VARS][VAR_TAU_TILE];
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
            tau[j] = taus[j0 + j < nt ? j0 + j : nt - 1];
        bank_var_tile_host(src, vars, nv, tau, r);
        for (uint32_t v = 0; v < nv; ++v)
            for (uint32_t j = 0; j < VAR_TAU_TILE && j0 + j < nt; ++j)
                out[(size_t)v * nt + j0 + j] = r[v][j];
    }
}

#if defined(__HIPCC__)
// bank_var.hip.  One workgroup a (row, tau tile); d_out is [n_rows][nv][nt] f64.  Exactly one of (d_jobs, d_rows) and d_vrows is given.
hipError_t launch_bank_var(const BankJob *d_jobs, const BankRow *d_rows, const VarRow *d_vrows, uint32_t n_rows, const VarDesc *d_vars,
                           uint32_t nv, const float *d_taus, uint32_t nt, double *d_out, hipStream_t s);
#endif

} // namespace psdk
