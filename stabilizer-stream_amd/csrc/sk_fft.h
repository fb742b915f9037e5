// sk_fft.h -- the per-bin arithmetic of the spectral kurtosis kernel (sk.hip): the first and second moment of the periodogram.
//
// A team transforms z = a + i b, a and b two consecutive segments of ONE real stream, exactly as the pair kernel does for a
// channel (cross_fft.h: team transform, natural-order store, separation of bins k and N - k).  Per owned bin k = 0 ... N/2 and
// segment, with P = |X[k]|^2 and w the segment's averaging weight,
//     row 0 (S1) += w P,        row 1 (S2) += w P^2.
// Weights.  The pair kernel carries the EWMA weight as an AMPLITUDE sqrt(w) on the windowed samples, so its |X|^2 is already
// w P.  Squaring that gives w^2 P^2, and recovering w P^2 from it means dividing by a weight that underflows for the oldest
// segments of a long job.  Here the transform runs with amplitude 1 instead, P is the plain periodogram, and both products are
// weighted afterwards: wp = w P, then wp and wp P.  (w P) P is the order: P P alone overflows f32 at P > 1.8e19 where the
// weighted product still fits, and a weight that underflows to 0 gives 0 in both rows, never a division.
// Range: a workgroup's partial rows are f32, so the sum of P^2 over its segments must stay below f32 max.
//
// Everything here is __host__ __device__: tests/host/sk_emul.cpp runs it lane by lane against an f64 DFT.
#pragma once
#include "cross_fft.h"

#include <cmath>

namespace psdk {

constexpr int SK_ROWS = 2; // S1, S2

// element of a workgroup's partial (and of a stage's accumulator): [SK_ROWS][n/2 + 1]
template <int N>
PSDK_HD int sk_row_at(int row, int k)
{
    return row * (N / 2 + 1) + k;
}

// the averaging weight of the job's segment `step` (1-based within the job): 1 while the stage averages as a boxcar, then
// gamma^(segments that follow it in the job) -- the square of the amplitude cross_amp gives the pair kernel
template <class Job>
PSDK_HD float sk_weight(const Job &job, int step)
{
    const int m = step > job.is_m1 ? step : job.is_m1;
    const int na = job.nb - m;
    if (na <= 0)
        return 1.0f;
    return (float)exp2((double)na * job.log2_gamma);
}

// Add bin k of the two segments held in the natural-order frame f, with the weights wa, wb:
//   acc[0] += wa Pa + wb Pb,   acc[1] += (wa Pa) Pa + (wb Pb) Pb.
// b_live = false: segment b does not exist (the odd last segment of a job); its separated bin is dropped.
template <int N>
PSDK_HD void sk_bin(int k, const cf *f, float wa, float wb, bool b_live, float *acc)
{
    const int kn = (N - k) & (N - 1);
    cf a, b;
    separate(lds_ld(f + LdsFrame<N>::at(k)), lds_ld(f + LdsFrame<N>::at(kn)), a, b);
    if (!b_live)
        b = {0.0f, 0.0f};
    const float pa = a.re * a.re + a.im * a.im, pb = b.re * b.re + b.im * b.im;
    const float wpa = wa * pa, wpb = wb * pb;
    acc[0] += wpa + wpb;
    acc[1] += wpa * pa + wpb * pb;
}

} // namespace psdk
