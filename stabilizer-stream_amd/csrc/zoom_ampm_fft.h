// zoom_ampm_fft.h -- the per-bin arithmetic and the row layout of the AM/PM kernel (zoom_ampm.hip).
//
// A segment of a channel is one complex transform Z of I + i Q, as in zoom_kernel.  The team leaves it in its LDS frame in natural
// order (store_natural, cross_fft.h: bin k at LdsFrame<N>::at(k)) and a thread adds, for each bin k = t + TEAM r <= N/2 it owns
// (CrossBins<N>, as cross_kernel's threads own theirs), with kn = (N - k) mod N, a = Z[k] and b = Z[kn]:
//     acc[0] += a.re a.re + a.im a.im                       upper     |Z_k|^2
//     acc[1] += b.re b.re + b.im b.im                       lower     |Z_kn|^2
//     acc[2] += a.re b.re - a.im b.im                       comp_re   Re(Z_k Z_kn)
//     acc[3] += a.re b.im + a.im b.re                       comp_im   Im(Z_k Z_kn)
// each sum formed left to right and then added to the accumulator.  The last two are the complementary spectrum: a product WITHOUT
// a conjugate.  At k = 0 and k = N/2 kn == k and it is Z_k^2; rows 0 and 1 are then equal.
// All four are bilinear in Z, so a segment's averaging weight w goes on the samples as the amplitude sqrt(w) (cross_amp,
// cross_channel.h), exactly as zoom_kernel does it; nothing here knows the weight.
// Row layout of a workgroup partial and of a stage's accumulators, four rows of N/2 + 1 (include/psdcascade.h): row c at index k
// is acc[c] of bin k -- rows 0 and 1 are zoom_kernel's upper and lower.
//
// Everything here is __host__ __device__: tests/host/zoom_ampm_emul.cpp runs it lane by lane against an f64 DFT.
#pragma once
#include "cross_fft.h"

namespace psdk {

constexpr int ZAMPM_ROWS = 4; // rows of a partial: upper, lower, comp_re, comp_im

// the transform bin that pairs with bin k (0 ... N/2) in rows 1 ... 3
template <int N>
PSDK_HD int ampm_partner(int k)
{
    return (N - k) & (N - 1);
}

// add bin k (0 ... N/2) of the segment held in the natural-order frame to its four accumulators
template <int N>
PSDK_HD void ampm_bin(int k, const cf *frame, float *acc)
{
    const cf a = lds_ld(frame + LdsFrame<N>::at(k));
    const cf b = lds_ld(frame + LdsFrame<N>::at(ampm_partner<N>(k)));
    acc[0] += a.re * a.re + a.im * a.im;
    acc[1] += b.re * b.re + b.im * b.im;
    acc[2] += a.re * b.re - a.im * b.im;
    acc[3] += a.re * b.im + a.im * b.re;
}

} // namespace psdk
