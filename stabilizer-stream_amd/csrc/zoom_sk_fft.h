// zoom_sk_fft.h -- the per-slot arithmetic and the row layout of the zoom spectral kurtosis kernel (zoom_sk.hip).
//
// A segment of a channel is one complex transform Z of I + i Q, as in zoom_kernel.  A thread holds sixteen bins of it in registers
// (bin freq_of_slot<N>(t, s) in slot s) and adds, with P = |Z|^2 and w the segment's averaging weight (sk_weight, sk_fft.h),
//     a1[s] += w P,        a2[s] += (w P) P.
// The transform runs with amplitude 1 and the weight goes on the products, in the order (w P) P, for the reasons sk_fft.h
// gives: nothing is squared twice, nothing is divided by, and a weight that underflows to 0 gives 0 in both moments.
// Nothing is separated and nothing is subtracted across bins: EVERY bin of the complex stream is complex, so circular Gaussian
// noise reads SK = 1 at offset 0 and at Nyquist as well -- the "2 at the real-valued bins" of the real object does not occur.
// Row layout of a workgroup partial and of a stage's accumulators, four rows of N/2 + 1 (include/psdcascade.h):
//     row 2 q + 0 (upper): bin k,    row 2 q + 1 (lower): bin (N - k) mod N;    q = 0 S1 = sum w P, 1 S2 = sum w P^2
// so rows 0 and 1 are zoom_kernel's upper and lower (two_sided_bin, two_sided_value of segment_kernel.h).
// Range: a workgroup's partial rows are f32, so the sum of P^2 over its segments must stay below f32 max.
//
// Everything here is __host__ __device__: tests/host/zoom_sk_emul.cpp runs it lane by lane against an f64 DFT.
#pragma once
#include "sk_fft.h"

namespace psdk {

constexpr int ZSK_Q = 2;            // moments a bin: S1, S2
constexpr int ZSK_ROWS = 2 * ZSK_Q; // rows of a partial: upper and lower of each moment

// add one bin z of a segment with the weight w to its two accumulators
PSDK_HD void zoom_sk_slot(cf z, float w, float &a1, float &a2)
{
    const float p = z.re * z.re + z.im * z.im;
    const float wp = w * p;
    a1 += wp;
    a2 += wp * p;
}

} // namespace psdk
