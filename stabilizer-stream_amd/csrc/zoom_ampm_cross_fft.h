// zoom_ampm_cross_fft.h -- the per-bin arithmetic and the row layout of the AM/PM cross kernel (zoom_ampm_cross.hip).
//
// A segment of a pair is two complex transforms of the same N samples: Z_a of channel a's I + i Q and Z_b of channel b's.  The team
// leaves each in an LDS frame of its own in natural order (store_natural, cross_fft.h: bin k at LdsFrame<N>::at(k)) and a thread
// adds, for each bin k = t + TEAM r <= N/2 it owns (CrossBins<N>, as cross_kernel's threads own theirs), with kn = (N - k) mod N,
// a = Z_a[k], an = Z_a[kn], b = Z_b[k], bn = Z_b[kn]:
//     acc[0]  += |a|^2                acc[1]  += |an|^2               S_aa upper / lower
//     acc[2]  += |b|^2                acc[3]  += |bn|^2               S_bb upper / lower
//     acc[4]  += Re conj(a) b         acc[5]  += Re conj(an) bn       Re S_ab upper / lower     (zoom_cross_bin's sums)
//     acc[6]  += Im conj(a) b         acc[7]  += Im conj(an) bn       Im S_ab upper / lower
//     acc[8]  += Re a bn              acc[9]  += Im a bn              cab[k] = Z_a[k] Z_b[kn]   WITHOUT a conjugate
//     acc[10] += Re an b              acc[11] += Im an b              cba[k] = Z_a[kn] Z_b[k]   WITHOUT a conjugate
// each sum formed left to right and then added to the accumulator.  At k = 0 and k = N/2 kn == k: upper and lower rows are equal
// there and cab == cba.  All twelve are bilinear in Z, so a segment's averaging weight w goes on the samples as the amplitude
// sqrt(w) (cross_amp, cross_channel.h), exactly as zoom_cross_kernel does it; nothing here knows the weight.
// Row layout of a workgroup partial and of a stage's accumulators, twelve rows of N/2 + 1 (include/psdcascade.h): row c at index k
// is acc[c] of bin k -- rows 0 ... 7 are the zoom cross object's eight, in its order and with its signs.
//
// Everything here is __host__ __device__: tests/host/zoom_ampm_cross_emul.cpp runs it lane by lane against an f64 DFT.
#pragma once
#include "cross_fft.h"

namespace psdk {

constexpr int ZXAMPM_ROWS = 12; // rows of a partial
constexpr int ZXAMPM_TURN = 4;  // rows that go through the frames' LDS at a time at the end of the kernel

// the zero-defaulted variant field of CsmBatch that launch_zoom_cross dispatches on (zoom_cross.hip)
constexpr int ZCROSS_VARIANT_CSD = 0;   // zoom_cross_kernel: eight rows
constexpr int ZCROSS_VARIANT_AMPM = 1;  // zoom_ampm_cross_kernel: twelve rows

// the transform bin that pairs with bin k (0 ... N/2)
template <int N>
PSDK_HD int xampm_partner(int k)
{
    return (N - k) & (N - 1);
}

// add bin k (0 ... N/2) of the pair's segment, held in the natural-order frames fa (channel a) and fb (channel b), to its twelve
// accumulators
template <int N>
PSDK_HD void ampm_cross_bin(int k, const cf *fa, const cf *fb, float *acc)
{
    const int kn = xampm_partner<N>(k);
    const cf a = lds_ld(fa + LdsFrame<N>::at(k));
    const cf an = lds_ld(fa + LdsFrame<N>::at(kn));
    const cf b = lds_ld(fb + LdsFrame<N>::at(k));
    const cf bn = lds_ld(fb + LdsFrame<N>::at(kn));
    acc[0] += a.re * a.re + a.im * a.im;
    acc[1] += an.re * an.re + an.im * an.im;
    acc[2] += b.re * b.re + b.im * b.im;
    acc[3] += bn.re * bn.re + bn.im * bn.im;
    acc[4] += a.re * b.re + a.im * b.im;
    acc[5] += an.re * bn.re + an.im * bn.im;
    acc[6] += a.re * b.im - a.im * b.re;
    acc[7] += an.re * bn.im - an.im * bn.re;
    acc[8] += a.re * bn.re - a.im * bn.im;
    acc[9] += a.re * bn.im + a.im * bn.re;
    acc[10] += an.re * b.re - an.im * b.im;
    acc[11] += an.re * b.im + an.im * b.re;
}

} // namespace psdk
