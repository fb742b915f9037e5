// zoom_cross_fft.h -- the per-bin arithmetic and the row layout of the zoom cross kernel (zoom_cross.hip).
//
// A segment of a pair is two complex transforms of the same N samples: Z_a of channel a's I + i Q and Z_b of channel b's.  A
// thread holds the same sixteen bins of both in registers (bin freq_of_slot<N>(t, s) in slot s) and adds four values a bin:
//     S_aa = |Z_a|^2,   S_bb = |Z_b|^2,   S_ab = conj(Z_a) Z_b   (Re and Im; the sign of cross_bin and csm_bin)
// Nothing is separated and nothing is subtracted across bins: bin j of the transform IS the spectrum at f0 + j / N (j <= N/2)
// or at f0 - (N - j) / N, and the row layout below only says where bin j is read out.
// Row layout of a workgroup partial and of a stage's accumulators, eight rows of N/2 + 1 (include/psdcascade.h):
//     row 2 q + 0 (upper): bin k,    row 2 q + 1 (lower): bin (N - k) mod N, not conjugated;    q = 0 S_aa, 1 S_bb, 2 Re S_ab, 3 Im S_ab
// (two_sided_bin, two_sided_value of segment_kernel.h; q is acc's index below)
//
// Everything here is __host__ __device__: tests/host/zoom_cross_emul.cpp runs it against an f64 DFT.
#pragma once
#include "cross_fft.h"

namespace psdk {

constexpr int ZCROSS_Q = 4;               // values a bin
constexpr int ZCROSS_ROWS = 2 * ZCROSS_Q; // rows of a partial: upper and lower of each value

// add one bin of the two spectra to its four accumulators: acc[0] S_aa, acc[1] S_bb, acc[2] Re S_ab, acc[3] Im S_ab, each
// `stride` floats from the one before (a thread keeps acc[q][slot])
PSDK_HD void zoom_cross_bin(cf za, cf zb, float *acc, int stride)
{
    acc[0] += za.re * za.re + za.im * za.im;
    acc[stride] += zb.re * zb.re + zb.im * zb.im;
    acc[2 * stride] += za.re * zb.re + za.im * zb.im;
    acc[3 * stride] += za.re * zb.im - za.im * zb.re;
}

} // namespace psdk
