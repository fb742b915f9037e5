// cross_fft.h -- the per-lane transform and two-for-one separation of the cross-spectral kernel (cross.hip).
//
// A team of N/E threads transforms z = a + i b, a and b two consecutive segments of ONE channel (they share its scale), with the
// radix passes of fft_core.h.  Unlike the power-only kernels the outputs are used with their phase, so the last pass reads its
// inputs unrotated and its outputs go back to the LDS frame in natural bin order (store_natural).  Bins k and N - k then give
//     A[k] = (Z[k] + conj Z[N-k]) / 2,    B[k] = (Z[k] - conj Z[N-k]) / (2i),
// and the products conj(X) Y are formed per segment.  The two channels are never packed into one transform: Y separated from
// x + i y carries an error of order eps |x|, which a channel 1e-4 the size of the other does not survive.
//
// Everything here is __host__ __device__: tests/host/cross_emul.cpp runs it lane by lane against an f64 DFT.
#pragma once
#include "fft_core.h"

namespace psdk {

// pass P of the team transform on the thread's registers: read the pass inputs (P > 0, unrotated), butterflies and twiddles,
// write the outputs back in place unless it is the last pass.  A thread writes exactly the frame slots it read, so a pass needs
// no barrier between its reads and writes; between passes the team synchronises.
template <int N, int P>
PSDK_HD void xfft_pass(int t, cf *v, cf *frame, const cf *tw)
{
    using PI = PassInfo<N, P>;
    if constexpr (P > 0)
        pass_load<N, P>(t, v, frame, 0);
    pass_compute<N, P>(t, v, tw);
    if constexpr (!PI::LAST) {
#pragma unroll
        for (int i = 0; i < PI::NB; ++i)
#pragma unroll
            for (int q = 0; q < PI::R; ++q)
                frame[LdsFrame<N>::at(PI::elem(t, i, q))] = v[i * PI::R + q];
    }
}

// the outputs of the last pass into the frame in natural bin order: bin k at LdsFrame<N>::at(k)
template <int N>
PSDK_HD void store_natural(int t, const cf *v, cf *frame)
{
#pragma unroll
    for (int s = 0; s < FftPlan<N>::E; ++s)
        frame[LdsFrame<N>::at(freq_of_slot<N>(t, s))] = v[s];
}

// two-for-one separation of bin k from Z[k] and Z[(N - k) mod N]
PSDK_HD void separate(cf zk, cf znk, cf &a, cf &b)
{
    a = {0.5f * (zk.re + znk.re), 0.5f * (zk.im - znk.im)};
    b = {0.5f * (zk.im + znk.im), 0.5f * (znk.re - zk.re)};
}

// Bins a team thread accumulates: k = t + TEAM r, r < XBINS (bin N/2 is r = E/2 of thread 0)
template <int N>
struct CrossBins {
    static constexpr int TEAM = FftPlan<N>::TEAM;
    static constexpr int H = N / 2 + 1;
    static constexpr int XBINS = (H + TEAM - 1) / TEAM;
};

// Add bin k of the two segments held in the natural-order frames fx (channel x) and fy (channel y):
//   acc[0] += |Xa|^2 + |Xb|^2,  acc[1] += |Ya|^2 + |Yb|^2,  acc[2] + i acc[3] += conj(Xa) Ya + conj(Xb) Yb.
// b_live = false: segment b does not exist (the odd last segment of a tile); its separated bins are dropped.
template <int N>
PSDK_HD void cross_bin(int k, const cf *fx, const cf *fy, bool b_live, float *acc)
{
    const int kn = (N - k) & (N - 1);
    cf xa, xb, ya, yb;
    separate(lds_ld(fx + LdsFrame<N>::at(k)), lds_ld(fx + LdsFrame<N>::at(kn)), xa, xb);
    separate(lds_ld(fy + LdsFrame<N>::at(k)), lds_ld(fy + LdsFrame<N>::at(kn)), ya, yb);
    if (!b_live) {
        xb = {0.0f, 0.0f};
        yb = {0.0f, 0.0f};
    }
    acc[0] += xa.re * xa.re + xa.im * xa.im + (xb.re * xb.re + xb.im * xb.im);
    acc[1] += ya.re * ya.re + ya.im * ya.im + (yb.re * yb.re + yb.im * yb.im);
    acc[2] += xa.re * ya.re + xa.im * ya.im + (xb.re * yb.re + xb.im * yb.im);
    acc[3] += xa.re * ya.im - xa.im * ya.re + (xb.re * yb.im - xb.im * yb.re);
}

} // namespace psdk
