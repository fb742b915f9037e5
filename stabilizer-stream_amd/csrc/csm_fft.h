// csm_fft.h -- the per-bin arithmetic of the cross-spectral matrix kernel (csm.hip): every product of one bin of M channels.
//
// Each channel's natural-order frame holds the spectrum of z = a + i b, two consecutive segments of that channel (cross_fft.h:
// one transform per channel, channels never packed together).  A bin is separated ONCE per channel and the M (M + 1) / 2
// products conj(X_a) X_b, a <= b, are formed from the separated values.  Row layout of the M x M real rows (the layout of
// include/psdcascade.h): row a M + a is S_aa; for a < b row a M + b is Re S_ab and row b M + a is Im S_ab.
//
// Everything here is __host__ __device__: tests/host/csm_emul.cpp runs it against an f64 DFT.
#pragma once
#include "cross_fft.h"

namespace psdk {

// Add bin k of the two segments held in the frames of M channels (channel c at frames + c * stride) to acc[M * M].
// b_live = false: segment b does not exist (the odd last segment of a tile); its separated bins are dropped.
// The sums are written as cross_bin writes them, so M = 2 forms the pair kernel's four values.
template <int N, int M>
PSDK_HD void csm_bin(int k, const cf *frames, int stride, bool b_live, float *acc)
{
    const int kn = (N - k) & (N - 1);
    const int pk = LdsFrame<N>::at(k), pn = LdsFrame<N>::at(kn);
    cf xa[M], xb[M];
#pragma unroll
    for (int c = 0; c < M; ++c) {
        separate(lds_ld(frames + c * stride + pk), lds_ld(frames + c * stride + pn), xa[c], xb[c]);
        if (!b_live)
            xb[c] = {0.0f, 0.0f};
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
        acc[a * M + a] += xa[a].re * xa[a].re + xa[a].im * xa[a].im + (xb[a].re * xb[a].re + xb[a].im * xb[a].im);
#pragma unroll
        for (int b = a + 1; b < M; ++b) {
            acc[a * M + b] += xa[a].re * xa[b].re + xa[a].im * xa[b].im + (xb[a].re * xb[b].re + xb[a].im * xb[b].im);
            acc[b * M + a] += xa[a].re * xa[b].im - xa[a].im * xa[b].re + (xb[a].re * xb[b].im - xb[a].im * xb[b].re);
        }
    }
}

// Workgroup shape of csm_kernel<N, M>: BLOCK threads are BLOCK / TEAM transform teams, each with M frames of its own; for the
// products the same threads are PG groups of GS threads, thread pt of a group owning bins pt + GS r, r < XB, of the teams
// g = group, group + PG, ... (plain constants: the host planner and the emulation read them too)
template <int N, int M>
struct CsmShape {
    static constexpr int TEAM = FftPlan<N>::TEAM;
    static constexpr int FRAME = LdsFrame<N>::SIZE;
    static constexpr int H = N / 2 + 1;
    static constexpr int LDS_MAX = 160 * 1024;
    // four wavefronts (one a SIMD, as the registers of the transform allow) unless the frames of 256 threads overflow the LDS
    static constexpr int BLOCK = (256 / TEAM) * M * FRAME * 8 <= LDS_MAX ? 256 : 128;
    static constexpr int TEAMS = BLOCK / TEAM;
    static constexpr int SPT = 2 * TEAMS; // segments per tile: one segment pair a team
    static constexpr int GS = N / 2 < BLOCK ? N / 2 : BLOCK;
    static constexpr int PG = BLOCK / GS;
    static constexpr int XB = (H + GS - 1) / GS;
    static constexpr int ROWS = M * M;
    static constexpr int LDS_BYTES = TEAMS * M * FRAME * 8;
    static_assert(TEAM <= BLOCK && LDS_BYTES <= LDS_MAX, "the frames of a workgroup fit the LDS");
    static_assert(PG == 1 || PG * ROWS * H * 4 <= LDS_BYTES, "the product groups are combined in the frames' LDS");
};

} // namespace psdk
