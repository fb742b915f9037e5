// sk.hip -- gfx950 kernel of the spectral kurtosis cascade (psdc_sk_*, cross_runtime.cpp): per-bin Gaussianity beside the PSD.
//
//   sk_kernel<N>   per segment of a (channel, stage): two consecutive segments of the ONE stream are detrended, windowed
//                  (cross_channel.h, amplitude 1) and transformed as z = a + i b by one team, separated as the pair kernel
//                  separates a channel (cross_fft.h), and every thread adds w P and w P^2 of both segments to the registers
//                  of its bins (sk_fft.h says why the weight is applied to the products and not to the samples).  A workgroup
//                  writes one partial of two rows, S1 and S2, k = 0 ... N/2; the teams are combined in a fixed order.
// Fold and stream tails are cross_post_kernel with nrows = 2 (cross.hip), the /8 decimator is hbf_dec8_kernel (kernels.hip),
// one job a channel.  One frame a team: half the LDS of cross_kernel<N>.
#include "sk.h"
#include "segment_kernel.h"
#include "sk_fft.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void sk_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using Bins = CrossBins<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, SPT = Cfg::SPT, H = Cfg::H, XB = Bins::XBINS;
    static_assert(SK_ROWS * H <= 2 * Cfg::FRAME, "the teams' rows reuse the frames' LDS");

    __shared__ cf frames[TEAMS * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CrossJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][SK_ROWS];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment pair a team
        const int seg_lo = lt * SPT;
        const SegPair sp = seg_pair(job, hop, min(job.nseg, seg_lo + SPT), seg_lo + 2 * team);
        float wa = 1.0f, wbw = 1.0f;
        if (job.ewma) {
            wa = sk_weight(job, job.step0 + sp.seg);
            wbw = sk_weight(job, job.step0 + sp.seg + 1);
        }
        cross_channel<N>(job.src[0], sp.ofs_a, sp.ofs_b, sp.act_a, sp.act_b, detrend, 1.0f, 1.0f, t, team, frame, red, win, tw);
        xteam_sync<TEAM>();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H)
                sk_bin<N>(k, frame, wa, wbw, sp.act_b, acc[r]);
        }
    }

    // combine the teams (fixed order) and write the workgroup's partial rows: element sk_row_at<N>(row, k)
    combine_owned<N, SK_ROWS, SK_ROWS>(frames, team, t, acc, job.partial + (size_t)wb * SK_ROWS * H);
}

int sk_segments_per_tile(int n) { return cross_segments_per_tile(n); }

hipError_t launch_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return sk_kernel<decltype(N)::value>; });
}

} // namespace psdk
