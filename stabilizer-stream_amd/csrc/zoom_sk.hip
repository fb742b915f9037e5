// zoom_sk.hip -- gfx950 kernel of the zoom and IQ spectral kurtosis cascades (psdc_zsk_*, psdc_iqsk_*, cross_runtime.cpp): SK
// around a carrier.
//
//   zoom_sk_kernel<N>   per segment of a (channel, stage): I and Q of the SAME segment are detrended, windowed (cross_channel.h,
//                       amplitude 1) and transformed as z = I + i Q by one team, exactly as zoom_kernel does; the team's threads
//                       get their sixteen bins back and add w P and (w P) P of each to two register sets (zoom_sk_fft.h), 32
//                       accumulators a thread.  No separation, no natural-order store.
// At the end the teams' values go through the frames' LDS in bin order, both moments at once (a team's frame holds 2 N floats),
// and are combined in a fixed order into one workgroup partial of 4 x (N/2 + 1): the same calls give the same bits.  No atomics.
// The LDS is zoom_kernel<N>'s.  Mixers are zoom_mix_kernel (zoom.hip) and iq_mix_kernel (iq.hip), fold and stream tails
// cross_post_kernel with nrows = 4 (cross.hip), the /8 decimator hbf_dec8_kernel (kernels.hip), one job for I and one for Q.
#include "zoom_sk.h"
#include "segment_kernel.h"
#include "zoom_sk_fft.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void zoom_sk_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                     const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, H = Cfg::H, E = Cfg::E;
    static_assert(ZSK_Q * N <= 2 * Cfg::FRAME, "both moments of a team's bins reuse its frame at once");

    __shared__ cf frames[TEAMS * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CrossJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[ZSK_Q][E]; // S1, S2 of the thread's sixteen bins
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team (an idle team's bins are zeros)
        const OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
        const float w = job.ewma ? sk_weight(job, job.step0 + sg.seg) : 1.0f;
        cf z[E];
        cross_channel<N, true, true>(job.src[0], sg.ofs, sg.ofs, sg.act, sg.act, detrend, 1.0f, 1.0f, t, team, frame, red, win, tw,
                                     job.src[1], nullptr, z);
#pragma unroll
        for (int s = 0; s < E; ++s)
            zoom_sk_slot(z[s], w, acc[0][s], acc[1][s]);
    }

    // the teams' moments through the frames' LDS in bin order, then combined in a fixed order into the four partial rows
    combine_slots<N, ZSK_Q, ZSK_Q>(frames, team, t, acc, job.partial + (size_t)wb * ZSK_ROWS * H);
}

hipError_t launch_zoom_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return zoom_sk_kernel<decltype(N)::value>; });
}

} // namespace psdk
