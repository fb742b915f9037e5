// zoom_cross.hip -- gfx950 kernel of the zoom cross cascade (psdc_zcsd_*, cross_runtime.cpp): two streams around a carrier.
//
//   zoom_cross_kernel<N>   per segment of a (pair, stage): a team transforms channel a's segment z_a = I_a + i Q_a
//                          (cross_channel.h, detrended and windowed as zoom_kernel's) and keeps its sixteen bins of Z_a in
//                          registers, transforms channel b's SAME segment in the same LDS frame, and adds the four values of
//                          zoom_cross_fft.h per bin straight from the two register sets: |Z_a|^2, |Z_b|^2, Re and Im of
//                          conj(Z_a) Z_b -- 64 accumulators a thread.  No separation, no natural-order store, nothing subtracted
//                          across bins.
// At the end the teams' values go through the frames' LDS in bin order, two of the four values at a time (a team's frame holds
// 2 N floats), and are combined in a fixed order into one workgroup partial of 8 x (N/2 + 1): the same calls give the same bits.
// The mixer is zoom_mix_kernel (zoom.hip), the fold and stream tails cross_post_kernel with nrows = 8 (cross.hip), the /8
// decimator hbf_dec8_kernel (kernels.hip), four jobs a (pair, stage).
#include "zoom_cross.h"
#include "segment_kernel.h"
#include "zoom_ampm_cross.h"
#include "zoom_ampm_cross_fft.h"
#include "zoom_cross_fft.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void zoom_cross_kernel(const CsmBatch batch, const float *__restrict__ win,
                                                                        const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, H = Cfg::H, E = Cfg::E;
    static_assert(N <= Cfg::FRAME, "two values of a team's bins at a time reuse its frame");

    __shared__ cf frames[TEAMS * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CsmJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[ZCROSS_Q][E];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
        const float amp = job.ewma ? cross_amp(job, job.step0 + sg.seg) : 1.0f;
        cf za[E], zb[E];
        cross_channel<N, true, true>(job.src[0], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, frame, red, win, tw,
                                     job.src[1], nullptr, za);
        cross_channel<N, true, true>(job.src[2], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, frame, red, win, tw,
                                     job.src[3], nullptr, zb);
#pragma unroll
        for (int s = 0; s < E; ++s)
            zoom_cross_bin(za[s], zb[s], &acc[0][s], E);
    }

    // the teams' values through the frames' LDS in bin order, values 2 p and 2 p + 1 in turn p, then combined in a fixed order
    // into the rows 4 p ... 4 p + 3 of the partial
    combine_slots<N, ZCROSS_Q, 2>(frames, team, t, acc, job.partial + (size_t)wb * ZCROSS_ROWS * H);
}

bool zoom_cross_supported(int n) { return seg_supported(n); } // every n the object runs

int zoom_cross_segments_per_tile(int n) { return seg_supported(n) ? seg_teams(n) : 0; }

int zoom_cross_block_threads(int n) { return seg_supported(n) ? seg_block(n) : 0; }

hipError_t launch_zoom_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    // a batch of the AM/PM cross kinds (cross_runtime.cpp marks it): the same jobs on the twelve-row kernel
    if (b.variant == ZCROSS_VARIANT_AMPM)
        return launch_zoom_ampm_cross(n, b, win, tw, s);
    if (b.variant != ZCROSS_VARIANT_CSD)
        return hipErrorInvalidValue;
    return seg_launch(n, b, win, tw, s, [](auto N) { return zoom_cross_kernel<decltype(N)::value>; });
}

} // namespace psdk
