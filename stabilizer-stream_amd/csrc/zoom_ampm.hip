// zoom_ampm.hip -- gfx950 kernel of the AM/PM cascades (psdc_zampm_*, psdc_iqampm_*, cross_runtime.cpp): the two sideband powers of
// a carrier and their complementary spectrum, from which amplitude and phase noise separate.
//
//   zoom_ampm_kernel<N>   per segment of a (channel, stage): I and Q of the SAME segment are detrended, windowed with the EWMA
//                         amplitude (cross_channel.h) and transformed as z = I + i Q by one team, exactly as zoom_kernel does; the
//                         team's threads get their sixteen bins back, put them into the team's frame in natural order and, once
//                         the team has synchronised, add the four products of zoom_ampm_fft.h for each bin k = t + TEAM r <= N/2
//                         they own, reading Z_k and Z_(N - k) mod N from the frame: 36 accumulators a thread.
// A team without a segment transforms zeros, adds zeros and takes part in every synchronisation.  At the end the teams' values go
// through the frames' LDS, two of the four rows at a time (a team's frame holds 2 N floats, two rows take N + 2), and are combined
// in a fixed order into one workgroup partial of 4 x (N/2 + 1): the same calls give the same bits.  No atomics.
// The LDS is zoom_kernel<N>'s.  Mixers are zoom_mix_kernel (zoom.hip) and iq_mix_kernel (iq.hip), fold and stream tails
// cross_post_kernel with nrows = 4 (cross.hip), the /8 decimator hbf_dec8_kernel (kernels.hip), one job for I and one for Q.
#include "zoom_ampm.h"
#include "segment_kernel.h"
#include "zoom_ampm_fft.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void zoom_ampm_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                       const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using Bins = CrossBins<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, H = Cfg::H, E = Cfg::E, XB = Bins::XBINS;
    static_assert(2 * H <= 2 * Cfg::FRAME, "two rows of a team's bins at a time reuse its frame");

    __shared__ cf frames[TEAMS * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CrossJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][ZAMPM_ROWS];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team (an idle team's bins are zeros)
        const OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
        const float amp = job.ewma ? cross_amp(job, job.step0 + sg.seg) : 1.0f;
        cf z[E];
        cross_channel<N, true, true>(job.src[0], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, frame, red, win, tw,
                                     job.src[1], nullptr, z);
        // the team is past the last pass's reads of the frame (xfft_run ends on a team sync); the next segment's pass 0 waits
        // for the readers below
        store_natural<N>(t, z, frame);
        xteam_sync<TEAM>();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H)
                ampm_bin<N>(k, frame, acc[r]);
        }
    }

    // the teams' values through the frames' LDS, rows 2 p and 2 p + 1 in turn p, then combined in a fixed order
    combine_owned<N, ZAMPM_ROWS, 2>(frames, team, t, acc, job.partial + (size_t)wb * ZAMPM_ROWS * H);
}

hipError_t launch_zoom_ampm(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return zoom_ampm_kernel<decltype(N)::value>; });
}

} // namespace psdk
