// zoom_ampm_cross.hip -- gfx950 kernel of the AM/PM cross cascades (psdc_zxampm_*, psdc_iqxampm_*, cross_runtime.cpp): the zoom
// cross object's eight rows of a pair and the two complementary cross spectra Z_a[k] Z_b[N - k] and Z_a[N - k] Z_b[k], from which
// the cross spectra of the two channels' amplitude and phase modulation separate.
//
//   zoom_ampm_cross_kernel<N>   per segment of a (pair, stage): a team transforms channel a's segment z_a = I_a + i Q_a
//                               (cross_channel.h, detrended and windowed with the EWMA amplitude as zoom_cross_kernel does) and
//                               puts its bins into the team's frame A in natural order, transforms channel b's SAME segment and
//                               puts it into frame B and, once the team has synchronised, adds the twelve values of
//                               zoom_ampm_cross_fft.h for each bin k = t + TEAM r <= N/2 the thread owns, reading Z_a[k], Z_a[kn],
//                               Z_b[k], Z_b[kn] from the frames: 12 XBINS = 108 accumulators a thread.  No transform bins stay
//                               live across the accumulation.
// The tile is zoom_cross_kernel's (one segment a team), the LDS cross_kernel's (two frames a team).  A team without a segment
// transforms zeros, adds zeros and takes part in every synchronisation.  At the end the teams' values go through the frames' LDS,
// ZXAMPM_TURN rows at a time, and are combined in a fixed order into one workgroup partial of 12 x (N/2 + 1): the same calls give
// the same bits.  No atomics.
// The launcher is reached through launch_zoom_cross (zoom_cross.hip) on CsmBatch::variant; mixers, the fold and stream tails
// (cross_post_kernel with nrows = 12) and the /8 decimator are the zoom cross / IQ cross objects'.
#include "zoom_ampm_cross.h"
#include "segment_kernel.h"
#include "zoom_ampm_cross_fft.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void zoom_ampm_cross_kernel(const CsmBatch batch, const float *__restrict__ win,
                                                                             const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using Bins = CrossBins<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, H = Cfg::H, E = Cfg::E, XB = Bins::XBINS;
    static_assert(ZXAMPM_ROWS % ZXAMPM_TURN == 0 && ZXAMPM_TURN * H <= 4 * Cfg::FRAME,
                  "a turn's rows of a team's bins reuse its two frames");

    __shared__ cf frames[TEAMS * 2 * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CsmJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *fa = frames + team * 2 * Cfg::FRAME;
    cf *fb = fa + Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][ZXAMPM_ROWS];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team (an idle team's bins are zeros)
        const OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
        const float amp = job.ewma ? cross_amp(job, job.step0 + sg.seg) : 1.0f;
        {
            cf z[E];
            cross_channel<N, true, true>(job.src[0], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, fa, red, win, tw,
                                         job.src[1], nullptr, z);
            // the team is past the last pass's reads of frame A (xfft_run ends on a team sync)
            store_natural<N>(t, z, fa);
        }
        {
            cf z[E];
            // (pass 0 of this transform waits for the readers of frame B below, as the next segment's waits for those of frame A)
            cross_channel<N, true, true>(job.src[2], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, fb, red, win, tw,
                                         job.src[3], nullptr, z);
            store_natural<N>(t, z, fb);
        }
        xteam_sync<TEAM>();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H)
                ampm_cross_bin<N>(k, fa, fb, acc[r]);
        }
    }

    // the teams' values through the frames' LDS, rows ZXAMPM_TURN p ... ZXAMPM_TURN p + 3 in turn p, then combined in a fixed order
    combine_owned<N, ZXAMPM_ROWS, ZXAMPM_TURN>(frames, team, t, acc, job.partial + (size_t)wb * ZXAMPM_ROWS * H);
}

hipError_t launch_zoom_ampm_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return zoom_ampm_cross_kernel<decltype(N)::value>; });
}

} // namespace psdk
