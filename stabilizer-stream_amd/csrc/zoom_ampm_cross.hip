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
#include "cross_channel.h"
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

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CsmJob &j) { return j.block_begin; });
    const CsmJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *fa = frames + team * 2 * Cfg::FRAME;
    cf *fb = fa + Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][ZXAMPM_ROWS];
#pragma unroll
    for (int r = 0; r < XB; ++r)
#pragma unroll
        for (int c = 0; c < ZXAMPM_ROWS; ++c)
            acc[r][c] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const int seg = lt * TEAMS + team;
        const bool act = seg < job.nseg;
        // a team without a segment reads the job's first one (always inside the streams) and drops it: its bins are zeros
        const long long ofs = (job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base;
        const float amp = job.ewma ? cross_amp(job, job.step0 + seg) : 1.0f;
        {
            cf z[E];
            cross_channel<N, true, true>(job.src[0], ofs, ofs, act, act, detrend, amp, amp, t, team, fa, red, win, tw, job.src[1],
                                         nullptr, z);
            // the team is past the last pass's reads of frame A (xfft_run ends on a team sync)
            store_natural<N>(t, z, fa);
        }
        {
            cf z[E];
            // (pass 0 of this transform waits for the readers of frame B below, as the next segment's waits for those of frame A)
            cross_channel<N, true, true>(job.src[2], ofs, ofs, act, act, detrend, amp, amp, t, team, fb, red, win, tw, job.src[3],
                                         nullptr, z);
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
    float *fq = reinterpret_cast<float *>(frames);
    float *out = job.partial + (size_t)wb * ZXAMPM_ROWS * H;
#pragma unroll
    for (int p = 0; p < ZXAMPM_ROWS / ZXAMPM_TURN; ++p) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H)
#pragma unroll
                for (int c = 0; c < ZXAMPM_TURN; ++c)
                    fq[(team * ZXAMPM_TURN + c) * H + k] = acc[r][ZXAMPM_TURN * p + c];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < ZXAMPM_TURN * H; e += Cfg::BLOCK) {
            float s = 0.0f;
#pragma unroll
            for (int g = 0; g < TEAMS; ++g)
                s += fq[g * ZXAMPM_TURN * H + e];
            out[ZXAMPM_TURN * p * H + e] = s;
        }
    }
}

hipError_t launch_zoom_ampm_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                        \
    case NN:                                                                                                                 \
        hipLaunchKernelGGL(zoom_ampm_cross_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);    \
        break;
        PSDK_CASE(64)
        PSDK_CASE(128)
        PSDK_CASE(256)
        PSDK_CASE(512)
        PSDK_CASE(1024)
        PSDK_CASE(2048)
        PSDK_CASE(4096)
#undef PSDK_CASE
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace psdk
