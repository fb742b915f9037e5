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
#include "cross_channel.h"
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

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CrossJob &j) { return j.block_begin; });
    const CrossJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][ZAMPM_ROWS];
#pragma unroll
    for (int r = 0; r < XB; ++r)
#pragma unroll
        for (int c = 0; c < ZAMPM_ROWS; ++c)
            acc[r][c] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const int seg = lt * TEAMS + team;
        const bool act = seg < job.nseg;
        // a team without a segment reads the job's first one (always inside the stream) and drops it: its bins are zeros
        const long long ofs = (job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base;
        const float amp = job.ewma ? cross_amp(job, job.step0 + seg) : 1.0f;
        cf z[E];
        cross_channel<N, true, true>(job.src[0], ofs, ofs, act, act, detrend, amp, amp, t, team, frame, red, win, tw, job.src[1],
                                     nullptr, z);
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
    float *fq = reinterpret_cast<float *>(frames);
    float *out = job.partial + (size_t)wb * ZAMPM_ROWS * H;
#pragma unroll
    for (int p = 0; p < ZAMPM_ROWS / 2; ++p) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H) {
                fq[(team * 2 + 0) * H + k] = acc[r][2 * p];
                fq[(team * 2 + 1) * H + k] = acc[r][2 * p + 1];
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 2 * H; e += Cfg::BLOCK) {
            float s = 0.0f;
#pragma unroll
            for (int g = 0; g < TEAMS; ++g)
                s += fq[g * 2 * H + e];
            out[2 * p * H + e] = s;
        }
    }
}

hipError_t launch_zoom_ampm(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                   \
    case NN:                                                                                                            \
        hipLaunchKernelGGL(zoom_ampm_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);     \
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
