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
#include "cross_channel.h"
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

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CsmJob &j) { return j.block_begin; });
    const CsmJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[ZCROSS_Q * E];
#pragma unroll
    for (int s = 0; s < ZCROSS_Q * E; ++s)
        acc[s] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const int seg = lt * TEAMS + team;
        const bool act = seg < job.nseg;
        // a team without a segment reads the job's first one (always inside the streams) and drops it
        const long long ofs = (job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base;
        const float amp = job.ewma ? cross_amp(job, job.step0 + seg) : 1.0f;
        cf za[E], zb[E];
        cross_channel<N, true, true>(job.src[0], ofs, ofs, act, act, detrend, amp, amp, t, team, frame, red, win, tw, job.src[1],
                                     nullptr, za);
        cross_channel<N, true, true>(job.src[2], ofs, ofs, act, act, detrend, amp, amp, t, team, frame, red, win, tw, job.src[3],
                                     nullptr, zb);
#pragma unroll
        for (int s = 0; s < E; ++s)
            zoom_cross_bin(za[s], zb[s], acc + s, E);
    }

    // the teams' values through the frames' LDS in bin order, values 2 p and 2 p + 1 in turn p, then combined in a fixed order
    // into the rows 4 p ... 4 p + 3 of the partial
    float *fq = reinterpret_cast<float *>(frames);
    float *out = job.partial + (size_t)wb * ZCROSS_ROWS * H;
#pragma unroll
    for (int p = 0; p < ZCROSS_Q / 2; ++p) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < E; ++s)
                fq[(team * 2 + j) * N + freq_of_slot<N>(t, s)] = acc[(2 * p + j) * E + s];
        __syncthreads();
        for (int e = threadIdx.x; e < 4 * H; e += Cfg::BLOCK) {
            const int row = 4 * p + e / H;
            const int k = zoom_cross_row_bin<N>(row, e % H);
            const int j = zoom_cross_row_value(row) - 2 * p;
            float s = 0.0f;
#pragma unroll
            for (int g = 0; g < TEAMS; ++g)
                s += fq[(g * 2 + j) * N + k];
            out[row * H + e % H] = s;
        }
    }
}

// every n the object runs
#define PSDK_ZCROSS_CASES(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

bool zoom_cross_supported(int n)
{
#define X(NN)      \
    if (n == NN) \
        return true;
    PSDK_ZCROSS_CASES(X)
#undef X
    return false;
}

int zoom_cross_segments_per_tile(int n)
{
#define X(NN)      \
    if (n == NN) \
        return CrossCfg<NN>::TEAMS;
    PSDK_ZCROSS_CASES(X)
#undef X
    return 0;
}

int zoom_cross_block_threads(int n)
{
#define X(NN)      \
    if (n == NN) \
        return CrossCfg<NN>::BLOCK;
    PSDK_ZCROSS_CASES(X)
#undef X
    return 0;
}

hipError_t launch_zoom_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    // a batch of the AM/PM cross kinds (cross_runtime.cpp marks it): the same jobs on the twelve-row kernel
    if (b.variant == ZCROSS_VARIANT_AMPM)
        return launch_zoom_ampm_cross(n, b, win, tw, s);
    if (b.variant != ZCROSS_VARIANT_CSD)
        return hipErrorInvalidValue;
#define X(NN)                                                                                                      \
    if (n == NN) {                                                                                                 \
        hipLaunchKernelGGL(zoom_cross_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw); \
        return hipGetLastError();                                                                                  \
    }
    PSDK_ZCROSS_CASES(X)
#undef X
    return hipErrorInvalidValue;
}

} // namespace psdk
