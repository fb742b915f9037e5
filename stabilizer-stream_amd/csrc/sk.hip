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
#include "cross_channel.h"
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

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CrossJob &j) { return j.block_begin; });
    const CrossJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][SK_ROWS];
#pragma unroll
    for (int r = 0; r < XB; ++r)
#pragma unroll
        for (int c = 0; c < SK_ROWS; ++c)
            acc[r][c] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment pair a team
        const int seg_lo = lt * SPT;
        const int seg_hi = min(job.nseg, seg_lo + SPT);
        const int la = seg_lo + 2 * team;
        const bool act_a = la < seg_hi, act_b = la + 1 < seg_hi;
        // lanes without a segment read the job's first one (always inside the stream) and drop it
        const long long ofs_safe = job.seg0 * (long long)hop - job.src_base;
        const long long ofs_a = (job.seg0 + la) * (long long)hop - job.src_base;
        const long long ofs_la = act_a ? ofs_a : ofs_safe, ofs_lb = act_b ? ofs_a + hop : ofs_safe;
        float wa = 1.0f, wbw = 1.0f;
        if (job.ewma) {
            wa = sk_weight(job, job.step0 + la);
            wbw = sk_weight(job, job.step0 + la + 1);
        }
        cross_channel<N>(job.src[0], ofs_la, ofs_lb, act_a, act_b, detrend, 1.0f, 1.0f, t, team, frame, red, win, tw);
        xteam_sync<TEAM>();
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k < H)
                sk_bin<N>(k, frame, wa, wbw, act_b, acc[r]);
        }
    }

    // combine the teams (fixed order) and write the workgroup's partial rows
    float *fq = reinterpret_cast<float *>(frames);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < XB; ++r) {
        const int k = t + TEAM * r;
        if (k < H)
#pragma unroll
            for (int c = 0; c < SK_ROWS; ++c)
                fq[team * SK_ROWS * H + sk_row_at<N>(c, k)] = acc[r][c];
    }
    __syncthreads();
    float *out = job.partial + (size_t)wb * SK_ROWS * H;
    for (int e = threadIdx.x; e < SK_ROWS * H; e += Cfg::BLOCK) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < TEAMS; ++g)
            s += fq[g * SK_ROWS * H + e];
        out[e] = s;
    }
}

int sk_segments_per_tile(int n) { return cross_segments_per_tile(n); }

hipError_t launch_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                   \
    case NN:                                                                                                            \
        hipLaunchKernelGGL(sk_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);            \
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
