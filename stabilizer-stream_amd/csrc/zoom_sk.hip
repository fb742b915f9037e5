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
#include "cross_channel.h"
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

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CrossJob &j) { return j.block_begin; });
    const CrossJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float a1[E], a2[E];
#pragma unroll
    for (int s = 0; s < E; ++s) {
        a1[s] = 0.0f;
        a2[s] = 0.0f;
    }

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const int seg = lt * TEAMS + team;
        const bool act = seg < job.nseg;
        // a team without a segment reads the job's first one (always inside the stream) and drops it: its bins are zeros
        const long long ofs = (job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base;
        const float w = job.ewma ? sk_weight(job, job.step0 + seg) : 1.0f;
        cf z[E];
        cross_channel<N, true, true>(job.src[0], ofs, ofs, act, act, detrend, 1.0f, 1.0f, t, team, frame, red, win, tw, job.src[1],
                                     nullptr, z);
#pragma unroll
        for (int s = 0; s < E; ++s)
            zoom_sk_slot(z[s], w, a1[s], a2[s]);
    }

    // the teams' moments through the frames' LDS in bin order, then combined in a fixed order into the four partial rows
    float *fq = reinterpret_cast<float *>(frames);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < E; ++s) {
        const int k = freq_of_slot<N>(t, s);
        fq[(team * ZSK_Q + 0) * N + k] = a1[s];
        fq[(team * ZSK_Q + 1) * N + k] = a2[s];
    }
    __syncthreads();
    float *out = job.partial + (size_t)wb * ZSK_ROWS * H;
    for (int e = threadIdx.x; e < ZSK_ROWS * H; e += Cfg::BLOCK) {
        const int row = e / H;
        const int k = zoom_sk_row_bin<N>(row, e - row * H);
        const int q = zoom_sk_row_moment(row);
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < TEAMS; ++g)
            s += fq[(g * ZSK_Q + q) * N + k];
        out[e] = s;
    }
}

hipError_t launch_zoom_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                   \
    case NN:                                                                                                            \
        hipLaunchKernelGGL(zoom_sk_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);       \
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
