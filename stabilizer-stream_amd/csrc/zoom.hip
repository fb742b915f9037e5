// zoom.hip -- gfx950 kernels of the zoom cascade (psdc_zoom_*, cross_runtime.cpp): a log-resolution spectrum around a carrier.
//
//   zoom_mix_kernel   the mixer in front of stage 0, in place of the input copy: reads a call's real samples once and stores
//                     I = x cos, Q = -x sin (zoom_lo.h) straight into the channel's two stage-0 streams.  A sample's phase is
//                     phase0 + ftw j in 64-bit integers from its stream index j: nothing is accumulated in floating point, so
//                     any cut of the stream into calls gives the same I and Q.
//   zoom_kernel<N>    per segment of a (channel, stage): I and Q of the SAME segment are detrended, windowed (cross_channel.h)
//                     and transformed as z = I + i Q by one team; every thread adds |Z_k|^2 of its sixteen bins straight from
//                     its registers (no separation, no natural-order store).  A workgroup writes one partial of two rows:
//                     upper[k] = |Z_k|^2 and lower[k] = |Z_(N - k) mod N|^2, k = 0 ... N/2.
// Fold and stream tails are cross_post_kernel with nrows = 2 (cross.hip), the /8 decimator is hbf_dec8_kernel (kernels.hip),
// one job for I and one for Q.
#include "zoom.h"
#include "cross_channel.h"
#include "zoom_lo.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void zoom_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                  const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, H = Cfg::H, E = Cfg::E;
    static_assert(N <= 2 * Cfg::FRAME, "the teams' rows reuse the frames' LDS");

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

    float acc[E];
#pragma unroll
    for (int s = 0; s < E; ++s)
        acc[s] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const int seg = lt * TEAMS + team;
        const bool act = seg < job.nseg;
        // a team without a segment reads the job's first one (always inside the stream) and drops it
        const long long ofs = (job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base;
        const float amp = job.ewma ? cross_amp(job, job.step0 + seg) : 1.0f;
        cross_channel<N, true>(job.src[0], ofs, ofs, act, act, detrend, amp, amp, t, team, frame, red, win, tw, job.src[1], acc);
    }

    // the teams' rows through the frames' LDS in bin order, then combined in a fixed order into the two partial rows
    float *fq = reinterpret_cast<float *>(frames);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < E; ++s)
        fq[team * N + freq_of_slot<N>(t, s)] = acc[s];
    __syncthreads();
    float *out = job.partial + (size_t)wb * 2 * H;
    for (int e = threadIdx.x; e < 2 * H; e += Cfg::BLOCK) {
        const int k = e < H ? e : (N - (e - H)) & (N - 1);
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < TEAMS; ++g)
            s += fq[g * N + k];
        out[e] = s;
    }
}

// A thread takes MIX_Q consecutive samples that start on a 16-byte boundary of the destination streams: one 16-byte store to
// each, and one 16-byte load where the source is aligned as well (else four 4-byte loads).  Thread 0 takes the up to three
// samples in front of the first boundary; the thread of the last quad takes the partial one.
constexpr int MIX_Q = 4, MIX_BLOCK = 256;

__global__ __launch_bounds__(MIX_BLOCK) void zoom_mix_kernel(const ZoomMixJob job, const unsigned head, const int src_aligned)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * MIX_BLOCK + threadIdx.x;
    if (g == 0) {
        for (unsigned i = 0; i < head; ++i)
            zoom_mix(job.x[i], job.phase0 + job.ftw * (job.j0 + i), job.dst_i[i], job.dst_q[i]);
        return;
    }
    const unsigned long long i0 = head + (g - 1) * MIX_Q;
    if (i0 >= job.len)
        return;
    unsigned long long ph = job.phase0 + job.ftw * (job.j0 + i0);
    if (job.len - i0 >= MIX_Q) {
        float4 x;
        if (src_aligned)
            x = *reinterpret_cast<const float4 *>(job.x + i0);
        else
            x = make_float4(job.x[i0], job.x[i0 + 1], job.x[i0 + 2], job.x[i0 + 3]);
        float4 vi, vq;
        zoom_mix(x.x, ph, vi.x, vq.x);
        zoom_mix(x.y, ph += job.ftw, vi.y, vq.y);
        zoom_mix(x.z, ph += job.ftw, vi.z, vq.z);
        zoom_mix(x.w, ph += job.ftw, vi.w, vq.w);
        *reinterpret_cast<float4 *>(job.dst_i + i0) = vi;
        *reinterpret_cast<float4 *>(job.dst_q + i0) = vq;
        return;
    }
    for (unsigned long long i = i0; i < job.len; ++i, ph += job.ftw)
        zoom_mix(job.x[i], ph, job.dst_i[i], job.dst_q[i]);
}

int zoom_segments_per_tile(int n) { return cross_supported(n) ? cross_block_threads(n) / (n / 16) : 0; }

int zoom_block_threads(int n) { return cross_block_threads(n); }

hipError_t launch_zoom(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                   \
    case NN:                                                                                                            \
        hipLaunchKernelGGL(zoom_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);          \
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

hipError_t launch_zoom_mix(const ZoomMixJob &j, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    if (((uintptr_t)j.dst_i & 3) || ((uintptr_t)j.x & 3) || (((uintptr_t)j.dst_i ^ (uintptr_t)j.dst_q) & 15))
        return hipErrorInvalidValue;
    const unsigned long long lead = (4 - (((uintptr_t)j.dst_i >> 2) & 3)) & 3;
    const unsigned head = (unsigned)(lead < j.len ? lead : j.len);
    const unsigned long long quads = (j.len - head + MIX_Q - 1) / MIX_Q;
    const unsigned long long blocks = (quads + 1 + MIX_BLOCK - 1) / MIX_BLOCK;
    if (blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const int src_aligned = ((uintptr_t)(j.x + head) & 15) == 0;
    hipLaunchKernelGGL(zoom_mix_kernel, dim3((unsigned)blocks), dim3(MIX_BLOCK), 0, s, j, head, src_aligned);
    return hipGetLastError();
}

} // namespace psdk
