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
#include "segment_kernel.h"
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

    int wb;
    const CrossJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *frame = frames + team * Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[1][E];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment a team
        const OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
        const float amp = job.ewma ? cross_amp(job, job.step0 + sg.seg) : 1.0f;
        cross_channel<N, true>(job.src[0], sg.ofs, sg.ofs, sg.act, sg.act, detrend, amp, amp, t, team, frame, red, win, tw, job.src[1],
                               acc[0]);
    }

    // the teams' rows through the frames' LDS in bin order, then combined in a fixed order into the two partial rows
    combine_slots<N, 1, 1>(frames, team, t, acc, job.partial + (size_t)wb * 2 * H);
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

int zoom_segments_per_tile(int n) { return seg_supported(n) ? seg_teams(n) : 0; }

int zoom_block_threads(int n) { return cross_block_threads(n); }

hipError_t launch_zoom(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return zoom_kernel<decltype(N)::value>; });
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
