// iq.hip -- gfx950 kernel of the IQ cascade's sample routes (psdc_iq_process*, cross_runtime.cpp).
//
//   iq_mix_kernel<INTERLEAVED>  the complex mixer in front of stage 0, where zoom_mix_kernel stands for a real stream: reads a
//                               call's complex samples once -- two planar streams, or one stream of (re, im) pairs -- and stores
//                               I' = fmaf(Q, s, I c), Q' = fmaf(Q, c, -(I s)) (iq_lo.h) straight into the channel's two stage-0
//                               streams.  A sample's phase is phase0 + ftw j in 64-bit integers from its stream index j, stepped
//                               in integers inside a thread: any cut of the stream into calls gives the same I' and Q'.
// The access scheme is zoom_mix_kernel's: a thread takes IQ_Q consecutive samples that start on a 16-byte boundary of the
// destination streams, one 16-byte store to each.  Where the source is 16-byte aligned as well it is read with 16-byte loads
// (planar: one from I and one from Q, each judged on its own; interleaved: two); otherwise with 4-byte loads (planar) or 8-byte
// loads (interleaved: a pair is 8-byte aligned).  Thread 0 takes the up to three samples in front of the first boundary; the
// thread of the last quad takes the partial one.  No LDS, no scratch.
#include "iq.h"
#include "iq_lo.h"

namespace psdk {

constexpr int IQ_Q = 4, IQ_BLOCK = 256;

namespace {

// complex sample i of the call, from either layout
template <bool INTERLEAVED>
__device__ __forceinline__ void iq_load1(const IqMixJob &job, unsigned long long i, float &a, float &b)
{
    if constexpr (INTERLEAVED) {
        const float2 z = *reinterpret_cast<const float2 *>(job.src_i + 2 * i);
        a = z.x, b = z.y;
    } else {
        a = job.src_i[i], b = job.src_q[i];
    }
}

} // namespace

// src_aligned: bit 0 -- the I stream (interleaved: the pairs) is 16-byte aligned at the first quad, bit 1 -- the Q stream is
template <bool INTERLEAVED>
__global__ __launch_bounds__(IQ_BLOCK) void iq_mix_kernel(const IqMixJob job, const unsigned head, const int src_aligned)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * IQ_BLOCK + threadIdx.x;
    if (g == 0) {
        for (unsigned i = 0; i < head; ++i) {
            float a, b;
            iq_load1<INTERLEAVED>(job, i, a, b);
            iq_mix(a, b, job.phase0 + job.ftw * (job.j0 + i), job.dst_i[i], job.dst_q[i]);
        }
        return;
    }
    const unsigned long long i0 = head + (g - 1) * IQ_Q;
    if (i0 >= job.len)
        return;
    unsigned long long ph = job.phase0 + job.ftw * (job.j0 + i0);
    if (job.len - i0 >= IQ_Q) {
        float4 a, b;
        if constexpr (INTERLEAVED) {
            const float *p = job.src_i + 2 * i0;
            if (src_aligned & 1) {
                const float4 u = *reinterpret_cast<const float4 *>(p), v = *reinterpret_cast<const float4 *>(p + 4);
                a = make_float4(u.x, u.z, v.x, v.z);
                b = make_float4(u.y, u.w, v.y, v.w);
            } else {
                const float2 z0 = *reinterpret_cast<const float2 *>(p), z1 = *reinterpret_cast<const float2 *>(p + 2),
                             z2 = *reinterpret_cast<const float2 *>(p + 4), z3 = *reinterpret_cast<const float2 *>(p + 6);
                a = make_float4(z0.x, z1.x, z2.x, z3.x);
                b = make_float4(z0.y, z1.y, z2.y, z3.y);
            }
        } else {
            if (src_aligned & 1)
                a = *reinterpret_cast<const float4 *>(job.src_i + i0);
            else
                a = make_float4(job.src_i[i0], job.src_i[i0 + 1], job.src_i[i0 + 2], job.src_i[i0 + 3]);
            if (src_aligned & 2)
                b = *reinterpret_cast<const float4 *>(job.src_q + i0);
            else
                b = make_float4(job.src_q[i0], job.src_q[i0 + 1], job.src_q[i0 + 2], job.src_q[i0 + 3]);
        }
        float4 vi, vq;
        iq_mix(a.x, b.x, ph, vi.x, vq.x);
        iq_mix(a.y, b.y, ph += job.ftw, vi.y, vq.y);
        iq_mix(a.z, b.z, ph += job.ftw, vi.z, vq.z);
        iq_mix(a.w, b.w, ph += job.ftw, vi.w, vq.w);
        *reinterpret_cast<float4 *>(job.dst_i + i0) = vi;
        *reinterpret_cast<float4 *>(job.dst_q + i0) = vq;
        return;
    }
    for (unsigned long long i = i0; i < job.len; ++i, ph += job.ftw) {
        float a, b;
        iq_load1<INTERLEAVED>(job, i, a, b);
        iq_mix(a, b, ph, job.dst_i[i], job.dst_q[i]);
    }
}

hipError_t launch_iq_mix(const IqMixJob &j, bool interleaved, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    if (!j.src_i || (!interleaved && !j.src_q) || !j.dst_i || !j.dst_q)
        return hipErrorInvalidValue;
    if (((uintptr_t)j.dst_i & 3) || (((uintptr_t)j.dst_i ^ (uintptr_t)j.dst_q) & 15))
        return hipErrorInvalidValue;
    if (interleaved ? ((uintptr_t)j.src_i & 7) != 0 : (((uintptr_t)j.src_i | (uintptr_t)j.src_q) & 3) != 0)
        return hipErrorInvalidValue;
    const unsigned long long lead = (4 - (((uintptr_t)j.dst_i >> 2) & 3)) & 3;
    const unsigned head = (unsigned)(lead < j.len ? lead : j.len);
    const unsigned long long quads = (j.len - head + IQ_Q - 1) / IQ_Q;
    const unsigned long long blocks = (quads + 1 + IQ_BLOCK - 1) / IQ_BLOCK;
    if (blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    if (interleaved) {
        const int src_aligned = ((uintptr_t)(j.src_i + 2 * (size_t)head) & 15) == 0 ? 1 : 0;
        hipLaunchKernelGGL(iq_mix_kernel<true>, dim3((unsigned)blocks), dim3(IQ_BLOCK), 0, s, j, head, src_aligned);
    } else {
        const int src_aligned = (((uintptr_t)(j.src_i + head) & 15) == 0 ? 1 : 0) | (((uintptr_t)(j.src_q + head) & 15) == 0 ? 2 : 0);
        hipLaunchKernelGGL(iq_mix_kernel<false>, dim3((unsigned)blocks), dim3(IQ_BLOCK), 0, s, j, head, src_aligned);
    }
    return hipGetLastError();
}

} // namespace psdk
