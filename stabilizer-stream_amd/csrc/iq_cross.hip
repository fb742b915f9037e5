// iq_cross.hip -- gfx950 kernel of the IQ cross cascade's sample routes (psdc_iqcsd_process*, cross_runtime.cpp).
//
//   iq_pair_mix_kernel<INTERLEAVED>  iq_mix_kernel for both sides of a pair in one launch: reads a call's complex samples of side a
//                                    and side b once -- four planar streams, or two streams of (re, im) pairs -- and stores each
//                                    side's I' = fmaf(Q, s, I c), Q' = fmaf(Q, c, -(I s)) (iq_lo.h, with the side's carrier)
//                                    straight into the pair's four stage-0 streams I_a, Q_a, I_b, Q_b.  A sample's phase is
//                                    phase0 + ftw j of its side in 64-bit integers from its stream index j (one index for both
//                                    sides), stepped in integers inside a thread: any cut of the stream into calls gives the same
//                                    bits, and they are the bits of two iq_mix_kernel launches.
// The access scheme is iq_mix_kernel's: a thread takes IQX_Q consecutive samples that start on a 16-byte boundary of the
// destination streams (all four share their 16-byte phase; the launcher checks it), one 16-byte store to each of the four.  Every
// source is judged on its own: one that is 16-byte aligned at the first quad is read with 16-byte loads (planar: one a stream;
// interleaved: two a side), any other with 4-byte loads (planar) or 8-byte loads (interleaved: a pair is 8-byte aligned).  Thread 0
// takes the up to three samples in front of the first boundary; the thread of the last quad takes the partial one.
// Shared oscillator: where both sides have the same ftw AND the same phase0 (two receivers tuned alike; kernel arguments, so the
// branch is wave-uniform), zoom_lo is evaluated once a sample and its (c, s) turns both sides through iq_rotate -- iq_mix is
// zoom_lo followed by iq_rotate, so the bits are those of two evaluations.  Equal ftw with different phase0 is two oscillators.
// No LDS, no scratch.
#include "iq_cross.h"
#include "iq_lo.h"

namespace psdk {

constexpr int IQX_Q = 4, IQX_BLOCK = 256;

namespace {

// complex sample i of one side, from either layout (interleaved: si points to the side's pairs)
template <bool INTERLEAVED>
__device__ __forceinline__ void iqx_load1(const float *si, const float *sq, unsigned long long i, float &a, float &b)
{
    if constexpr (INTERLEAVED) {
        const float2 z = *reinterpret_cast<const float2 *>(si + 2 * i);
        a = z.x, b = z.y;
    } else {
        a = si[i], b = sq[i];
    }
}

// the four complex samples i0 ... i0 + 3 of one side; al_i / al_q: the I stream (interleaved: the pairs) / the Q stream is 16-byte
// aligned there
template <bool INTERLEAVED>
__device__ __forceinline__ void iqx_load4(const float *si, const float *sq, unsigned long long i0, bool al_i, bool al_q, float4 &a,
                                          float4 &b)
{
    if constexpr (INTERLEAVED) {
        const float *p = si + 2 * i0;
        if (al_i) {
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
        if (al_i)
            a = *reinterpret_cast<const float4 *>(si + i0);
        else
            a = make_float4(si[i0], si[i0 + 1], si[i0 + 2], si[i0 + 3]);
        if (al_q)
            b = *reinterpret_cast<const float4 *>(sq + i0);
        else
            b = make_float4(sq[i0], sq[i0 + 1], sq[i0 + 2], sq[i0 + 3]);
    }
}

// samples [i, end) of both sides one by one (the head and the partial last quad), the first at phases pa, pb
template <bool INTERLEAVED>
__device__ __forceinline__ void iqx_singles(const IqPairMixJob &job, unsigned long long i, unsigned long long end,
                                            unsigned long long pa, unsigned long long pb, bool shared)
{
    for (; i < end; ++i, pa += job.ftw[0], pb += job.ftw[1]) {
        float ia, qa, ib, qb;
        iqx_load1<INTERLEAVED>(job.src[0], job.src[1], i, ia, qa);
        iqx_load1<INTERLEAVED>(job.src[2], job.src[3], i, ib, qb);
        if (shared) {
            float c, s;
            zoom_lo(pa, c, s);
            iq_rotate(ia, qa, c, s, job.dst[0][i], job.dst[1][i]);
            iq_rotate(ib, qb, c, s, job.dst[2][i], job.dst[3][i]);
        } else {
            iq_mix(ia, qa, pa, job.dst[0][i], job.dst[1][i]);
            iq_mix(ib, qb, pb, job.dst[2][i], job.dst[3][i]);
        }
    }
}

} // namespace

// src_aligned: bit c -- src[c] is 16-byte aligned at the first quad (interleaved: bits 0 and 2, the pairs of side a and side b)
template <bool INTERLEAVED>
__global__ __launch_bounds__(IQX_BLOCK) void iq_pair_mix_kernel(const IqPairMixJob job, const unsigned head, const int src_aligned)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * IQX_BLOCK + threadIdx.x;
    const bool shared = job.ftw[0] == job.ftw[1] && job.phase0[0] == job.phase0[1]; // wave-uniform
    if (g == 0) {
        iqx_singles<INTERLEAVED>(job, 0, head, job.phase0[0] + job.ftw[0] * job.j0, job.phase0[1] + job.ftw[1] * job.j0, shared);
        return;
    }
    const unsigned long long i0 = head + (g - 1) * IQX_Q;
    if (i0 >= job.len)
        return;
    unsigned long long pa = job.phase0[0] + job.ftw[0] * (job.j0 + i0), pb = job.phase0[1] + job.ftw[1] * (job.j0 + i0);
    if (job.len - i0 < IQX_Q) {
        iqx_singles<INTERLEAVED>(job, i0, job.len, pa, pb, shared);
        return;
    }
    float4 ai, aq, bi, bq;
    iqx_load4<INTERLEAVED>(job.src[0], job.src[1], i0, src_aligned & 1, src_aligned & 2, ai, aq);
    iqx_load4<INTERLEAVED>(job.src[2], job.src[3], i0, src_aligned & 4, src_aligned & 8, bi, bq);
    float4 via, vqa, vib, vqb;
    if (shared) { // one carrier on both sides: one oscillator a sample
        float c, s;
        zoom_lo(pa, c, s);
        iq_rotate(ai.x, aq.x, c, s, via.x, vqa.x);
        iq_rotate(bi.x, bq.x, c, s, vib.x, vqb.x);
        zoom_lo(pa += job.ftw[0], c, s);
        iq_rotate(ai.y, aq.y, c, s, via.y, vqa.y);
        iq_rotate(bi.y, bq.y, c, s, vib.y, vqb.y);
        zoom_lo(pa += job.ftw[0], c, s);
        iq_rotate(ai.z, aq.z, c, s, via.z, vqa.z);
        iq_rotate(bi.z, bq.z, c, s, vib.z, vqb.z);
        zoom_lo(pa += job.ftw[0], c, s);
        iq_rotate(ai.w, aq.w, c, s, via.w, vqa.w);
        iq_rotate(bi.w, bq.w, c, s, vib.w, vqb.w);
    } else {
        iq_mix(ai.x, aq.x, pa, via.x, vqa.x);
        iq_mix(ai.y, aq.y, pa += job.ftw[0], via.y, vqa.y);
        iq_mix(ai.z, aq.z, pa += job.ftw[0], via.z, vqa.z);
        iq_mix(ai.w, aq.w, pa += job.ftw[0], via.w, vqa.w);
        iq_mix(bi.x, bq.x, pb, vib.x, vqb.x);
        iq_mix(bi.y, bq.y, pb += job.ftw[1], vib.y, vqb.y);
        iq_mix(bi.z, bq.z, pb += job.ftw[1], vib.z, vqb.z);
        iq_mix(bi.w, bq.w, pb += job.ftw[1], vib.w, vqb.w);
    }
    *reinterpret_cast<float4 *>(job.dst[0] + i0) = via;
    *reinterpret_cast<float4 *>(job.dst[1] + i0) = vqa;
    *reinterpret_cast<float4 *>(job.dst[2] + i0) = vib;
    *reinterpret_cast<float4 *>(job.dst[3] + i0) = vqb;
}

hipError_t launch_iq_pair_mix(const IqPairMixJob &j, bool interleaved, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    for (int c = 0; c < 4; ++c) {
        if (!j.dst[c] || ((uintptr_t)j.dst[c] & 3) || (((uintptr_t)j.dst[0] ^ (uintptr_t)j.dst[c]) & 15))
            return hipErrorInvalidValue;
        if (interleaved && (c & 1))
            continue;
        if (!j.src[c] || ((uintptr_t)j.src[c] & (interleaved ? 7 : 3)))
            return hipErrorInvalidValue;
    }
    const unsigned long long lead = (4 - (((uintptr_t)j.dst[0] >> 2) & 3)) & 3;
    const unsigned head = (unsigned)(lead < j.len ? lead : j.len);
    const unsigned long long quads = (j.len - head + IQX_Q - 1) / IQX_Q;
    const unsigned long long blocks = (quads + 1 + IQX_BLOCK - 1) / IQX_BLOCK;
    if (blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    int src_aligned = 0;
    for (int c = 0; c < 4; ++c) {
        if (interleaved && (c & 1))
            continue;
        const float *first = j.src[c] + (interleaved ? 2 : 1) * (size_t)head;
        src_aligned |= ((uintptr_t)first & 15) == 0 ? 1 << c : 0;
    }
    if (interleaved)
        hipLaunchKernelGGL(iq_pair_mix_kernel<true>, dim3((unsigned)blocks), dim3(IQX_BLOCK), 0, s, j, head, src_aligned);
    else
        hipLaunchKernelGGL(iq_pair_mix_kernel<false>, dim3((unsigned)blocks), dim3(IQX_BLOCK), 0, s, j, head, src_aligned);
    return hipGetLastError();
}

} // namespace psdk
