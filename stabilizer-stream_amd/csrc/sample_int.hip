// sample_int.hip -- gfx950 kernels of the integer sample feeds (psdc_int_*, cross_runtime.cpp): the three mixers in front of
// stage 0 reading int16 / int8 samples in place of f32.
//
//   zoom_mix_int_kernel<T>     zoom_mix_kernel (zoom.hip) on real integers
//   iq_mix_int_kernel<T>       iq_mix_kernel<true> (iq.hip) on interleaved (re, im) integer pairs
//   iq_pair_mix_int_kernel<T>  iq_pair_mix_kernel<true> (iq_cross.hip) on the integer pairs of both sides, shared oscillator included
//   sample_cvt_int_kernel<T>   the converter of the objects with no mixer (psdc_sint_*): 1 ... 4 channels of real integers to f32
// T = int16_t or int8_t.  A thread's work is sample_int.h's sint_*_thread (the same source the host check runs): the f32 mixers'
// access scheme, a sample converted as __fmul_rn((float)v, scale) in registers and mixed by zoom_lo.h / iq_lo.h unchanged, so a
// launch stores the bits the f32 kernel stores for the converted stream.  The f32 kernels and their TUs are untouched.
// No LDS, no scratch.
#include "sample_int.h"

namespace psdk {

template <typename T>
__global__ __launch_bounds__(SINT_BLOCK) void zoom_mix_int_kernel(const SintMixJob job, const unsigned head, const int src_aligned)
{
    sint_zoom_thread<T>(job, head, src_aligned != 0, (unsigned long long)blockIdx.x * SINT_BLOCK + threadIdx.x);
}

template <typename T>
__global__ __launch_bounds__(SINT_BLOCK) void iq_mix_int_kernel(const SintMixJob job, const unsigned head, const int src_aligned)
{
    sint_iq_thread<T>(job, head, src_aligned != 0, (unsigned long long)blockIdx.x * SINT_BLOCK + threadIdx.x);
}

template <typename T>
__global__ __launch_bounds__(SINT_BLOCK) void iq_pair_mix_int_kernel(const SintPairMixJob job, const unsigned head, const int src_aligned)
{
    sint_iq_pair_thread<T>(job, head, src_aligned, (unsigned long long)blockIdx.x * SINT_BLOCK + threadIdx.x);
}

// grid: x -- the groups of a channel, y -- the channel
template <typename T>
__global__ __launch_bounds__(SINT_BLOCK) void sample_cvt_int_kernel(const SintCvtJob job, const unsigned head, const int src_aligned_mask)
{
    sint_cvt_thread<T>(job, head, src_aligned_mask, blockIdx.y, (unsigned long long)blockIdx.x * SINT_BLOCK + threadIdx.x);
}

namespace {

// the launch's grid, or 0 if it does not fit
unsigned sint_blocks(unsigned head, unsigned long long len)
{
    const unsigned long long blocks = (sint_threads(head, len) + SINT_BLOCK - 1) / SINT_BLOCK;
    return blocks > 0x7FFFFFFFull ? 0u : (unsigned)blocks;
}

bool sint_dst_ok(const float *d0, const float *d)
{
    return d && !((uintptr_t)d & 3) && !(((uintptr_t)d0 ^ (uintptr_t)d) & 15);
}

} // namespace

hipError_t launch_zoom_mix_int(const SintMixJob &j, int kind, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    const size_t unit = (size_t)sint_bytes(kind);
    if (!unit || !j.src || (uintptr_t)j.src % unit || !sint_dst_ok(j.dst_i, j.dst_i) || !sint_dst_ok(j.dst_i, j.dst_q))
        return hipErrorInvalidValue;
    const unsigned head = sint_head(j.dst_i, j.len), blocks = sint_blocks(head, j.len);
    if (!blocks)
        return hipErrorInvalidValue;
    const int al = sint_src_aligned(j.src, head, unit);
    if (kind == SAMPLE_S16)
        hipLaunchKernelGGL(zoom_mix_int_kernel<int16_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    else
        hipLaunchKernelGGL(zoom_mix_int_kernel<int8_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    return hipGetLastError();
}

hipError_t launch_iq_mix_int(const SintMixJob &j, int kind, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    const size_t unit = 2 * (size_t)sint_bytes(kind);
    if (!unit || !j.src || (uintptr_t)j.src % unit || !sint_dst_ok(j.dst_i, j.dst_i) || !sint_dst_ok(j.dst_i, j.dst_q))
        return hipErrorInvalidValue;
    const unsigned head = sint_head(j.dst_i, j.len), blocks = sint_blocks(head, j.len);
    if (!blocks)
        return hipErrorInvalidValue;
    const int al = sint_src_aligned(j.src, head, unit);
    if (kind == SAMPLE_S16)
        hipLaunchKernelGGL(iq_mix_int_kernel<int16_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    else
        hipLaunchKernelGGL(iq_mix_int_kernel<int8_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    return hipGetLastError();
}

hipError_t launch_iq_pair_mix_int(const SintPairMixJob &j, int kind, hipStream_t s)
{
    if (j.len == 0)
        return hipSuccess;
    const size_t unit = 2 * (size_t)sint_bytes(kind);
    if (!unit)
        return hipErrorInvalidValue;
    for (int c = 0; c < 4; ++c)
        if (!sint_dst_ok(j.dst[0], j.dst[c]))
            return hipErrorInvalidValue;
    for (int side = 0; side < 2; ++side)
        if (!j.src[side] || (uintptr_t)j.src[side] % unit)
            return hipErrorInvalidValue;
    const unsigned head = sint_head(j.dst[0], j.len), blocks = sint_blocks(head, j.len);
    if (!blocks)
        return hipErrorInvalidValue;
    const int al = (sint_src_aligned(j.src[0], head, unit) ? 1 : 0) | (sint_src_aligned(j.src[1], head, unit) ? 2 : 0);
    if (kind == SAMPLE_S16)
        hipLaunchKernelGGL(iq_pair_mix_int_kernel<int16_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    else
        hipLaunchKernelGGL(iq_pair_mix_int_kernel<int8_t>, dim3(blocks), dim3(SINT_BLOCK), 0, s, j, head, al);
    return hipGetLastError();
}

hipError_t launch_cvt_int(const SintCvtJob &j, int kind, hipStream_t s)
{
    const size_t unit = (size_t)sint_bytes(kind);
    if (!unit || j.nch < 1 || j.nch > 4)
        return hipErrorInvalidValue;
    if (j.len == 0)
        return hipSuccess;
    for (unsigned c = 0; c < j.nch; ++c)
        if (!j.src[c] || (uintptr_t)j.src[c] % unit || !sint_dst_ok(j.dst[0], j.dst[c]))
            return hipErrorInvalidValue;
    const unsigned head = sint_head(j.dst[0], j.len), blocks = sint_blocks(head, j.len);
    if (!blocks)
        return hipErrorInvalidValue;
    int al = 0;
    for (unsigned c = 0; c < j.nch; ++c)
        al |= (sint_src_aligned(j.src[c], head, unit) ? 1 : 0) << c;
    if (kind == SAMPLE_S16)
        hipLaunchKernelGGL(sample_cvt_int_kernel<int16_t>, dim3(blocks, j.nch), dim3(SINT_BLOCK), 0, s, j, head, al);
    else
        hipLaunchKernelGGL(sample_cvt_int_kernel<int8_t>, dim3(blocks, j.nch), dim3(SINT_BLOCK), 0, s, j, head, al);
    return hipGetLastError();
}

} // namespace psdk
