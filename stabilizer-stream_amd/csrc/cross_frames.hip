// cross_frames.hip -- gfx950 kernel that decodes stream frames straight into the stage-0 x / y buffers of cross pairs
// (psdc_csd_process_frames[_device], cross_runtime.cpp).
//
//   cross_frames_kernel<FMT>  each (frame, batch, trace) cell of the traces in use is read and converted ONCE, and its f32 samples
//                             are stored to every destination that takes the trace.  The arithmetic is frames.h's (adcdac_volts,
//                             payload_trace): the same bits as adcdac_kernel / payload_kernel, i.e. Payload::traces.
// AdcDac: one thread per (frame, batch): the batch's 64 bytes are contiguous and so are the threads' (a frame's 8 header bytes
// aside), each cell of 16 bytes is two 8-byte loads when the frames are 8-byte aligned (the header is 8 bytes and a batch 64:
// every cell is then aligned), bytes otherwise; a destination takes 8 samples as two 16-byte stores when its base is 16-byte
// aligned, dword stores otherwise.  Fls / ThermostatEem / Mpll (one sample per batch and trace): one thread per four consecutive
// batches, so that a destination again takes one 16-byte store.
#include "cross.h"
#include "frames.h"

namespace psdk {

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_MAX_BLOCKS = 4096;
constexpr int CF_RUN = 4; // batches a thread of the one-sample formats

__device__ __forceinline__ bool aligned16(const float *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int FMT, int T, class Word>
__device__ __forceinline__ void decode_trace(const Word &word, unsigned used, float &out)
{
    if constexpr (T < wire_fmt_v(FMT).ntraces)
        if ((used >> T) & 1u)
            out = payload_trace<FMT, T>(word);
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(CF_THREADS) void cross_frames_kernel(const CrossFramesBatch b)
{
    const unsigned batches = (unsigned)b.batches;
    const unsigned total = b.n_frames * batches; // batches in the launch (< 2^23: the host cuts pieces of <= 2^22 samples a trace)
    unsigned used = 0, al16 = 0;                 // traces in use, destinations with a 16-byte aligned base (wave-uniform)
    for (int k = 0; k < b.ndst; ++k) {
        used |= 1u << b.trace[k];
        al16 |= (aligned16(b.dst[k]) ? 1u : 0u) << k;
    }
    if constexpr (FMT == 1) {
        const bool al8 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 7u) == 0;
        for (unsigned g = blockIdx.x * CF_THREADS + threadIdx.x; g < total; g += gridDim.x * CF_THREADS) {
            const unsigned f = g / batches, bb = g - f * batches;
            const uint8_t *p = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * 64;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (!((used >> t) & 1u))
                    continue;
                const uint8_t *q = p + t * 16;
                uint32_t w[4];
                if (al8) {
                    const uint2 lo = *reinterpret_cast<const uint2 *>(q), hi = *reinterpret_cast<const uint2 *>(q + 8);
                    w[0] = lo.x, w[1] = lo.y, w[2] = hi.x, w[3] = hi.y;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        w[i] = (uint32_t)q[4 * i] | ((uint32_t)q[4 * i + 1] << 8) | ((uint32_t)q[4 * i + 2] << 16) |
                               ((uint32_t)q[4 * i + 3] << 24);
                }
                float v[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = adcdac_volts(w[i] & 0xffffu, t >= 2);
                    v[2 * i + 1] = adcdac_volts(w[i] >> 16, t >= 2);
                }
                for (int k = 0; k < b.ndst; ++k) {
                    if (b.trace[k] != t)
                        continue;
                    float *d = b.dst[k] + (size_t)g * 8;
                    if ((al16 >> k) & 1u) {
                        reinterpret_cast<float4 *>(d)[0] = make_float4(v[0], v[1], v[2], v[3]);
                        reinterpret_cast<float4 *>(d)[1] = make_float4(v[4], v[5], v[6], v[7]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            d[i] = v[i];
                    }
                }
            }
        }
    } else {
        constexpr int BB = wire_fmt_v(FMT).batch_bytes;
        constexpr int NT = wire_fmt_v(FMT).ntraces;
        const bool al4 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 3u) == 0;
        const unsigned runs = (total + CF_RUN - 1) / CF_RUN;
        for (unsigned r = blockIdx.x * CF_THREADS + threadIdx.x; r < runs; r += gridDim.x * CF_THREADS) {
            const unsigned g0 = r * CF_RUN;
            unsigned f = g0 / batches, bb = g0 - f * batches;
            float v[4][CF_RUN] = {};
#pragma unroll
            for (int c = 0; c < CF_RUN; ++c) {
                if (g0 + c < total) {
                    const uint8_t *p = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * BB;
                    auto word = [&](int i) { return payload_word(p, i, al4); };
                    decode_trace<FMT, 0>(word, used, v[0][c]);
                    decode_trace<FMT, 1>(word, used, v[1][c]);
                    decode_trace<FMT, 2>(word, used, v[2][c]);
                    decode_trace<FMT, 3>(word, used, v[3][c]);
                }
                if (++bb == batches)
                    bb = 0, ++f;
            }
            const bool full = g0 + CF_RUN <= total;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (!((used >> t) & 1u))
                    continue;
                for (int k = 0; k < b.ndst; ++k) {
                    if (b.trace[k] != t)
                        continue;
                    float *d = b.dst[k] + g0;
                    if (full && ((al16 >> k) & 1u)) {
                        *reinterpret_cast<float4 *>(d) = make_float4(v[t][0], v[t][1], v[t][2], v[t][3]);
                    } else {
#pragma unroll
                        for (int c = 0; c < CF_RUN; ++c)
                            if (g0 + c < total)
                                d[c] = v[t][c];
                    }
                }
            }
        }
    }
}

hipError_t launch_cross_frames(const CrossFramesBatch &b, hipStream_t s)
{
    if (b.ndst < 1 || b.ndst > CROSS_FRAMES_MAX_DST || b.batches < 1 || b.fmt < 1 || b.fmt > 4)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)b.n_frames * (unsigned)b.batches;
    if (total == 0)
        return hipSuccess;
    if (total >= (1ull << 31))
        return hipErrorInvalidValue;
    for (int k = 0; k < b.ndst; ++k)
        if (!b.dst[k] || b.trace[k] < 0 || b.trace[k] >= wire_fmt_v(b.fmt).ntraces)
            return hipErrorInvalidValue;
    const unsigned long long items = b.fmt == 1 ? total : (total + CF_RUN - 1) / CF_RUN;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(CF_MAX_BLOCKS, (items + CF_THREADS - 1) / CF_THREADS);
    if (b.fmt == 1)
        hipLaunchKernelGGL(cross_frames_kernel<1>, dim3(blocks), dim3(CF_THREADS), 0, s, b);
    else if (b.fmt == 2)
        hipLaunchKernelGGL(cross_frames_kernel<2>, dim3(blocks), dim3(CF_THREADS), 0, s, b);
    else if (b.fmt == 3)
        hipLaunchKernelGGL(cross_frames_kernel<3>, dim3(blocks), dim3(CF_THREADS), 0, s, b);
    else
        hipLaunchKernelGGL(cross_frames_kernel<4>, dim3(blocks), dim3(CF_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
