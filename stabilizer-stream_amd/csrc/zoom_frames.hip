// zoom_frames.hip -- gfx950 kernel that decodes stream frames and mixes them straight into the stage-0 I / Q streams of zoom
// channels (psdc_zoomcascade_process_frames[_device], cross_runtime.cpp).
//
//   zoom_frames_kernel<FMT>  the work decomposition of cross_frames_kernel<FMT> with the arithmetic of zoom_mix_kernel: each
//                            (frame, batch, trace) cell of the traces in use is read and converted ONCE (frames.h: adcdac_volts,
//                            payload_trace -- the bits of Payload::traces), and for every channel that takes the trace the samples
//                            are mixed in registers (zoom_lo.h's zoom_mix) with that channel's ftw, phase0 and stream index and
//                            stored to its I and Q streams.  The f32 trace never exists in memory.
// Sample i of the launch is stream sample j0 + i of a channel and has the phase phase0 + ftw (j0 + i) mod 2^64, from the index in
// 64-bit integers as in zoom_mix_kernel: the same bits as the decoded trace through zoom_mix_kernel, however the frames are cut.
// AdcDac: one thread per (frame, batch), 8 samples a trace; a cell is two 8-byte loads when base and frame size are 8-byte aligned,
// bytes otherwise; a channel takes the 8 samples as two 16-byte stores to each of I and Q when its position in the streams is
// 16-byte aligned (I and Q share their 16-byte phase), dword stores otherwise.  Fls / ThermostatEem / Mpll: one thread per four
// consecutive batches, one 16-byte store to each stream; the last partial run is stored sample by sample.
#include "zoom.h"
#include "frames.h"
#include "zoom_lo.h"

namespace psdk {

namespace {

constexpr int ZF_THREADS = 256;
constexpr int ZF_MAX_BLOCKS = 4096;
constexpr int ZF_RUN = 4; // batches a thread of the one-sample formats

template <int FMT, int T, class Word>
__device__ __forceinline__ void zf_decode_trace(const Word &word, unsigned used, float &out)
{
    if constexpr (T < wire_fmt_v(FMT).ntraces)
        if ((used >> T) & 1u)
            out = payload_trace<FMT, T>(word);
}

// CNT consecutive samples of one channel, the first at stream index j0 + i0: mixed and stored at I / Q position i0
template <int CNT>
__device__ __forceinline__ void zf_mix_store(const ZoomFramesBatch &b, int k, const float *v, size_t i0, bool al16, unsigned valid)
{
    const unsigned long long ftw = b.ftw[k];
    unsigned long long ph = b.phase0[k] + ftw * (b.j0[k] + i0);
    float vi[CNT], vq[CNT];
#pragma unroll
    for (int i = 0; i < CNT; ++i, ph += ftw)
        zoom_mix(v[i], ph, vi[i], vq[i]);
    float *di = b.dst_i[k] + i0, *dq = b.dst_q[k] + i0;
    if (al16 && valid == CNT) {
#pragma unroll
        for (int i = 0; i < CNT; i += 4) {
            *reinterpret_cast<float4 *>(di + i) = make_float4(vi[i], vi[i + 1], vi[i + 2], vi[i + 3]);
            *reinterpret_cast<float4 *>(dq + i) = make_float4(vq[i], vq[i + 1], vq[i + 2], vq[i + 3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CNT; ++i)
            if ((unsigned)i < valid) {
                di[i] = vi[i];
                dq[i] = vq[i];
            }
    }
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(ZF_THREADS) void zoom_frames_kernel(const ZoomFramesBatch b)
{
    const unsigned batches = (unsigned)b.batches;
    const unsigned total = b.n_frames * batches; // batches in the launch (< 2^23: the host cuts pieces of <= 2^22 samples a trace)
    unsigned used = 0, al16 = 0;                 // traces in use, channels at a 16-byte aligned stream position (wave-uniform)
    for (int k = 0; k < b.nch; ++k) {
        used |= 1u << b.trace[k];
        al16 |= ((reinterpret_cast<uintptr_t>(b.dst_i[k]) & 15u) == 0 ? 1u : 0u) << k;
    }
    if constexpr (FMT == 1) {
        const bool al8 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 7u) == 0;
        for (unsigned g = blockIdx.x * ZF_THREADS + threadIdx.x; g < total; g += gridDim.x * ZF_THREADS) {
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
                for (int k = 0; k < b.nch; ++k)
                    if (b.trace[k] == t)
                        zf_mix_store<8>(b, k, v, (size_t)g * 8, (al16 >> k) & 1u, 8);
            }
        }
    } else {
        constexpr int BB = wire_fmt_v(FMT).batch_bytes;
        constexpr int NT = wire_fmt_v(FMT).ntraces;
        const bool al4 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 3u) == 0;
        const unsigned runs = (total + ZF_RUN - 1) / ZF_RUN;
        for (unsigned r = blockIdx.x * ZF_THREADS + threadIdx.x; r < runs; r += gridDim.x * ZF_THREADS) {
            const unsigned g0 = r * ZF_RUN;
            unsigned f = g0 / batches, bb = g0 - f * batches;
            float v[4][ZF_RUN] = {};
#pragma unroll
            for (int c = 0; c < ZF_RUN; ++c) {
                if (g0 + c < total) {
                    const uint8_t *p = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * BB;
                    auto word = [&](int i) { return payload_word(p, i, al4); };
                    zf_decode_trace<FMT, 0>(word, used, v[0][c]);
                    zf_decode_trace<FMT, 1>(word, used, v[1][c]);
                    zf_decode_trace<FMT, 2>(word, used, v[2][c]);
                    zf_decode_trace<FMT, 3>(word, used, v[3][c]);
                }
                if (++bb == batches)
                    bb = 0, ++f;
            }
            const unsigned valid = total - g0 < (unsigned)ZF_RUN ? total - g0 : (unsigned)ZF_RUN;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (!((used >> t) & 1u))
                    continue;
                for (int k = 0; k < b.nch; ++k)
                    if (b.trace[k] == t)
                        zf_mix_store<ZF_RUN>(b, k, v[t], (size_t)g0, (al16 >> k) & 1u, valid);
            }
        }
    }
}

hipError_t launch_zoom_frames(const ZoomFramesBatch &b, hipStream_t s)
{
    if (b.nch < 1 || b.nch > ZOOM_FRAMES_MAX_CH || b.batches < 1 || b.fmt < 1 || b.fmt > 4)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)b.n_frames * (unsigned)b.batches;
    if (total == 0)
        return hipSuccess;
    if (total >= (1ull << 31))
        return hipErrorInvalidValue;
    for (int k = 0; k < b.nch; ++k)
        if (!b.dst_i[k] || !b.dst_q[k] || ((uintptr_t)b.dst_i[k] & 3) || (((uintptr_t)b.dst_i[k] ^ (uintptr_t)b.dst_q[k]) & 15) ||
            b.trace[k] < 0 || b.trace[k] >= wire_fmt_v(b.fmt).ntraces)
            return hipErrorInvalidValue;
    const unsigned long long items = b.fmt == 1 ? total : (total + ZF_RUN - 1) / ZF_RUN;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(ZF_MAX_BLOCKS, (items + ZF_THREADS - 1) / ZF_THREADS);
    if (b.fmt == 1)
        hipLaunchKernelGGL(zoom_frames_kernel<1>, dim3(blocks), dim3(ZF_THREADS), 0, s, b);
    else if (b.fmt == 2)
        hipLaunchKernelGGL(zoom_frames_kernel<2>, dim3(blocks), dim3(ZF_THREADS), 0, s, b);
    else if (b.fmt == 3)
        hipLaunchKernelGGL(zoom_frames_kernel<3>, dim3(blocks), dim3(ZF_THREADS), 0, s, b);
    else
        hipLaunchKernelGGL(zoom_frames_kernel<4>, dim3(blocks), dim3(ZF_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
