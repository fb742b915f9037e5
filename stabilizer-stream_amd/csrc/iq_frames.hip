// iq_frames.hip -- gfx950 kernel that decodes stream frames and mixes two traces of them, as I and Q of one complex stream, straight
// into the stage-0 I / Q streams of IQ channels (psdc_iq_process_frames[_device], cross_runtime.cpp).
//
//   iq_frames_kernel<FMT>  the work decomposition of cross_frames_kernel<FMT> / zoom_frames_kernel<FMT> with the arithmetic of
//                          iq_mix_kernel: each (frame, batch, trace) cell of the traces in use is read and converted ONCE (frames.h:
//                          adcdac_volts, payload_trace -- the bits of Payload::traces), and for every channel whose (i_trace, q_trace)
//                          it feeds the two samples are mixed in registers (iq_lo.h's iq_mix) with that channel's ftw, phase0 and
//                          stream index and stored to its I and Q streams.  The f32 traces never exist in memory.
// Sample i of the launch is stream sample j0 + i of a channel and has the phase phase0 + ftw (j0 + i) mod 2^64, from the index in
// 64-bit integers as in iq_mix_kernel: the same bits as the decoded traces through iq_mix_kernel, however the frames are cut.
// AdcDac: one thread per (frame, batch), 8 samples a trace; a cell is two 8-byte loads when base and frame size are 8-byte aligned,
// bytes otherwise; a channel takes the 8 samples as two 16-byte stores to each of I and Q when its position in the streams is
// 16-byte aligned (I and Q share their 16-byte phase), dword stores otherwise.  Fls / ThermostatEem / Mpll: one thread per four
// consecutive batches, one 16-byte store to each stream; the last partial run is stored sample by sample.
// A channel's two traces are picked from the thread's decoded cells with selects on constant indices (the trace numbers are
// wave-uniform kernel arguments): no register array is indexed at run time, so nothing goes to scratch.
#include "iq.h"
#include "frames.h"
#include "iq_lo.h"

namespace psdk {

namespace {

constexpr int QF_THREADS = 256;
constexpr int QF_MAX_BLOCKS = 4096;
constexpr int QF_RUN = 4; // batches a thread of the one-sample formats

template <int FMT, int T, class Word>
__device__ __forceinline__ void qf_decode_trace(const Word &word, unsigned used, float &out)
{
    if constexpr (T < wire_fmt_v(FMT).ntraces)
        if ((used >> T) & 1u)
            out = payload_trace<FMT, T>(word);
}

// CNT consecutive samples of one channel, the first at stream index j0 + i0: I from trace ti and Q from trace tq of the thread's
// decoded cells v[trace][sample], mixed and stored at I / Q position i0
template <int CNT>
__device__ __forceinline__ void qf_mix_store(const IqFramesBatch &b, int k, const float (&v)[4][CNT], int ti, int tq, size_t i0,
                                             bool al16, unsigned valid)
{
    const unsigned long long ftw = b.ftw[k];
    unsigned long long ph = b.phase0[k] + ftw * (b.j0[k] + i0);
    float vi[CNT], vq[CNT];
#pragma unroll
    for (int i = 0; i < CNT; ++i, ph += ftw) {
        const float a = ti == 0 ? v[0][i] : ti == 1 ? v[1][i] : ti == 2 ? v[2][i] : v[3][i];
        const float c = tq == 0 ? v[0][i] : tq == 1 ? v[1][i] : tq == 2 ? v[2][i] : v[3][i];
        iq_mix(a, c, ph, vi[i], vq[i]);
    }
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
__global__ __launch_bounds__(QF_THREADS) void iq_frames_kernel(const IqFramesBatch b)
{
    const unsigned batches = (unsigned)b.batches;
    const unsigned total = b.n_frames * batches; // batches in the launch (< 2^23: the host cuts pieces of <= 2^22 samples a trace)
    unsigned used = 0, al16 = 0;                 // traces in use, channels at a 16-byte aligned stream position (wave-uniform)
    for (int k = 0; k < b.nch; ++k) {
        used |= (1u << b.trace_i[k]) | (1u << b.trace_q[k]);
        al16 |= ((reinterpret_cast<uintptr_t>(b.dst_i[k]) & 15u) == 0 ? 1u : 0u) << k;
    }
    if constexpr (FMT == 1) {
        const bool al8 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 7u) == 0;
        for (unsigned g = blockIdx.x * QF_THREADS + threadIdx.x; g < total; g += gridDim.x * QF_THREADS) {
            const unsigned f = g / batches, bb = g - f * batches;
            const uint8_t *p = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * 64;
            float v[4][8] = {};
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
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[t][2 * i] = adcdac_volts(w[i] & 0xffffu, t >= 2);
                    v[t][2 * i + 1] = adcdac_volts(w[i] >> 16, t >= 2);
                }
            }
            for (int k = 0; k < b.nch; ++k)
                qf_mix_store<8>(b, k, v, b.trace_i[k], b.trace_q[k], (size_t)g * 8, (al16 >> k) & 1u, 8);
        }
    } else {
        constexpr int BB = wire_fmt_v(FMT).batch_bytes;
        const bool al4 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 3u) == 0;
        const unsigned runs = (total + QF_RUN - 1) / QF_RUN;
        for (unsigned r = blockIdx.x * QF_THREADS + threadIdx.x; r < runs; r += gridDim.x * QF_THREADS) {
            const unsigned g0 = r * QF_RUN;
            unsigned f = g0 / batches, bb = g0 - f * batches;
            float v[4][QF_RUN] = {};
#pragma unroll
            for (int c = 0; c < QF_RUN; ++c) {
                if (g0 + c < total) {
                    const uint8_t *p = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * BB;
                    auto word = [&](int i) { return payload_word(p, i, al4); };
                    qf_decode_trace<FMT, 0>(word, used, v[0][c]);
                    qf_decode_trace<FMT, 1>(word, used, v[1][c]);
                    qf_decode_trace<FMT, 2>(word, used, v[2][c]);
                    qf_decode_trace<FMT, 3>(word, used, v[3][c]);
                }
                if (++bb == batches)
                    bb = 0, ++f;
            }
            const unsigned valid = total - g0 < (unsigned)QF_RUN ? total - g0 : (unsigned)QF_RUN;
            for (int k = 0; k < b.nch; ++k)
                qf_mix_store<QF_RUN>(b, k, v, b.trace_i[k], b.trace_q[k], (size_t)g0, (al16 >> k) & 1u, valid);
        }
    }
}

hipError_t launch_iq_frames(const IqFramesBatch &b, hipStream_t s)
{
    if (b.nch < 1 || b.nch > ZOOM_FRAMES_MAX_CH || b.batches < 1 || b.fmt < 1 || b.fmt > 4)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)b.n_frames * (unsigned)b.batches;
    if (total == 0)
        return hipSuccess;
    if (total >= (1ull << 31))
        return hipErrorInvalidValue;
    const int nt = wire_fmt_v(b.fmt).ntraces;
    for (int k = 0; k < b.nch; ++k)
        if (!b.dst_i[k] || !b.dst_q[k] || ((uintptr_t)b.dst_i[k] & 3) || (((uintptr_t)b.dst_i[k] ^ (uintptr_t)b.dst_q[k]) & 15) ||
            b.trace_i[k] < 0 || b.trace_i[k] >= nt || b.trace_q[k] < 0 || b.trace_q[k] >= nt)
            return hipErrorInvalidValue;
    const unsigned long long items = b.fmt == 1 ? total : (total + QF_RUN - 1) / QF_RUN;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(QF_MAX_BLOCKS, (items + QF_THREADS - 1) / QF_THREADS);
    if (b.fmt == 1)
        hipLaunchKernelGGL(iq_frames_kernel<1>, dim3(blocks), dim3(QF_THREADS), 0, s, b);
    else if (b.fmt == 2)
        hipLaunchKernelGGL(iq_frames_kernel<2>, dim3(blocks), dim3(QF_THREADS), 0, s, b);
    else if (b.fmt == 3)
        hipLaunchKernelGGL(iq_frames_kernel<3>, dim3(blocks), dim3(QF_THREADS), 0, s, b);
    else
        hipLaunchKernelGGL(iq_frames_kernel<4>, dim3(blocks), dim3(QF_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
