// iq_cross_frames.hip -- gfx950 kernel that decodes stream frames and mixes four traces of them, as I and Q of two complex streams,
// straight into the four stage-0 streams (I_a, Q_a, I_b, Q_b) of IQ cross pairs (psdc_iqcsd_process_frames[_device],
// cross_runtime.cpp).
//
//   iq_cross_frames_kernel<FMT>  zoom_cross_frames_kernel<FMT> with two traces a side: each (frame, batch, trace) cell of the traces
//                                in use is read and converted ONCE a thread (frames.h: adcdac_volts, payload_trace -- the bits of
//                                Payload::traces) and then handed to every entry of every pair that takes it; a side's I and Q are
//                                turned in registers by the side's carrier (iq_lo.h's iq_mix) and stored to its two streams.  The
//                                f32 traces never exist in memory.
// Sample i of the launch is stream sample j0 + i of both sides of a pair and has the phase phase0 + ftw (j0 + i) mod 2^64 of its
// side, from the index in 64-bit integers as in iq_pair_mix_kernel: the same bits as the decoded traces through
// iq_pair_mix_kernel, however the frames are cut.
// Shared oscillator: where both sides of a pair have the same ftw AND the same phase0 (decided per pair from the job table, so
// wave-uniform), zoom_lo is evaluated once a sample and its (c, s) turns both sides through iq_rotate, as in iq_pair_mix_kernel:
// the bits are those of two iq_mix calls.
// AdcDac: one thread per (frame, batch), 8 samples a trace; a cell is two 8-byte loads when base and frame size are 8-byte aligned,
// bytes otherwise; a pair takes the 8 samples as two 16-byte stores to each of its four streams when its position in the streams
// is 16-byte aligned (the four share their 16-byte phase), dword stores otherwise.  Fls / ThermostatEem / Mpll: one thread per four
// consecutive batches, one 16-byte store to each stream; the last partial run is stored sample by sample.
// The job table is indexed by the wave-uniform pair counter alone and the per-trace sample arrays by compile-time trace alone (an
// entry's trace is picked with an unrolled chain of wave-uniform selects), so nothing is indexed dynamically: no scratch.
#include "iq_cross.h"
#include "frames.h"
#include "iq_lo.h"

namespace psdk {

namespace {

constexpr int QXF_THREADS = 256;
constexpr int QXF_MAX_BLOCKS = 4096;
constexpr int QXF_RUN = 4; // batches a thread of the one-sample formats

template <int FMT, int T, class Word>
__device__ __forceinline__ void qxf_decode_trace(const Word &word, unsigned used, float &out)
{
    if constexpr (T < wire_fmt_v(FMT).ntraces)
        if ((used >> T) & 1u)
            out = payload_trace<FMT, T>(word);
}

// x = v[t] for a wave-uniform t < NT, without a dynamic index
template <int CNT, int NT>
__device__ __forceinline__ void qxf_pick(const float (&v)[4][CNT], int t, float (&x)[CNT])
{
#pragma unroll
    for (int i = 0; i < CNT; ++i) {
        x[i] = v[0][i];
#pragma unroll
        for (int tt = 1; tt < NT; ++tt)
            if (t == tt)
                x[i] = v[tt][i];
    }
}

// CNT consecutive values of one stream, stored at d
template <int CNT>
__device__ __forceinline__ void qxf_store(float *d, const float (&v)[CNT], bool vec, unsigned valid)
{
    if (vec) {
#pragma unroll
        for (int i = 0; i < CNT; i += 4)
            *reinterpret_cast<float4 *>(d + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < CNT; ++i)
            if ((unsigned)i < valid)
                d[i] = v[i];
    }
}

// CNT consecutive samples of both sides of pair p, the first at stream index j0 + i0: turned and stored at position i0 of the
// pair's four streams
template <int CNT, int NT>
__device__ __forceinline__ void qxf_mix_store(const IqCrossFramesBatch &b, int p, const float (&v)[4][CNT], size_t i0, bool al16,
                                              unsigned valid)
{
    float xia[CNT], xqa[CNT], xib[CNT], xqb[CNT];
    qxf_pick<CNT, NT>(v, b.trace[p][0], xia);
    qxf_pick<CNT, NT>(v, b.trace[p][1], xqa);
    qxf_pick<CNT, NT>(v, b.trace[p][2], xib);
    qxf_pick<CNT, NT>(v, b.trace[p][3], xqb);
    const unsigned long long j = b.j0[p] + i0;
    const unsigned long long fa = b.ftw[p][0], fb = b.ftw[p][1];
    unsigned long long pa = b.phase0[p][0] + fa * j, pb = b.phase0[p][1] + fb * j;
    float ia[CNT], qa[CNT], ib[CNT], qb[CNT];
    if (fa == fb && b.phase0[p][0] == b.phase0[p][1]) { // one carrier on both sides: one oscillator a sample
#pragma unroll
        for (int i = 0; i < CNT; ++i, pa += fa) {
            float c, s;
            zoom_lo(pa, c, s);
            iq_rotate(xia[i], xqa[i], c, s, ia[i], qa[i]);
            iq_rotate(xib[i], xqb[i], c, s, ib[i], qb[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CNT; ++i, pa += fa, pb += fb) {
            iq_mix(xia[i], xqa[i], pa, ia[i], qa[i]);
            iq_mix(xib[i], xqb[i], pb, ib[i], qb[i]);
        }
    }
    const bool vec = al16 && valid == CNT;
    qxf_store<CNT>(b.dst[p][0] + i0, ia, vec, valid);
    qxf_store<CNT>(b.dst[p][1] + i0, qa, vec, valid);
    qxf_store<CNT>(b.dst[p][2] + i0, ib, vec, valid);
    qxf_store<CNT>(b.dst[p][3] + i0, qb, vec, valid);
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(QXF_THREADS) void iq_cross_frames_kernel(const IqCrossFramesBatch b)
{
    constexpr int NT = wire_fmt_v(FMT).ntraces;
    const unsigned batches = (unsigned)b.batches;
    const unsigned total = b.n_frames * batches; // batches in the launch (< 2^23: the host cuts pieces of <= 2^22 samples a trace)
    unsigned used = 0, al16 = 0;                 // traces in use, pairs at a 16-byte aligned stream position (wave-uniform)
    for (int p = 0; p < b.npairs; ++p) {
        used |= (1u << b.trace[p][0]) | (1u << b.trace[p][1]) | (1u << b.trace[p][2]) | (1u << b.trace[p][3]);
        al16 |= ((reinterpret_cast<uintptr_t>(b.dst[p][0]) & 15u) == 0 ? 1u : 0u) << p;
    }
    if constexpr (FMT == 1) {
        const bool al8 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 7u) == 0;
        for (unsigned g = blockIdx.x * QXF_THREADS + threadIdx.x; g < total; g += gridDim.x * QXF_THREADS) {
            const unsigned f = g / batches, bb = g - f * batches;
            const uint8_t *p0 = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * 64;
            float v[4][8] = {};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (!((used >> t) & 1u))
                    continue;
                const uint8_t *q = p0 + t * 16;
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
            for (int p = 0; p < b.npairs; ++p)
                qxf_mix_store<8, NT>(b, p, v, (size_t)g * 8, (al16 >> p) & 1u, 8);
        }
    } else {
        constexpr int BB = wire_fmt_v(FMT).batch_bytes;
        const bool al4 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 3u) == 0;
        const unsigned runs = (total + QXF_RUN - 1) / QXF_RUN;
        for (unsigned r = blockIdx.x * QXF_THREADS + threadIdx.x; r < runs; r += gridDim.x * QXF_THREADS) {
            const unsigned g0 = r * QXF_RUN;
            unsigned f = g0 / batches, bb = g0 - f * batches;
            float v[4][QXF_RUN] = {};
#pragma unroll
            for (int c = 0; c < QXF_RUN; ++c) {
                if (g0 + c < total) {
                    const uint8_t *q = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * BB;
                    auto word = [&](int i) { return payload_word(q, i, al4); };
                    qxf_decode_trace<FMT, 0>(word, used, v[0][c]);
                    qxf_decode_trace<FMT, 1>(word, used, v[1][c]);
                    qxf_decode_trace<FMT, 2>(word, used, v[2][c]);
                    qxf_decode_trace<FMT, 3>(word, used, v[3][c]);
                }
                if (++bb == batches)
                    bb = 0, ++f;
            }
            const unsigned valid = total - g0 < (unsigned)QXF_RUN ? total - g0 : (unsigned)QXF_RUN;
            for (int p = 0; p < b.npairs; ++p)
                qxf_mix_store<QXF_RUN, NT>(b, p, v, (size_t)g0, (al16 >> p) & 1u, valid);
        }
    }
}

hipError_t launch_iq_cross_frames(const IqCrossFramesBatch &b, hipStream_t s)
{
    if (b.npairs < 1 || b.npairs > IQ_CROSS_FRAMES_MAX_PAIRS || b.batches < 1 || b.fmt < 1 || b.fmt > 4)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)b.n_frames * (unsigned)b.batches;
    if (total == 0)
        return hipSuccess;
    if (total >= (1ull << 31))
        return hipErrorInvalidValue;
    for (int p = 0; p < b.npairs; ++p)
        for (int c = 0; c < 4; ++c) {
            if (!b.dst[p][c] || ((uintptr_t)b.dst[p][c] & 3) || (((uintptr_t)b.dst[p][0] ^ (uintptr_t)b.dst[p][c]) & 15))
                return hipErrorInvalidValue;
            if (b.trace[p][c] < 0 || b.trace[p][c] >= wire_fmt_v(b.fmt).ntraces)
                return hipErrorInvalidValue;
        }
    const unsigned long long items = b.fmt == 1 ? total : (total + QXF_RUN - 1) / QXF_RUN;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(QXF_MAX_BLOCKS, (items + QXF_THREADS - 1) / QXF_THREADS);
    if (b.fmt == 1)
        hipLaunchKernelGGL(iq_cross_frames_kernel<1>, dim3(blocks), dim3(QXF_THREADS), 0, s, b);
    else if (b.fmt == 2)
        hipLaunchKernelGGL(iq_cross_frames_kernel<2>, dim3(blocks), dim3(QXF_THREADS), 0, s, b);
    else if (b.fmt == 3)
        hipLaunchKernelGGL(iq_cross_frames_kernel<3>, dim3(blocks), dim3(QXF_THREADS), 0, s, b);
    else
        hipLaunchKernelGGL(iq_cross_frames_kernel<4>, dim3(blocks), dim3(QXF_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
