// zoom_cross_frames.hip -- gfx950 kernel that decodes stream frames and mixes them straight into the four stage-0 streams (I_a, Q_a,
// I_b, Q_b) of zoom cross pairs (psdc_zoomcsdcascade_process_frames[_device], cross_runtime.cpp).
//
//   zoom_cross_frames_kernel<FMT>  the work decomposition and the arithmetic of zoom_frames_kernel<FMT>, pair-shaped: each (frame,
//                                  batch, trace) cell of the traces in use is read and converted ONCE a thread (frames.h:
//                                  adcdac_volts, payload_trace -- the bits of Payload::traces) and then handed to every side of
//                                  every pair that takes it; a side's samples are mixed in registers with the side's carrier and
//                                  stored to its I and Q streams.  The f32 trace never exists in memory.
// Sample i of the launch is stream sample j0 + i of both sides of a pair and has the phase phase0 + ftw (j0 + i) mod 2^64 of its
// side, from the index in 64-bit integers as in zoom_mix_kernel and zoom_frames_kernel: the same bits as the decoded traces through
// two zoom_mix_kernel launches, however the frames are cut.
// Shared oscillator: where both sides of a pair have the same ftw AND the same phase0 (two receivers on one carrier; decided per
// pair from the job table, so wave-uniform), zoom_lo is evaluated once a sample and its (c, s) mixes both traces.  I = x c and
// Q = -(x s) are formed separately from (c, s) exactly as zoom_mix forms them, so the bits are those of two zoom_mix calls.  Equal
// ftw with different phase0 is two oscillators, and so is the +-ftw recipe (the top 32 bits of -phi are not the negation of the
// top 32 bits of phi).
// AdcDac: one thread per (frame, batch), 8 samples a trace; a cell is two 8-byte loads when base and frame size are 8-byte aligned,
// bytes otherwise; a pair takes the 8 samples as two 16-byte stores to each of its four streams when its position in the streams
// is 16-byte aligned (the four share their 16-byte phase), dword stores otherwise.  Fls / ThermostatEem / Mpll: one thread per four
// consecutive batches, one 16-byte store to each stream; the last partial run is stored sample by sample.
// The job table is indexed by the wave-uniform pair counter alone and the per-trace sample arrays by compile-time trace alone (a
// side's trace is picked with an unrolled chain of wave-uniform selects), so nothing is indexed dynamically: no scratch.
#include "zoom_cross.h"
#include "frames.h"
#include "zoom_lo.h"

namespace psdk {

namespace {

constexpr int ZXF_THREADS = 256;
constexpr int ZXF_MAX_BLOCKS = 4096;
constexpr int ZXF_RUN = 4; // batches a thread of the one-sample formats

template <int FMT, int T, class Word>
__device__ __forceinline__ void zxf_decode_trace(const Word &word, unsigned used, float &out)
{
    if constexpr (T < wire_fmt_v(FMT).ntraces)
        if ((used >> T) & 1u)
            out = payload_trace<FMT, T>(word);
}

// x = v[t] for a wave-uniform t < NT, without a dynamic index
template <int CNT, int NT>
__device__ __forceinline__ void zxf_pick(const float (&v)[4][CNT], int t, float (&x)[CNT])
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
__device__ __forceinline__ void zxf_store(float *d, const float (&v)[CNT], bool vec, unsigned valid)
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

// CNT consecutive samples of both sides of pair p, the first at stream index j0 + i0: mixed and stored at position i0 of the
// pair's four streams
template <int CNT, int NT>
__device__ __forceinline__ void zxf_mix_store(const ZoomCrossFramesBatch &b, int p, const float (&v)[4][CNT], size_t i0, bool al16,
                                              unsigned valid)
{
    float xa[CNT], xb[CNT];
    zxf_pick<CNT, NT>(v, b.trace[p][0], xa);
    zxf_pick<CNT, NT>(v, b.trace[p][1], xb);
    const unsigned long long j = b.j0[p] + i0;
    const unsigned long long fa = b.ftw[p][0], fb = b.ftw[p][1];
    unsigned long long pa = b.phase0[p][0] + fa * j, pb = b.phase0[p][1] + fb * j;
    float ia[CNT], qa[CNT], ib[CNT], qb[CNT];
    if (fa == fb && b.phase0[p][0] == b.phase0[p][1]) { // one carrier on both sides: one oscillator a sample
#pragma unroll
        for (int i = 0; i < CNT; ++i, pa += fa) {
            float c, s;
            zoom_lo(pa, c, s);
            ia[i] = xa[i] * c;
            qa[i] = -(xa[i] * s);
            ib[i] = xb[i] * c;
            qb[i] = -(xb[i] * s);
        }
    } else {
#pragma unroll
        for (int i = 0; i < CNT; ++i, pa += fa, pb += fb) {
            zoom_mix(xa[i], pa, ia[i], qa[i]);
            zoom_mix(xb[i], pb, ib[i], qb[i]);
        }
    }
    const bool vec = al16 && valid == CNT;
    zxf_store<CNT>(b.dst[p][0] + i0, ia, vec, valid);
    zxf_store<CNT>(b.dst[p][1] + i0, qa, vec, valid);
    zxf_store<CNT>(b.dst[p][2] + i0, ib, vec, valid);
    zxf_store<CNT>(b.dst[p][3] + i0, qb, vec, valid);
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(ZXF_THREADS) void zoom_cross_frames_kernel(const ZoomCrossFramesBatch b)
{
    constexpr int NT = wire_fmt_v(FMT).ntraces;
    const unsigned batches = (unsigned)b.batches;
    const unsigned total = b.n_frames * batches; // batches in the launch (< 2^23: the host cuts pieces of <= 2^22 samples a trace)
    unsigned used = 0, al16 = 0;                 // traces in use, pairs at a 16-byte aligned stream position (wave-uniform)
    for (int p = 0; p < b.npairs; ++p) {
        used |= (1u << b.trace[p][0]) | (1u << b.trace[p][1]);
        al16 |= ((reinterpret_cast<uintptr_t>(b.dst[p][0]) & 15u) == 0 ? 1u : 0u) << p;
    }
    if constexpr (FMT == 1) {
        const bool al8 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 7u) == 0;
        for (unsigned g = blockIdx.x * ZXF_THREADS + threadIdx.x; g < total; g += gridDim.x * ZXF_THREADS) {
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
                zxf_mix_store<8, NT>(b, p, v, (size_t)g * 8, (al16 >> p) & 1u, 8);
        }
    } else {
        constexpr int BB = wire_fmt_v(FMT).batch_bytes;
        const bool al4 = ((reinterpret_cast<uintptr_t>(b.frames) | b.frame_size) & 3u) == 0;
        const unsigned runs = (total + ZXF_RUN - 1) / ZXF_RUN;
        for (unsigned r = blockIdx.x * ZXF_THREADS + threadIdx.x; r < runs; r += gridDim.x * ZXF_THREADS) {
            const unsigned g0 = r * ZXF_RUN;
            unsigned f = g0 / batches, bb = g0 - f * batches;
            float v[4][ZXF_RUN] = {};
#pragma unroll
            for (int c = 0; c < ZXF_RUN; ++c) {
                if (g0 + c < total) {
                    const uint8_t *q = b.frames + (size_t)f * b.frame_size + 8 + (size_t)bb * BB;
                    auto word = [&](int i) { return payload_word(q, i, al4); };
                    zxf_decode_trace<FMT, 0>(word, used, v[0][c]);
                    zxf_decode_trace<FMT, 1>(word, used, v[1][c]);
                    zxf_decode_trace<FMT, 2>(word, used, v[2][c]);
                    zxf_decode_trace<FMT, 3>(word, used, v[3][c]);
                }
                if (++bb == batches)
                    bb = 0, ++f;
            }
            const unsigned valid = total - g0 < (unsigned)ZXF_RUN ? total - g0 : (unsigned)ZXF_RUN;
            for (int p = 0; p < b.npairs; ++p)
                zxf_mix_store<ZXF_RUN, NT>(b, p, v, (size_t)g0, (al16 >> p) & 1u, valid);
        }
    }
}

hipError_t launch_zoom_cross_frames(const ZoomCrossFramesBatch &b, hipStream_t s)
{
    if (b.npairs < 1 || b.npairs > ZOOM_CROSS_FRAMES_MAX_PAIRS || b.batches < 1 || b.fmt < 1 || b.fmt > 4)
        return hipErrorInvalidValue;
    const unsigned long long total = (unsigned long long)b.n_frames * (unsigned)b.batches;
    if (total == 0)
        return hipSuccess;
    if (total >= (1ull << 31))
        return hipErrorInvalidValue;
    for (int p = 0; p < b.npairs; ++p) {
        for (int c = 0; c < 4; ++c)
            if (!b.dst[p][c] || ((uintptr_t)b.dst[p][c] & 3) || (((uintptr_t)b.dst[p][0] ^ (uintptr_t)b.dst[p][c]) & 15))
                return hipErrorInvalidValue;
        for (int side = 0; side < 2; ++side)
            if (b.trace[p][side] < 0 || b.trace[p][side] >= wire_fmt_v(b.fmt).ntraces)
                return hipErrorInvalidValue;
    }
    const unsigned long long items = b.fmt == 1 ? total : (total + ZXF_RUN - 1) / ZXF_RUN;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(ZXF_MAX_BLOCKS, (items + ZXF_THREADS - 1) / ZXF_THREADS);
    if (b.fmt == 1)
        hipLaunchKernelGGL(zoom_cross_frames_kernel<1>, dim3(blocks), dim3(ZXF_THREADS), 0, s, b);
    else if (b.fmt == 2)
        hipLaunchKernelGGL(zoom_cross_frames_kernel<2>, dim3(blocks), dim3(ZXF_THREADS), 0, s, b);
    else if (b.fmt == 3)
        hipLaunchKernelGGL(zoom_cross_frames_kernel<3>, dim3(blocks), dim3(ZXF_THREADS), 0, s, b);
    else
        hipLaunchKernelGGL(zoom_cross_frames_kernel<4>, dim3(blocks), dim3(ZXF_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
