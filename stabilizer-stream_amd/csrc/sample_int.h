// sample_int.h -- the integer sample feeds of the four mixer-fronted objects (psdc_int_*, sample_int.hip): int16 / int8 samples
// read where the f32 mixers (zoom.hip, iq.hip, iq_cross.hip) read floats, converted in registers and mixed by the same formulas;
// and of the three real-input objects (psdc_sint_*: PSD, pair, matrix): the same conversion with no mixer behind it (sint_cvt_thread).
// Usable from host and device like iq_lo.h: tests/host/sample_int_emul.cpp runs everything below on the host.
//
// Conversion: the f32 sample the mixer sees is (float)v * scale -- the int-to-float conversion is exact (|v| <= 2^15), and the
// product is ONE stand-alone f32 product rounded to nearest (__fmul_rn on the device; on the host a plain product, which no
// compiler may fuse into anything because the mix formulas of zoom_lo.h and iq_lo.h take it as a finished operand of a
// stand-alone product or of an explicit fmaf).  So an integer launch stores the bits the f32 mixer stores for the converted stream.
//
// Unit: one integer (real objects) or one interleaved (re, im) pair of integers (complex objects: sc16 is 4 bytes, sc8 is 2).
//
// Access scheme: that of the f32 mixers.  A thread takes SINT_Q = 4 consecutive units that start on a 16-byte boundary of the
// destination streams and does one 16-byte store to each stream; thread 0 takes the `head` (0 ... 3) units in front of the first
// boundary; the thread of the last group takes the partial one.  sint_span() is that map.  A full group whose source address is
// aligned to the group's byte size is read with ONE load (16 bytes for four sc16 units, 8 for four s16 or four sc8 units, 4 for
// four s8 units: sint_load_group); every other unit is read element-wise at the unit's own size.  A wide load is made only for
// a FULL group, so no byte outside [src, src + len * unit) is read.
// Four units a thread, not 8 or 16: the mixers are bound by their stores (a real s8 unit is 1 byte in and 8 bytes out, an sc16
// unit 4 in and 8 out), the 16-byte stores of four units already fill a wave's store path, and the f32 mixers' grid, head and
// tail rules carry over unchanged, which keeps one index map for the f32 and the integer mixers.
#pragma once
#include "iq_lo.h"

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace psdk {

constexpr int SAMPLE_F32 = 0, SAMPLE_S16 = 1, SAMPLE_S8 = 2; // S16, S8: PSDC_SAMPLE_S16, PSDC_SAMPLE_S8 of psdcascade.h
constexpr int SINT_Q = 4, SINT_BLOCK = 256;

// bytes of one integer of a kind (0: not an integer kind)
ZOOM_HD int sint_bytes(int kind) { return kind == SAMPLE_S16 ? 2 : kind == SAMPLE_S8 ? 1 : 0; }

// ---- the index map -------------------------------------------------------------------------------------------------------
// the units thread g of a launch reads and writes: [first, first + count), count <= SINT_Q.  wide: the group is full and the
// launch's source is aligned, so its count * unit bytes at byte offset first * unit come with one load; else count loads of one
// unit each.  Threads past the last group get count = 0.
struct SintSpan {
    unsigned long long first;
    unsigned count;
    bool wide;
};

ZOOM_HD SintSpan sint_span(unsigned long long g, unsigned head, unsigned long long len, bool src_aligned)
{
    if (g == 0)
        return SintSpan{0, head, false};
    const unsigned long long i0 = head + (g - 1) * SINT_Q;
    if (i0 >= len)
        return SintSpan{len, 0, false};
    const unsigned long long rem = len - i0;
    if (rem >= SINT_Q)
        return SintSpan{i0, (unsigned)SINT_Q, src_aligned};
    return SintSpan{i0, (unsigned)rem, false};
}

// units in front of the first 16-byte boundary of a destination stream of floats (at most len)
inline unsigned sint_head(const float *dst, unsigned long long len)
{
    const unsigned long long lead = (4 - (((uintptr_t)dst >> 2) & 3)) & 3;
    return (unsigned)(lead < len ? lead : len);
}

// threads a launch needs: thread 0 and one a group
inline unsigned long long sint_threads(unsigned head, unsigned long long len) { return 1 + (len - head + SINT_Q - 1) / SINT_Q; }

// the first group's source address is aligned to a group's bytes (then every group's is)
inline bool sint_src_aligned(const void *src, unsigned head, size_t unit_bytes)
{
    return ((uintptr_t)src + (size_t)head * unit_bytes) % (SINT_Q * unit_bytes) == 0;
}

// ---- unpack and scale ----------------------------------------------------------------------------------------------------
ZOOM_HD float sint_scale(int v, float scale)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn((float)v, scale);
#else
    return (float)v * scale;
#endif
}

// integer `lane` of a packed little-endian 32-bit word (T = int16_t: lanes 0, 1; int8_t: lanes 0 ... 3), sign-extended, scaled
template <typename T>
ZOOM_HD float sint_lane(uint32_t w, int lane, float scale)
{
    constexpr int B = 8 * (int)sizeof(T);
    const int32_t top = (int32_t)(w << (32 - B * (lane + 1))); // the lane's bits at the top of the word
    return sint_scale((int)(top >> (32 - B)), scale);          // the arithmetic shift extends the sign
}

// the packed words of one full group: SINT_Q units of C integers of type T (C = 1 real, 2 complex)
template <typename T, int C>
struct SintGroup {
    static constexpr int BYTES = SINT_Q * C * (int)sizeof(T), WORDS = BYTES / 4, LANES = 4 / (int)sizeof(T);
    uint32_t w[WORDS];
    // component c of unit u of the group, converted
    ZOOM_HD float get(int u, int c, float scale) const
    {
        const int e = u * C + c;
        return sint_lane<T>(w[e / LANES], e % LANES, scale);
    }
};

// one load of a group's bytes; p is aligned to SintGroup<T, C>::BYTES
template <typename T, int C>
ZOOM_HD void sint_load_group(const T *p, SintGroup<T, C> &g)
{
    __builtin_memcpy(g.w, __builtin_assume_aligned(p, SintGroup<T, C>::BYTES), SintGroup<T, C>::BYTES);
}

// one integer read at its own size
template <typename T>
ZOOM_HD float sint_load1(const T *p, float scale)
{
    return sint_scale((int)*p, scale);
}

// one (re, im) unit read at its own size (4 bytes for sc16, 2 for sc8); p is aligned to it
template <typename T>
ZOOM_HD void sint_load1c(const T *p, float scale, float &re, float &im)
{
    typename std::conditional<sizeof(T) == 2, uint32_t, uint16_t>::type w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, sizeof(w)), sizeof(w));
    re = sint_lane<T>((uint32_t)w, 0, scale);
    im = sint_lane<T>((uint32_t)w, 1, scale);
}

// ---- the mixers, one thread each -----------------------------------------------------------------------------------------
// One call's units of one stream: ZoomMixJob (real) or IqMixJob's interleaved case (complex) with integers at src.  Unit i
// (i < len) is stream sample j0 + i and has the phase phase0 + ftw (j0 + i) mod 2^64; dst_i and dst_q are equally aligned.
struct SintMixJob {
    const void *src;
    float *dst_i;
    float *dst_q;
    unsigned long long len;
    unsigned long long j0;
    unsigned long long ftw;
    unsigned long long phase0;
    float scale;
};

// Both sides of a pair: IqPairMixJob's interleaved case with integer pairs at src[0] (side a) and src[1] (side b); side s goes
// to dst[2 s] (I') and dst[2 s + 1] (Q').  The four destinations are equally aligned.
struct SintPairMixJob {
    const void *src[2];
    float *dst[4];
    unsigned long long len;
    unsigned long long j0;
    unsigned long long ftw[2];
    unsigned long long phase0[2];
    float scale;
};

struct SintF4 { // a thread's four outputs of one stream, stored with one 16-byte store
    float v[SINT_Q];
};

ZOOM_HD void sint_store4(float *dst, const SintF4 &f) { __builtin_memcpy(__builtin_assume_aligned(dst, 16), f.v, 16); }

// thread g of zoom_mix_kernel on integers
template <typename T>
ZOOM_HD void sint_zoom_thread(const SintMixJob &job, unsigned head, bool src_aligned, unsigned long long g)
{
    const SintSpan sp = sint_span(g, head, job.len, src_aligned);
    if (sp.count == 0)
        return;
    const T *src = static_cast<const T *>(job.src);
    unsigned long long ph = job.phase0 + job.ftw * (job.j0 + sp.first);
    if (sp.count == SINT_Q) { // a full group (thread 0's head is at most three units)
        float x[SINT_Q];
        if (sp.wide) {
            SintGroup<T, 1> grp;
            sint_load_group<T, 1>(src + sp.first, grp);
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u)
                x[u] = grp.get(u, 0, job.scale);
        } else {
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u)
                x[u] = sint_load1(src + sp.first + u, job.scale);
        }
        SintF4 vi, vq;
#pragma unroll
        for (int u = 0; u < SINT_Q; ++u, ph += job.ftw)
            zoom_mix(x[u], ph, vi.v[u], vq.v[u]);
        sint_store4(job.dst_i + sp.first, vi);
        sint_store4(job.dst_q + sp.first, vq);
        return;
    }
    for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i, ph += job.ftw)
        zoom_mix(sint_load1(src + i, job.scale), ph, job.dst_i[i], job.dst_q[i]);
}

// the four complex units of a full group of one side: re to a[], im to b[]
template <typename T>
ZOOM_HD void sint_load4c(const T *pairs, unsigned long long first, bool wide, float scale, float (&a)[SINT_Q], float (&b)[SINT_Q])
{
    const T *p = pairs + 2 * first;
    if (wide) {
        SintGroup<T, 2> grp;
        sint_load_group<T, 2>(p, grp);
#pragma unroll
        for (int u = 0; u < SINT_Q; ++u)
            a[u] = grp.get(u, 0, scale), b[u] = grp.get(u, 1, scale);
    } else {
#pragma unroll
        for (int u = 0; u < SINT_Q; ++u)
            sint_load1c(p + 2 * u, scale, a[u], b[u]);
    }
}

// thread g of iq_mix_kernel<true> on integer pairs
template <typename T>
ZOOM_HD void sint_iq_thread(const SintMixJob &job, unsigned head, bool src_aligned, unsigned long long g)
{
    const SintSpan sp = sint_span(g, head, job.len, src_aligned);
    if (sp.count == 0)
        return;
    const T *src = static_cast<const T *>(job.src);
    unsigned long long ph = job.phase0 + job.ftw * (job.j0 + sp.first);
    if (sp.count == SINT_Q) { // a full group (thread 0's head is at most three units)
        float a[SINT_Q], b[SINT_Q];
        sint_load4c<T>(src, sp.first, sp.wide, job.scale, a, b);
        SintF4 vi, vq;
#pragma unroll
        for (int u = 0; u < SINT_Q; ++u, ph += job.ftw)
            iq_mix(a[u], b[u], ph, vi.v[u], vq.v[u]);
        sint_store4(job.dst_i + sp.first, vi);
        sint_store4(job.dst_q + sp.first, vq);
        return;
    }
    for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i, ph += job.ftw) {
        float a, b;
        sint_load1c(src + 2 * i, job.scale, a, b);
        iq_mix(a, b, ph, job.dst_i[i], job.dst_q[i]);
    }
}

// thread g of iq_pair_mix_kernel<true> on integer pairs.  src_aligned: bit 0 -- side a's pairs are aligned at the first group,
// bit 1 -- side b's.  The shared oscillator is that kernel's: one zoom_lo a sample where both sides have the same ftw AND phase0.
template <typename T>
ZOOM_HD void sint_iq_pair_thread(const SintPairMixJob &job, unsigned head, int src_aligned, unsigned long long g)
{
    const SintSpan sp = sint_span(g, head, job.len, true);
    if (sp.count == 0)
        return;
    const bool shared = job.ftw[0] == job.ftw[1] && job.phase0[0] == job.phase0[1]; // wave-uniform
    const T *sa = static_cast<const T *>(job.src[0]), *sb = static_cast<const T *>(job.src[1]);
    unsigned long long pa = job.phase0[0] + job.ftw[0] * (job.j0 + sp.first), pb = job.phase0[1] + job.ftw[1] * (job.j0 + sp.first);
    if (sp.count == SINT_Q) { // a full group (thread 0's head is at most three units)
        float ai[SINT_Q], aq[SINT_Q], bi[SINT_Q], bq[SINT_Q];
        sint_load4c<T>(sa, sp.first, sp.wide && (src_aligned & 1), job.scale, ai, aq);
        sint_load4c<T>(sb, sp.first, sp.wide && (src_aligned & 2), job.scale, bi, bq);
        SintF4 via, vqa, vib, vqb;
        if (shared) {
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u, pa += job.ftw[0]) {
                float c, s;
                zoom_lo(pa, c, s);
                iq_rotate(ai[u], aq[u], c, s, via.v[u], vqa.v[u]);
                iq_rotate(bi[u], bq[u], c, s, vib.v[u], vqb.v[u]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u, pa += job.ftw[0], pb += job.ftw[1]) {
                iq_mix(ai[u], aq[u], pa, via.v[u], vqa.v[u]);
                iq_mix(bi[u], bq[u], pb, vib.v[u], vqb.v[u]);
            }
        }
        sint_store4(job.dst[0] + sp.first, via);
        sint_store4(job.dst[1] + sp.first, vqa);
        sint_store4(job.dst[2] + sp.first, vib);
        sint_store4(job.dst[3] + sp.first, vqb);
        return;
    }
    for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i, pa += job.ftw[0], pb += job.ftw[1]) {
        float ia, qa, ib, qb;
        sint_load1c(sa + 2 * i, job.scale, ia, qa);
        sint_load1c(sb + 2 * i, job.scale, ib, qb);
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

// ---- the converter, one thread ---------------------------------------------------------------------------------------------
// The feeds of the objects with no mixer in front of stage 0 (psdc_sint_*: PSD, pair, matrix): nch (1 ... 4) equally long
// channels of integers, each written as f32 where the f32 call's copy writes, dst[c][i] = sint_scale(src[c][i], scale).  The
// mixers' access scheme without the oscillator; the destinations of a launch share their 16-byte phase.
struct SintCvtJob {
    const void *src[4];
    float *dst[4];
    unsigned nch;
    unsigned long long len;
    float scale;
};

// thread g of channel ch of sample_cvt_int_kernel.  src_aligned_mask: bit c -- channel c's source is aligned at the first group
template <typename T>
ZOOM_HD void sint_cvt_thread(const SintCvtJob &job, unsigned head, int src_aligned_mask, unsigned ch, unsigned long long g)
{
    if (ch >= job.nch)
        return;
    const SintSpan sp = sint_span(g, head, job.len, (src_aligned_mask >> ch) & 1);
    if (sp.count == 0)
        return;
    const T *src = static_cast<const T *>(job.src[ch]);
    float *dst = job.dst[ch];
    if (sp.count == SINT_Q) { // a full group (thread 0's head is at most three units)
        SintF4 v;
        if (sp.wide) {
            SintGroup<T, 1> grp;
            sint_load_group<T, 1>(src + sp.first, grp);
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u)
                v.v[u] = grp.get(u, 0, job.scale);
        } else {
#pragma unroll
            for (int u = 0; u < SINT_Q; ++u)
                v.v[u] = sint_load1(src + sp.first + u, job.scale);
        }
        sint_store4(dst + sp.first, v);
        return;
    }
    for (unsigned long long i = sp.first; i < sp.first + sp.count; ++i)
        dst[i] = sint_load1(src + i, job.scale);
}

#if defined(__HIPCC__)
// the launches (sample_int.hip); kind: SAMPLE_S16 or SAMPLE_S8.  hipErrorInvalidValue for another kind, a null or misaligned
// pointer, or destinations that do not share their 16-byte phase.
hipError_t launch_zoom_mix_int(const SintMixJob &j, int kind, hipStream_t s);
hipError_t launch_iq_mix_int(const SintMixJob &j, int kind, hipStream_t s);
hipError_t launch_iq_pair_mix_int(const SintPairMixJob &j, int kind, hipStream_t s);
hipError_t launch_cvt_int(const SintCvtJob &j, int kind, hipStream_t s); // also for nch outside 1 ... 4
#endif

} // namespace psdk
