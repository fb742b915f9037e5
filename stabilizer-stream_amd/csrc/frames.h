// frames.h -- device side of the frame sources: where a sample of an AdcDac trace sits in a run of frames (kernels.h FrameSpan)
// and how the wire words of every payload format become f32 (src/de/frame.rs:5-9 header of 8 bytes, src/de/data.rs payloads).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wire_format.h"

namespace psdk {

// byte offset, within the span, of (batch, channel 0) cell `cell` (cell < 2^24)
__device__ __forceinline__ unsigned frame_cell_offset(const FrameSpan &fs, unsigned cell)
{
    const unsigned f = fs.batches == 1 ? cell : __umulhi(cell, fs.magic); // cell / batches
    // (24-bit multiplies -- full rate, where v_mul_lo_u32 is quarter rate: f < 2^24, batches < 2^8, frame_size < 2^24,
    // products below 2^32)
    const unsigned b = cell - __umul24(f, fs.batches);
    return __umul24(f, fs.frame_size) + 8u + b * 64u;
}

__device__ __forceinline__ float adcdac_lsb() { return 4.096f * 2.5f / 32768.0f; } // src/de/data.rs:28-35 (one constant, asserted equal)

// wire word -> volts: i16::from_le_bytes (ADC) / .wrapping_add(i16::MIN) (DAC: flips the sign bit) as f32 * LSB
__device__ __forceinline__ float adcdac_volts(unsigned word16, bool dac)
{
    if (dac)
        word16 ^= 0x8000u;
    return (float)(short)(unsigned short)word16 * adcdac_lsb();
}

// one sample of trace ch (generic kernels, seams, tails: off the hot path)
__device__ __forceinline__ float frame_sample(const FrameSpan &fs, int ch, unsigned long long i)
{
    const unsigned off = frame_cell_offset(fs, (unsigned)(i >> 3)) + (unsigned)ch * 16u + ((unsigned)i & 7u) * 2u;
    const unsigned short w = *reinterpret_cast<const unsigned short *>(fs.frames + off);
    return adcdac_volts(w, ch >= 2);
}

// four consecutive samples (i a multiple of 4) as one 8-byte load, converted
__device__ __forceinline__ float4 frame_sample4(const FrameSpan &fs, int ch, unsigned long long i)
{
    const unsigned off = frame_cell_offset(fs, (unsigned)(i >> 3)) + (unsigned)ch * 16u + ((unsigned)i & 4u) * 2u;
    const uint2 r = *reinterpret_cast<const uint2 *>(fs.frames + off);
    const bool dac = ch >= 2;
    return make_float4(adcdac_volts(r.x & 0xffffu, dac), adcdac_volts(r.x >> 16, dac), adcdac_volts(r.y & 0xffffu, dac),
                       adcdac_volts(r.y >> 16, dac));
}

// The other payload formats (src/de/data.rs:84-212) -- Fls (format id 2), ThermostatEem (3), Mpll (4): ONE sample per batch and
// trace.  The arithmetic is the reference's, operation by operation in f32 (`as f32` conversions, separate products and sum --
// rustc never fuses them --, a correctly rounded square root, the scale constants evaluated in f32 in the reference's order): the
// traces are bit-identical to Payload::traces.  (payload_kernel in kernels.hip, cross_frames_kernel in cross_frames.hip; bytes per batch and traces: wire_format.h.)

// u32::from_le_bytes of word i of the batch at p: one load when the frames are 4-byte aligned (every valid frame_size is a multiple
// of 8; the base is the caller's), bytes otherwise
__device__ __forceinline__ uint32_t payload_word(const uint8_t *p, int i, bool aligned)
{
    const uint8_t *q = p + 4 * i;
    if (aligned)
        return *reinterpret_cast<const uint32_t *>(q);
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}

// a.powi(2) + c.powi(2), .sqrt(): two products, one sum, a correctly rounded root.  (HIP's __fmul_rn / __fadd_rn are plain
// operators the backend may fuse, and __fsqrt_rn is the approximate native root: the pragma and sqrtf -- IEEE under hipcc's
// default -fhip-fp32-correctly-rounded-divide-sqrt -- are what pins the arithmetic.)
__device__ __forceinline__ float payload_hyp(float a, float c)
{
#pragma clang fp contract(off)
    const float aa = a * a, cc = c * c;
    const float sum = aa + cc;
    return sqrtf(sum);
}

// trace T of one batch of format FMT; word(i) = u32::from_le_bytes of the batch's word i
template <int FMT, int T, class Word>
__device__ __forceinline__ float payload_trace(const Word &word)
{
    auto i32f = [&](int i) { return (float)(int32_t)word(i); }; // i32::from_le_bytes(..) as f32
    if constexpr (FMT == 2) { // Fls::traces, data.rs:97-139
        constexpr float inv_max = 1.0f / 2147483648.0f;          // 1.0 / (i32::MAX as f32)
        constexpr float ap = 6.28318530717958647692f / 65536.0f; // TAU / (1i64 << 16) as f32
        if constexpr (T == 0)
            return payload_hyp(i32f(0), i32f(1)) * inv_max; // "AR" :100-110
        if constexpr (T == 1) {
            const long long ph = (long long)((unsigned long long)word(2) | ((unsigned long long)word(3) << 32));
            return (float)ph * ap; // "AP" :111-123
        }
        if constexpr (T == 2)
            return i32f(7) / 2147483648.0f; // "BI" b[1][0] :124-130 (a power of two: exact)
        return i32f(8) / 2147483648.0f;     // "BQ" b[1][1] :131-137
    } else if constexpr (FMT == 3) { // ThermostatEem::traces, data.rs:154-163: words 0, 8, 13, 16 as f32
        return __uint_as_float(word(T == 0 ? 0 : T == 1 ? 8 : T == 2 ? 13 : 16));
    } else { // Mpll::traces, data.rs:178-211
        static_assert(FMT == 4 && T < 3, "Mpll carries three traces");
        constexpr float two32 = 4294967296.0f;
        constexpr float c_phase = 6.28318530717958647692f / two32;    // TAU / (1u64 << 32) as f32
        constexpr float c_freq = 1.0f / 1.28e-3f / two32;             // 1.0 / 1.28e-3 / (1u64 << 32) as f32
        constexpr float c_amp = 10.24f / 10.0f * 2.0f * 2.0f / two32; // 10.24 / 10.0 * 2.0 * 2.0 / (1u64 << 32) as f32
        if constexpr (T == 0)
            return i32f(4) * c_phase; // "phase (rad)"
        if constexpr (T == 1)
            return i32f(5) * c_freq; // "frequency (kHz)"
        return payload_hyp(i32f(0), i32f(1)) * c_amp; // "amplitude (V/G10)"
    }
}

} // namespace psdk
