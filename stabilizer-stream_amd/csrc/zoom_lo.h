// zoom_lo.h -- the local oscillator of the zoom cascade (psdc_zoom_*, zoom.hip): cos and sin of a 64-bit phase in f32.
//
// A phase is an unsigned 64-bit count of 2^-64 turns; its top 32 bits are used (the truncation is 2 pi 2^-32 rad).  The
// octant reduction is exact integer arithmetic: the top three bits name the octant, the 29 bits below are the distance r
// into it, and an odd octant is walked backwards (2^29 - r), so the polynomials see t = r / 2^29 in [0, 1], the angle
// pi/4 t.  r has up to 30 significant bits and f32 holds 24: t is carried as th + tl, both exact (the top 24 bits and the
// low 6), and tl enters through the first derivative: t^2 = th^2 + 2 th tl and sin = (th + tl) P(t^2).
//     sin(pi/4 t) = t (a1 + t^2 (s0 + t^2 (s1 + t^2 (s2 + t^2 s3)))),  a1 = pi/4 carried as a1h + a1l
//     cos(pi/4 t) = 1 + t^2 (c0 + t^2 (c1 + t^2 (c2 + t^2 c3)))
// (least-squares fits weighted for the absolute error of the result: 2^-29.5 and 2^-27.1 before rounding).  Every sum is an
// explicit fmaf and every product stands alone or feeds one, so no compiler may contract anything and the host and the device
// run the same operations.  What is checked: the values against f64 on the host (tests/host/zoom_emul.cpp), and the GPU's
// spectra within the parity bound of a restatement that mixes with this code on the host (tests/test_gpu_zoom.py); no test reads
// the device's I and Q back to compare bits.  No libm.  Quarter turns have r = 0 in an even octant: t = 0 gives sin = 0 and cos = 1 exactly, so the pair is
// exactly (+-1, 0) or (0, +-1).  Worst absolute error over the 3.1e6 phases of the host check: 2^-24.0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZOOM_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define ZOOM_HD inline
#endif

namespace psdk {

// (c, s) = (cos, sin)(2 pi phase / 2^64)
ZOOM_HD void zoom_lo(uint64_t phase, float &c, float &s)
{
    const uint32_t p = (uint32_t)(phase >> 32);
    const uint32_t oct = p >> 29;
    uint32_t r = p & 0x1FFFFFFFu;
    if (oct & 1u)
        r = 0x20000000u - r;
    const float th = (float)(int)(r & ~0x3Fu) * 0x1p-29f; // <= 24 significant bits: exact
    const float tl = (float)(int)(r & 0x3Fu) * 0x1p-29f;
    const float t2 = fmaf(th, th, (tl + tl) * th);
    float qs = fmaf(t2, 0x1.4b98c2p-22f, -0x1.32c9e4p-15f);
    qs = fmaf(t2, qs, 0x1.466bbap-9f);
    qs = fmaf(t2, qs, -0x1.4abbcep-4f);
    const float u = fmaf(t2, qs, -0x1.777a5cp-26f);      // P - a1h
    const float pf = fmaf(t2, qs, 0x1.921fb6p-1f);       // P
    const float sn = fmaf(th, 0x1.921fb6p-1f, fmaf(tl, pf, th * u));
    float qc = fmaf(t2, 0x1.d9f188p-19f, -0x1.55c64ap-12f);
    qc = fmaf(t2, qc, 0x1.03c1dep-6f);
    qc = fmaf(t2, qc, -0x1.3bd3ccp-2f);
    const float cs = fmaf(t2, qc, 1.0f);
    // the angle is q pi/2 + a (even octant) or q pi/2 - a (odd), q = (oct + 1) / 2 mod 4
    const uint32_t q = ((oct + 1u) >> 1) & 3u;
    const float sa = (oct & 1u) ? -sn : sn; // sin(+-a)
    const float cq = (q & 1u) ? sa : cs;    // q = 0: (c, sa); 1: (-sa, c); 2: (-c, -sa); 3: (sa, -c)
    const float sq = (q & 1u) ? cs : sa;
    c = (q == 1u || q == 2u) ? -cq : cq;
    s = (q >= 2u) ? -sq : sq;
}

// one sample through the mixer: z = x exp(-2 pi i phase / 2^64)
ZOOM_HD void zoom_mix(float x, uint64_t phase, float &i, float &q)
{
    float c, s;
    zoom_lo(phase, c, s);
    i = x * c;
    q = -(x * s);
}

} // namespace psdk
