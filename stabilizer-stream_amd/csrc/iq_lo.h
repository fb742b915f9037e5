// iq_lo.h -- the complex mixer of the IQ cascade (psdc_iq_*, iq.hip, iq_frames.hip): a complex f32 sample z = I + i Q turned by
// the local oscillator of zoom_lo.h, z' = z exp(-2 pi i phase / 2^64).
//
// With (c, s) = zoom_lo(phase), unchanged, the f32 operations are fixed:
//     I' = fmaf(Q, s,  I * c)
//     Q' = fmaf(Q, c, -(I * s))
// Each is one stand-alone product and one explicit fmaf: nothing is left for a compiler to contract, so the host and the device
// run the same operations and agree bit for bit (tests/host/iq_emul.cpp runs this header on the host).  The order has two
// consequences the tests lean on:
//   Q = 0          fmaf(0, s, I c) = I c and fmaf(0, c, -(I s)) = -(I s): zoom_mix's x c and -(x s), up to the sign of a zero;
//   phase = 0      c = 1 and s = 0 exactly, so I' = Q 0 + I = I and Q' = Q - I 0 = Q for finite input (again up to the sign of
//                  a zero: -0 comes back as +0).
#pragma once
#include "zoom_lo.h"

namespace psdk {

// z' = z (c - i s): the rotation, given the oscillator's pair
ZOOM_HD void iq_rotate(float i, float q, float c, float s, float &io, float &qo)
{
    io = fmaf(q, s, i * c);
    qo = fmaf(q, c, -(i * s));
}

// one complex sample through the mixer: z' = z exp(-2 pi i phase / 2^64)
ZOOM_HD void iq_mix(float i, float q, uint64_t phase, float &io, float &qo)
{
    float c, s;
    zoom_lo(phase, c, s);
    iq_rotate(i, q, c, s, io, qo);
}

} // namespace psdk
