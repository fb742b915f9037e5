// iq.h -- launch interface of the IQ cascade's front end (iq.hip, iq_frames.hip): the complex mixer / de-interleaver in front of
// stage 0 and the frames decoder that routes two traces into one channel.  Everything behind them is the zoom object's
// (zoom.h: zoom_kernel<N>, and the pair object's decimator, fold and tails).
#pragma once
#include "zoom.h"

namespace psdk {

// One call's complex samples of one channel through the mixer: sample i (i < len) is stream sample j0 + i and has the phase
// phase0 + ftw (j0 + i) mod 2^64; I' goes to dst_i[i], Q' to dst_q[i] (iq_lo.h).  dst_i and dst_q are equally aligned.
// Planar: src_i and src_q are the two streams, each 4-byte aligned.  Interleaved: src_i points to (re, im) pairs, 8-byte
// aligned, and src_q is not used.
struct IqMixJob {
    const float *src_i;
    const float *src_q;
    float *dst_i;
    float *dst_q;
    unsigned long long len;
    unsigned long long j0;
    unsigned long long ftw;
    unsigned long long phase0;
};

// Frames decoded and mixed straight into the stage-0 I / Q streams (iq_frames.hip): ZoomFramesBatch with two traces a channel.
// For every channel k < nch, trace trace_i[k] is I and trace trace_q[k] is Q of the complex sample (they may be the same trace,
// and a trace may go to several channels); the rest is as in ZoomFramesBatch.
struct IqFramesBatch {
    const uint8_t *frames;
    unsigned long long frame_size;
    unsigned n_frames;
    int batches;
    int fmt; // 1 AdcDac, 2 Fls, 3 ThermostatEem, 4 Mpll
    int nch;
    int trace_i[ZOOM_FRAMES_MAX_CH];
    int trace_q[ZOOM_FRAMES_MAX_CH];
    float *dst_i[ZOOM_FRAMES_MAX_CH];
    float *dst_q[ZOOM_FRAMES_MAX_CH];
    unsigned long long ftw[ZOOM_FRAMES_MAX_CH];
    unsigned long long phase0[ZOOM_FRAMES_MAX_CH];
    unsigned long long j0[ZOOM_FRAMES_MAX_CH];
};

hipError_t launch_iq_mix(const IqMixJob &j, bool interleaved, hipStream_t s);
hipError_t launch_iq_frames(const IqFramesBatch &b, hipStream_t s);

} // namespace psdk
