// iq_cross.h -- launch interface of the IQ cross cascade's front end (iq_cross.hip, iq_cross_frames.hip): the pair mixer that turns
// two complex streams in one launch, and the frames decoder that routes four traces into one pair.  Everything behind them is the
// zoom cross object's (zoom_cross.h: zoom_cross_kernel<N> and its eight rows, and the pair object's decimator, fold and tails).
#pragma once
#include "zoom_cross.h"

namespace psdk {

// One call's complex samples of both sides of a pair through the mixer.  Sample i (i < len) is stream sample j0 + i of both sides
// (a pair's streams move together); side s has the phase phase0[s] + ftw[s] (j0 + i) mod 2^64, and its I' goes to dst[2 s][i], its
// Q' to dst[2 s + 1][i] (iq_lo.h).  The four destinations are equally aligned.
// Planar: src[0 ... 3] are the streams I_a, Q_a, I_b, Q_b, each 4-byte aligned.  Interleaved: src[0] and src[2] point to the
// (re, im) pairs of side a and side b, each 8-byte aligned, and src[1], src[3] are not used.
struct IqPairMixJob {
    const float *src[4];
    float *dst[4];
    unsigned long long len;
    unsigned long long j0;
    unsigned long long ftw[2];
    unsigned long long phase0[2];
};

// Frames decoded and mixed straight into the four stage-0 streams of IQ cross pairs (iq_cross_frames.hip): ZoomCrossFramesBatch
// with two traces a side.  For every pair p < npairs, traces trace[p][0] and trace[p][1] are I and Q of side a and trace[p][2],
// trace[p][3] those of side b; side s is mixed with carrier (ftw[p][s], phase0[p][s]) into dst[p][2 s] and dst[p][2 s + 1].  A
// trace may go to any number of entries; the rest is as in ZoomCrossFramesBatch.
constexpr int IQ_CROSS_FRAMES_MAX_PAIRS = CROSS_FRAMES_MAX_DST / 4;
struct IqCrossFramesBatch {
    const uint8_t *frames;
    unsigned long long frame_size;
    unsigned n_frames;
    int batches;
    int fmt; // 1 AdcDac, 2 Fls, 3 ThermostatEem, 4 Mpll
    int npairs;
    int trace[IQ_CROSS_FRAMES_MAX_PAIRS][4];
    float *dst[IQ_CROSS_FRAMES_MAX_PAIRS][4];
    unsigned long long ftw[IQ_CROSS_FRAMES_MAX_PAIRS][2];
    unsigned long long phase0[IQ_CROSS_FRAMES_MAX_PAIRS][2];
    unsigned long long j0[IQ_CROSS_FRAMES_MAX_PAIRS];
};

hipError_t launch_iq_pair_mix(const IqPairMixJob &j, bool interleaved, hipStream_t s);
hipError_t launch_iq_cross_frames(const IqCrossFramesBatch &b, hipStream_t s);

} // namespace psdk
