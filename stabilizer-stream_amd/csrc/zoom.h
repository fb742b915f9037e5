// zoom.h -- launch interface of the zoom cascade's kernels (zoom.hip): the mixer in front of stage 0 and the two-sided
// |Z_k|^2 segment kernel.  The jobs are the pair object's (cross.h): src[0] is the I stream, src[1] the Q stream, and a
// workgroup's partial is 2 rows (upper, lower) of n/2 + 1.  Decimator, fold and tails are those of the pair object.
#pragma once
#include "cross.h"

namespace psdk {

// One call's samples of one channel through the mixer: sample i of x (i < len) is stream sample j0 + i and has phase
// phase0 + ftw (j0 + i) mod 2^64; I goes to dst_i[i], Q to dst_q[i].  dst_i and dst_q are equally aligned.
struct ZoomMixJob {
    const float *x;
    float *dst_i;
    float *dst_q;
    unsigned long long len;
    unsigned long long j0;
    unsigned long long ftw;
    unsigned long long phase0;
};

// Frames decoded and mixed straight into the stage-0 I / Q streams (zoom_frames.hip): one launch reads n_frames frames of format
// `fmt` and, for every channel k < nch, mixes trace trace[k] of them with the channel's carrier into dst_i[k] / dst_q[k] (equally
// aligned; a trace may go to several channels).  Sample i of the launch is stream sample j0[k] + i of channel k, with the phase
// phase0[k] + ftw[k] (j0[k] + i) mod 2^64; a channel receives n_frames * batches * (8 for AdcDac, else 1) samples.  A channel is
// two of the CROSS_FRAMES_MAX_DST destination streams of a frames launch.
constexpr int ZOOM_FRAMES_MAX_CH = CROSS_FRAMES_MAX_DST / 2;
struct ZoomFramesBatch {
    const uint8_t *frames;
    unsigned long long frame_size;
    unsigned n_frames;
    int batches;
    int fmt; // 1 AdcDac, 2 Fls, 3 ThermostatEem, 4 Mpll
    int nch;
    int trace[ZOOM_FRAMES_MAX_CH];
    float *dst_i[ZOOM_FRAMES_MAX_CH];
    float *dst_q[ZOOM_FRAMES_MAX_CH];
    unsigned long long ftw[ZOOM_FRAMES_MAX_CH];
    unsigned long long phase0[ZOOM_FRAMES_MAX_CH];
    unsigned long long j0[ZOOM_FRAMES_MAX_CH];
};

int zoom_segments_per_tile(int n);
int zoom_block_threads(int n);
hipError_t launch_zoom(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);
hipError_t launch_zoom_mix(const ZoomMixJob &j, hipStream_t s);
hipError_t launch_zoom_frames(const ZoomFramesBatch &b, hipStream_t s);

} // namespace psdk
