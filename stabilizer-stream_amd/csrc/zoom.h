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

int zoom_segments_per_tile(int n);
int zoom_block_threads(int n);
hipError_t launch_zoom(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);
hipError_t launch_zoom_mix(const ZoomMixJob &j, hipStream_t s);

} // namespace psdk
