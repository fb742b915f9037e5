// zoom_sk.h -- launch interface of the zoom / IQ spectral kurtosis cascades' segment kernel (zoom_sk.hip).  The jobs and the tile
// are zoom_kernel's (zoom.h: src[0] the I stream, src[1] the Q stream, one segment a team, zoom_segments_per_tile); a
// workgroup's partial is 4 rows of n/2 + 1: S1 upper, S1 lower, S2 upper, S2 lower (zoom_sk_fft.h).  Mixers, decimator, fold and
// tails are those of the zoom object.
#pragma once
#include "zoom.h"

namespace psdk {

hipError_t launch_zoom_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
