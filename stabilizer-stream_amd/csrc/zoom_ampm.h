// zoom_ampm.h -- launch interface of the AM/PM cascades' segment kernel (zoom_ampm.hip).  The jobs and the tile are zoom_kernel's
// (zoom.h: src[0] the I stream, src[1] the Q stream, one segment a team, zoom_segments_per_tile); a workgroup's partial is 4 rows
// of n/2 + 1: upper, lower, comp_re, comp_im (zoom_ampm_fft.h).  Mixers, decimator, fold and tails are those of the zoom object.
#pragma once
#include "zoom.h"

namespace psdk {

hipError_t launch_zoom_ampm(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
