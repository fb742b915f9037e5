// zoom_ampm_cross.h -- launch interface of the AM/PM cross cascades' segment kernel (zoom_ampm_cross.hip).  The jobs and the tile
// are zoom_cross_kernel's (zoom_cross.h: src[0], src[1] are I and Q of channel a, src[2], src[3] those of channel b, one segment a
// team, zoom_cross_segments_per_tile); a workgroup's partial is the twelve rows of zoom_ampm_cross_fft.h.  The host runtime does
// not call this launcher: it marks the batch (CsmBatch::variant) and launch_zoom_cross sends it here.
#pragma once
#include "zoom_cross.h"

namespace psdk {

hipError_t launch_zoom_ampm_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
