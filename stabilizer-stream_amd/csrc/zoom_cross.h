// zoom_cross.h -- launch interface of the zoom cross kernel (zoom_cross.hip): two real streams around a carrier each, the
// two-sided auto spectra of both and their cross spectrum.  The jobs are the matrix object's (csm.h) with four streams:
// src[0], src[1] are I and Q of channel a, src[2], src[3] those of channel b; a workgroup's partial is the eight rows of
// zoom_cross_fft.h.  The mixer is zoom_mix_kernel (zoom.h), one launch a channel; decimator, fold and tails are the pair object's.
#pragma once
#include "csm.h"
#include "zoom.h"

namespace psdk {

bool zoom_cross_supported(int n); // 64 ... 4096, powers of two
int zoom_cross_segments_per_tile(int n);
int zoom_cross_block_threads(int n);
hipError_t launch_zoom_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
