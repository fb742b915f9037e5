// zoom_cross.h -- launch interface of the zoom cross kernel (zoom_cross.hip): two real streams around a carrier each, the
// two-sided auto spectra of both and their cross spectrum.  The jobs are the matrix object's (csm.h) with four streams:
// src[0], src[1] are I and Q of channel a, src[2], src[3] those of channel b; a workgroup's partial is the eight rows of
// zoom_cross_fft.h.  The mixer is zoom_mix_kernel (zoom.h), one launch a channel; decimator, fold and tails are the pair object's.
#pragma once
#include "csm.h"
#include "zoom.h"

namespace psdk {

// Frames decoded and mixed straight into the four stage-0 streams of zoom cross pairs (zoom_cross_frames.hip): one launch reads
// n_frames frames of format `fmt` and, for every pair p < npairs, mixes trace trace[p][0] of them with carrier (ftw[p][0],
// phase0[p][0]) into dst[p][0] (I_a) and dst[p][1] (Q_a), and trace trace[p][1] with carrier (ftw[p][1], phase0[p][1]) into
// dst[p][2] (I_b) and dst[p][3] (Q_b).  The four destinations of a pair are equally aligned; a trace may go to any number of
// sides, both sides of one pair included.  Sample i of the launch is stream sample j0[p] + i of both sides (a pair's streams
// move together) and has the phase phase0 + ftw (j0[p] + i) mod 2^64 of its side; a side receives n_frames * batches * (8 for
// AdcDac, else 1) samples.  Two sides with the same ftw and phase0 share one oscillator evaluation a sample.  A pair is four of
// the CROSS_FRAMES_MAX_DST destination streams of a frames launch.
constexpr int ZOOM_CROSS_FRAMES_MAX_PAIRS = CROSS_FRAMES_MAX_DST / 4;
struct ZoomCrossFramesBatch {
    const uint8_t *frames;
    unsigned long long frame_size;
    unsigned n_frames;
    int batches;
    int fmt; // 1 AdcDac, 2 Fls, 3 ThermostatEem, 4 Mpll
    int npairs;
    int trace[ZOOM_CROSS_FRAMES_MAX_PAIRS][2];
    float *dst[ZOOM_CROSS_FRAMES_MAX_PAIRS][4];
    unsigned long long ftw[ZOOM_CROSS_FRAMES_MAX_PAIRS][2];
    unsigned long long phase0[ZOOM_CROSS_FRAMES_MAX_PAIRS][2];
    unsigned long long j0[ZOOM_CROSS_FRAMES_MAX_PAIRS];
};

bool zoom_cross_supported(int n); // 64 ... 4096, powers of two
int zoom_cross_segments_per_tile(int n);
int zoom_cross_block_threads(int n);
hipError_t launch_zoom_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s);
hipError_t launch_zoom_cross_frames(const ZoomCrossFramesBatch &b, hipStream_t s);

} // namespace psdk
