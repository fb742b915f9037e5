// csm.h -- launch interface of the cross-spectral matrix kernel (csm.hip): groups of m = 2 ... 4 channels, every channel
// transformed once a segment, every product conj(X_a) X_b accumulated.  The decimator, the fold + tail epilogue and the frame
// decoder are those of the pair object (kernels.h, cross.h).
#pragma once
#include "cross.h"

namespace psdk {

constexpr int CSM_MAX_M = 4;
constexpr int CSM_MAX_JOBS = 128; // (group, stage) jobs per csm launch

// One span of consecutive segments of one (group, stage): the channels' streams share the base index.  The fields after src
// are CrossJob's.
struct CsmJob {
    const float *src[CSM_MAX_M];
    long long src_base;
    long long seg0;
    float *partial; // [nblocks][m * m][n/2 + 1]: the partial rows of each workgroup, rows as in csm_fft.h
    double log2_gamma;
    int nseg;
    int block_begin;
    int nblocks;
    int ntiles;
    int step0;
    int nb;
    int is_m1;
    int ewma;
};

struct CsmBatch {
    int njobs;
    int nblocks;
    int hop;
    int detrend;
    int variant; // 0 unless set: which segment kernel launch_zoom_cross runs (zoom_ampm_cross_fft.h); the other launchers do not read it
    CsmJob jobs[CSM_MAX_JOBS];
};

bool csm_supported(int n, int m); // n 64 ... 2048 for m 2 ... 4, and n 4096 for m = 2, 3
int csm_segments_per_tile(int n, int m);
int csm_block_threads(int n, int m);
hipError_t launch_csm(int n, int m, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
