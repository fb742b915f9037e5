// cross.h -- launch interface between the cross-spectral host runtime (cross_runtime.cpp) and its gfx950 kernels (cross.hip).
// Job tables travel by value in the kernel-argument segment, as in kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace psdk {

constexpr int CROSS_MAX_JOBS = 128;  // (pair, stage) jobs per cross launch
constexpr int CROSS_MAX_FOLD = 128;  // (pair, stage) folds per epilogue launch
constexpr int CROSS_MAX_TAIL = 256;  // stream-tail copies per epilogue launch ((pair, stage) x 2 channels)

// One span of consecutive segments of one (pair, stage): both channels' streams share the base index.
struct CrossJob {
    const float *src[2]; // channel x / y: sample with absolute stream index i is src[c][i - src_base]
    long long src_base;
    long long seg0;      // absolute index of the first segment (segment j starts at j * hop)
    float *partial;      // [nblocks][4][n/2 + 1]: xx, yy, re, im partial rows of each workgroup
    double log2_gamma;   // EWMA as in SegJob (plan.h)
    int nseg;
    int block_begin;
    int nblocks;
    int ntiles;
    int step0;
    int nb;
    int is_m1;
    int ewma;
};

struct CrossBatch {
    int njobs;
    int nblocks;
    int hop;
    int detrend;
    CrossJob jobs[CROSS_MAX_JOBS];
};

// acc[r][k] = g_total acc[r][k] + sum_b partial[b][r][k], in f64, b in order; r < CrossPostBatch::nrows
// fresh != 0: acc[r][k] = sum_b partial[b][r][k], and acc is not read (a waterfall ring slot taken over by a new block: what it
// held may be anything, a NaN included, which g_total = 0 would keep)
struct CrossFoldJob {
    const float *partial;
    double *acc; // [nrows][n/2 + 1]
    double g_total;
    int nparts;
    int fresh;
};

// carry a stream tail to the front of the other buffer: workgroups [block_begin, block_begin + nblocks) of the tail part of the
// grid, CROSS_TAIL_CHUNK samples each (a decimated stage's tail holds what the stage above produced this round: 2^21 samples
// behind a 2^24-sample call)
constexpr int CROSS_TAIL_CHUNK = 1 << 15;
struct CrossTailJob {
    const float *src;
    float *dst;
    long long count;
    int block_begin;
    int nblocks;
};

struct CrossPostBatch {
    int nfold;
    int nbins;      // n/2 + 1
    int nrows;      // real rows of every fold job: 4 for a pair, m * m for a group of m channels (csm.h)
    int fold_xb;    // workgroups per fold job (cross_fold_blocks)
    int ntail;
    int tail_blocks;
    CrossFoldJob fold[CROSS_MAX_FOLD];
    CrossTailJob tail[CROSS_MAX_TAIL];
};

// Frames decoded straight into the stage-0 streams (cross_frames.hip): one launch reads n_frames frames of format `fmt` and writes
// trace trace[k] of them to dst[k], k < ndst (the x / y buffers of up to 16 pairs; a trace may go to several).  dst[k] receives
// n_frames * batches * (8 for AdcDac, else 1) samples.
constexpr int CROSS_FRAMES_MAX_DST = 32;
struct CrossFramesBatch {
    const uint8_t *frames;
    unsigned long long frame_size;
    unsigned n_frames;
    int batches;
    int fmt;  // 1 AdcDac, 2 Fls, 3 ThermostatEem, 4 Mpll
    int ndst;
    int trace[CROSS_FRAMES_MAX_DST];
    float *dst[CROSS_FRAMES_MAX_DST];
};

bool cross_supported(int n);             // 64 ... 4096, powers of two
int cross_segments_per_tile(int n);
int cross_block_threads(int n); // threads of a cross_kernel workgroup (one wavefront a SIMD: its registers allow no more)
int cross_fold_blocks(int nrows, int nbins); // workgroups of one fold job
hipError_t launch_cross(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);
hipError_t launch_cross_post(const CrossPostBatch &b, hipStream_t s);
hipError_t launch_cross_frames(const CrossFramesBatch &b, hipStream_t s);

} // namespace psdk
