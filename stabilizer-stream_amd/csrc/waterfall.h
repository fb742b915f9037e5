// waterfall.h -- launch interface of the waterfall cascades' read-out kernels (waterfall.hip, waterfall_robust.hip), driven by
// cross_runtime.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace psdk {

// One (unit, stage) ring read out as images: the newest `nr` blocks, oldest first.  A ring slot holds 2 * sides rows of nbins
// f64: S1 of every side, then S2 of every side (sides 1: sk_fft.h's rows; sides 2: zoom_sk_fft.h's, upper before lower).
// psd / sk: [nr][sides][nbins] f32 in device memory, either may be NULL.  Every row but the newest holds `block` segments.
struct WfImageJob {
    const double *ring;
    float *psd, *sk;
    unsigned long long started; // blocks started (the newest may be partial)
    unsigned depth;             // K: slots of the ring
    unsigned nr;                // rows to write, 1 ... min(K, started)
    unsigned nbins, sides;
    unsigned block, newest;     // segments of a full block and of the newest one
    float gsc_block, gsc_newest; // 1 / (gain(count) * decimation) for those two counts
};

// One (unit, stage) ring reduced along time by wf_robust_kernel (waterfall_robust.hip; waterfall_robust.h is the arithmetic): the
// `rows` complete blocks that end with block `last`, every one of `block` segments.  The outputs are [sides][nbins] in device
// memory, any may be NULL: median, min, max and excised in f32, scaled by g; kept in u32.
struct WfRobustJob {
    const double *ring;
    float *median, *min, *max, *excised;
    unsigned *kept;
    unsigned long long started; // blocks started (the newest may be partial and is then not among the rows)
    unsigned long long last;    // the newest considered block
    unsigned depth;             // K: slots of the ring
    unsigned rows;              // R: 1 ... min(4096, complete blocks the ring holds)
    unsigned nbins, sides;
    unsigned block;             // B
    double g;                   // (double)gsc_block of WfImageJob
    double sk_lo, sk_hi;        // a row is kept for `excised` iff its SK in f64 lies in [sk_lo, sk_hi]
};

#if defined(__HIPCC__)
hipError_t launch_wf_image(const WfImageJob &j, hipStream_t s);
hipError_t launch_wf_robust(const WfRobustJob &j, hipStream_t s);
#endif

} // namespace psdk
