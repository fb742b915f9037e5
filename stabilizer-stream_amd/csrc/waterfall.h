// waterfall.h -- launch interface of the waterfall cascades' read-out kernel (waterfall.hip), driven by cross_runtime.cpp.
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

#if defined(__HIPCC__)
hipError_t launch_wf_image(const WfImageJob &j, hipStream_t s);
#endif

} // namespace psdk
