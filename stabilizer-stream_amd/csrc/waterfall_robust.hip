// waterfall_robust.hip -- the robust read-out kernel of the waterfall cascades (psdcx_wf_robust*, psdcx_zwf_robust*;
// include/psdcascade_robust.h).
//
//   wf_robust_kernel  reduces the newest R complete blocks of one (unit, stage) ring along time: per (side, bin) the median, the
//                     minimum, the maximum and the SK-excised mean of S1 with the number of rows kept (waterfall_robust.h is the
//                     arithmetic).  One thread a (side, bin), consecutive threads on consecutive bins: every pass over the rows
//                     reads consecutive f64 of one slot; the outputs are consecutive f32 / u32.  No LDS, no scratch: the median
//                     is a bisection on the bit pattern, which re-reads the rows (they sit in L2) and keeps nothing per row.
#include "waterfall.h"
#include "waterfall_robust.h"

namespace psdk {

constexpr int WF_ROBUST_THREADS = 256;

__global__ __launch_bounds__(WF_ROBUST_THREADS) void wf_robust_kernel(const WfRobustJob j)
{
    const unsigned xb = (j.nbins + WF_ROBUST_THREADS - 1) / WF_ROBUST_THREADS; // workgroups a side
    const unsigned side = blockIdx.x / xb;
    const unsigned k = (blockIdx.x % xb) * WF_ROBUST_THREADS + threadIdx.x;
    if (k >= j.nbins)
        return;
    WfRobustRows w;
    w.ring = j.ring;
    w.last = j.last;
    w.K = j.depth;
    w.R = j.rows;
    w.set = (size_t)2 * j.sides * j.nbins;
    w.o1 = (size_t)side * j.nbins + k;
    w.o2 = (size_t)(j.sides + side) * j.nbins + k;
    const WfRobustBin b = wf_robust_bin(w, j.block, j.g, j.sk_lo, j.sk_hi, j.median != nullptr, j.excised || j.kept);
    const size_t o = (size_t)side * j.nbins + k;
    if (j.median)
        j.median[o] = b.median;
    if (j.min)
        j.min[o] = b.min;
    if (j.max)
        j.max[o] = b.max;
    if (j.excised)
        j.excised[o] = b.excised;
    if (j.kept)
        j.kept[o] = b.kept;
}

hipError_t launch_wf_robust(const WfRobustJob &j, hipStream_t s)
{
    if (j.rows == 0 || (!j.median && !j.min && !j.max && !j.excised && !j.kept))
        return hipSuccess;
    if (!j.ring || j.nbins == 0 || j.sides == 0 || j.depth == 0 || j.block < 2 || j.rows > j.depth || j.rows > WF_ROBUST_MAX_ROWS ||
        j.last >= j.started || j.started - j.last > j.depth || j.rows > j.last + 1 || j.started - j.last - 1 + j.rows > j.depth)
        return hipErrorInvalidValue;
    const unsigned xb = (j.nbins + WF_ROBUST_THREADS - 1) / WF_ROBUST_THREADS;
    hipLaunchKernelGGL(wf_robust_kernel, dim3(j.sides * xb), dim3(WF_ROBUST_THREADS), 0, s, j);
    return hipGetLastError();
}

} // namespace psdk
