// waterfall.hip -- the read-out kernel of the waterfall cascades (psdc_wf_*, psdc_zwf_*).
//
//   wf_image_kernel   unrolls one (unit, stage) ring into images: row r of the output is the r-th oldest of the newest `nr`
//                     blocks (waterfall_read.h maps it to its slot), every element the PSD and / or the spectral kurtosis of one
//                     bin of one side from the slot's f64 moments.  One thread a bin of a row: consecutive threads read
//                     consecutive f64 and write consecutive f32; no LDS, no scratch.
// The segment kernels that fill the rings are sk_kernel and zoom_sk_kernel, unchanged.
#include "waterfall.h"
#include "waterfall_read.h"

namespace psdk {

constexpr int WF_THREADS = 256;

__global__ __launch_bounds__(WF_THREADS) void wf_image_kernel(const WfImageJob j)
{
    const unsigned xb = (j.nbins + WF_THREADS - 1) / WF_THREADS; // workgroups a row
    const unsigned row = blockIdx.x / xb;                        // r * sides + side
    const unsigned k = (blockIdx.x % xb) * WF_THREADS + threadIdx.x;
    if (k >= j.nbins)
        return;
    const unsigned r = row / j.sides, side = row % j.sides;
    const bool newest = r + 1 == j.nr;
    const unsigned count = newest ? j.newest : j.block;
    const double *slot = j.ring + (size_t)wf_row_slot(j.started, j.depth, j.nr, r) * 2 * j.sides * j.nbins;
    const double s1 = slot[(size_t)side * j.nbins + k];
    const size_t o = (size_t)row * j.nbins + k;
    if (j.psd)
        j.psd[o] = wf_psd(s1, newest ? j.gsc_newest : j.gsc_block);
    if (j.sk)
        j.sk[o] = wf_sk(count, s1, slot[(size_t)(j.sides + side) * j.nbins + k]);
}

hipError_t launch_wf_image(const WfImageJob &j, hipStream_t s)
{
    if (j.nr == 0 || (!j.psd && !j.sk))
        return hipSuccess;
    if (!j.ring || j.nbins == 0 || j.sides == 0 || j.depth == 0 || j.nr > j.depth || j.nr > j.started)
        return hipErrorInvalidValue;
    const unsigned xb = (j.nbins + WF_THREADS - 1) / WF_THREADS;
    hipLaunchKernelGGL(wf_image_kernel, dim3(j.nr * j.sides * xb), dim3(WF_THREADS), 0, s, j);
    return hipGetLastError();
}

} // namespace psdk
