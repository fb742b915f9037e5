// cross_readout.hip -- the kernels of the bank read-out of the pair and matrix objects (psdcxr_*; include/psdcascade_crossread.h,
// arithmetic in cross_readout.h).
//
//   cross_stitch_kernel  every included stage of every selected unit in one launch, as bank_stitch_kernel: one thread a bin,
//                        workgroup blockIdx.x serves tile blockIdx.x % tiles of job blockIdx.x / tiles (jobs along x: no 65535
//                        limit), the job uniform over the workgroup.  A thread loads the f64 accumulators of its bin, one from each
//                        row (consecutive threads on consecutive bins of a row: coalesced), and writes every requested output.
//                        PAIR: the four rows xx, yy, re, im held in registers; sxx, syy, sxy, freq, coherence and transfer from
//                        them in this one launch.  Otherwise: a loop over the job's rows (m * m <= 16) into [unit][row][stride].
//                        No LDS, no scratch, no atomics.
//   cross_band_kernel    bank_band_kernel with four row sums a band: one workgroup a selected pair, every thread walks the pair's
//                        stitched rows in a stride of BANK_BAND_THREADS and keeps 4 x 8 f64 sums, lane 0 of each wavefront gets the
//                        wavefront's sums through a shuffle tree, thread 0 adds the four wavefronts from LDS in order.
// Built with -ffp-contract=off, as bank_readout.hip: every product rounds before it is added.
#include <hip/hip_runtime.h>

#include "cross_readout.h"

namespace psdk {

template <bool PAIR>
__global__ __launch_bounds__(XREAD_THREADS) void cross_stitch_kernel(const CrossReadJob *__restrict__ jobs, uint32_t tiles, const CrossPairOut pair,
                                                                     float *__restrict__ rows, float *__restrict__ freq, size_t stride)
{
    const CrossReadJob j = jobs[blockIdx.x / tiles];
    const uint32_t i = (blockIdx.x % tiles) * XREAD_THREADS + threadIdx.x;
    if (i >= j.bins_end - j.bins_start)
        return;
    if (PAIR)
        cross_pair_element(j, i, pair);
    else
        cross_rows_element(j, i, rows, freq, stride);
}

__global__ __launch_bounds__(BANK_BAND_THREADS) void cross_band_kernel(const CrossReadJob *__restrict__ jobs, const BankRow *__restrict__ units,
                                                                       const BankBands bands, double *__restrict__ out)
{
    __shared__ double part[BANK_MAX_BANDS][XREAD_PAIR_ROWS][BANK_BAND_THREADS / BANK_WAVE];
    const BankRow u = units[blockIdx.x];
    double acc[XREAD_PAIR_ROWS][BANK_MAX_BANDS];
#pragma unroll
    for (uint32_t r = 0; r < XREAD_PAIR_ROWS; ++r)
#pragma unroll
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
            acc[r][b] = 0.0;
    cross_band_thread(jobs + u.job0, u.njobs, u.len, threadIdx.x, BANK_BAND_THREADS, bands, acc);
    const uint32_t lane = threadIdx.x % BANK_WAVE, wave = threadIdx.x / BANK_WAVE;
#pragma unroll
    for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
#pragma unroll
        for (uint32_t r = 0; r < XREAD_PAIR_ROWS; ++r) {
            double v = acc[r][b];
#pragma unroll
            for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
                v += __shfl_down(v, off, BANK_WAVE);
            if (lane == 0)
                part[b][r][wave] = v;
        }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
#pragma unroll
            for (uint32_t r = 0; r < XREAD_PAIR_ROWS; ++r) {
                double sum = part[b][r][0];
#pragma unroll
                for (uint32_t w = 1; w < BANK_BAND_THREADS / BANK_WAVE; ++w)
                    sum += part[b][r][w];
                if (b < bands.n)
                    out[((size_t)blockIdx.x * bands.n + b) * XREAD_PAIR_ROWS + r] = sum;
            }
    }
}

// the grid of a stitch launch (0: more workgroups than a grid's x dimension takes)
static uint32_t stitch_grid(uint32_t n_jobs, uint32_t max_bins, uint32_t *tiles)
{
    *tiles = (max_bins + XREAD_THREADS - 1) / XREAD_THREADS;
    const uint64_t blocks = (uint64_t)*tiles * n_jobs;
    return blocks > 0x7FFFFFFFull ? 0 : (uint32_t)blocks;
}

hipError_t launch_cross_stitch_pair(const CrossReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const CrossPairOut &out, hipStream_t s)
{
    if (n_jobs == 0 || max_bins == 0 || !out.any())
        return hipSuccess;
    uint32_t tiles = 0;
    const uint32_t grid = stitch_grid(n_jobs, max_bins, &tiles);
    if (!d_jobs || !grid)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_stitch_kernel<true>, dim3(grid), dim3(XREAD_THREADS), 0, s, d_jobs, tiles, out, (float *)nullptr, (float *)nullptr,
                       out.stride);
    return hipGetLastError();
}

hipError_t launch_cross_stitch_rows(const CrossReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, float *d_rows, float *d_freq, size_t stride,
                                    hipStream_t s)
{
    if (n_jobs == 0 || max_bins == 0 || (!d_rows && !d_freq))
        return hipSuccess;
    uint32_t tiles = 0;
    const uint32_t grid = stitch_grid(n_jobs, max_bins, &tiles);
    if (!d_jobs || !grid)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_stitch_kernel<false>, dim3(grid), dim3(XREAD_THREADS), 0, s, d_jobs, tiles, CrossPairOut{}, d_rows, d_freq, stride);
    return hipGetLastError();
}

hipError_t launch_cross_band(const CrossReadJob *d_jobs, const BankRow *d_units, uint32_t n_units, const BankBands &bands, double *d_out,
                             hipStream_t s)
{
    if (n_units == 0 || bands.n == 0)
        return hipSuccess;
    if (!d_jobs || !d_units || !d_out || bands.n > BANK_MAX_BANDS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_band_kernel, dim3(n_units), dim3(BANK_BAND_THREADS), 0, s, d_jobs, d_units, bands, d_out);
    return hipGetLastError();
}

} // namespace psdk
