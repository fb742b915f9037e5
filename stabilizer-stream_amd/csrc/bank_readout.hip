// bank_readout.hip -- the kernels of the bank read-out (psdcr_*; include/psdcascade_readout.h, arithmetic in bank_readout.h).
//
//   bank_stitch_kernel  every included stage of every selected row in one launch: one thread an output element, consecutive
//                       threads on consecutive bins of a job; workgroup blockIdx.x serves tile blockIdx.x % tiles of job
//                       blockIdx.x / tiles (jobs along x: no 65535 limit).  The job is uniform over the workgroup; plain coalesced
//                       f32 loads and stores, one f32 multiply an element.  No LDS, no scratch.
//   bank_band_kernel    one workgroup a selected row: every thread walks the row in a stride of BANK_BAND_THREADS and keeps up to 8
//                       f64 sums, lane 0 of each wavefront gets the wavefront's sums through a shuffle tree, thread 0 adds the
//                       four wavefronts from LDS in order and stores the row's results.  The order is a function of the row's
//                       length alone: no atomics.
// Both are bound by latency, not by traffic (64 channels of six stages are about 100 KB).
#include <hip/hip_runtime.h>

#include "bank_readout.h"

namespace psdk {

__global__ __launch_bounds__(BANK_STITCH_THREADS) void bank_stitch_kernel(const BankJob *__restrict__ jobs, uint32_t tiles,
                                                                          float *__restrict__ psd, float *__restrict__ freq, size_t stride)
{
    const BankJob j = jobs[blockIdx.x / tiles];
    const uint32_t i = (blockIdx.x % tiles) * BANK_STITCH_THREADS + threadIdx.x;
    if (i >= j.bins_end - j.bins_start)
        return;
    const uint32_t k = j.bins_start + i;
    const size_t o = (size_t)j.row * stride + j.start + i;
    if (psd)
        psd[o] = bank_psd(j, k);
    if (freq)
        freq[o] = bank_freq(j, k);
}

__global__ __launch_bounds__(BANK_BAND_THREADS) void bank_band_kernel(const BankJob *__restrict__ jobs, const BankRow *__restrict__ rows,
                                                                      const BankBands bands, double *__restrict__ out)
{
    __shared__ double part[BANK_MAX_BANDS][BANK_BAND_THREADS / BANK_WAVE];
    const BankRow r = rows[blockIdx.x];
    double acc[BANK_MAX_BANDS];
#pragma unroll
    for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
        acc[b] = 0.0;
    bank_band_thread(jobs + r.job0, r.njobs, r.len, threadIdx.x, BANK_BAND_THREADS, bands, acc);
    const uint32_t lane = threadIdx.x % BANK_WAVE, wave = threadIdx.x / BANK_WAVE;
#pragma unroll
    for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b) {
        double v = acc[b];
#pragma unroll
        for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
            v += __shfl_down(v, off, BANK_WAVE);
        if (lane == 0)
            part[b][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b) {
            double sum = part[b][0];
#pragma unroll
            for (uint32_t w = 1; w < BANK_BAND_THREADS / BANK_WAVE; ++w)
                sum += part[b][w];
            if (b < bands.n)
                out[(size_t)blockIdx.x * bands.n + b] = sum;
        }
    }
}

hipError_t launch_bank_stitch(const BankJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, float *d_psd, float *d_freq, size_t stride,
                              hipStream_t s)
{
    if (n_jobs == 0 || max_bins == 0 || (!d_psd && !d_freq))
        return hipSuccess;
    if (!d_jobs)
        return hipErrorInvalidValue;
    const uint64_t tiles = (max_bins + BANK_STITCH_THREADS - 1) / BANK_STITCH_THREADS;
    if (tiles * n_jobs > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_stitch_kernel, dim3((uint32_t)(tiles * n_jobs)), dim3(BANK_STITCH_THREADS), 0, s, d_jobs, (uint32_t)tiles, d_psd,
                       d_freq, stride);
    return hipGetLastError();
}

hipError_t launch_bank_band(const BankJob *d_jobs, const BankRow *d_rows, uint32_t n_rows, const BankBands &bands, double *d_out,
                            hipStream_t s)
{
    if (n_rows == 0 || bands.n == 0)
        return hipSuccess;
    if (!d_jobs || !d_rows || !d_out || bands.n > BANK_MAX_BANDS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(bank_band_kernel, dim3(n_rows), dim3(BANK_BAND_THREADS), 0, s, d_jobs, d_rows, bands, d_out);
    return hipGetLastError();
}

} // namespace psdk
