// carrier_readout.hip -- the kernels of the bank read-out of the zoom, IQ, zoom / IQ SK and zoom / IQ AM/PM objects (psdczr_*;
// include/psdcascade_carrierread.h, arithmetic in carrier_readout.h).
//
//   carrier_stitch_kernel<MODE>  cross_stitch_kernel's shape: one thread a bin, workgroup blockIdx.x < tile_blocks serves tile
//                                blockIdx.x % tiles of job blockIdx.x / tiles (jobs along x), the job uniform over the workgroup.
//                                A thread loads the f64 accumulators of its bin (two: upper, lower; the other two only for an SK
//                                or AM/PM output; consecutive threads on consecutive bins of a row: coalesced) and writes every
//                                requested output.  AM/PM: the channel's unit record is workgroup-uniform too; every thread
//                                forms the carrier from it (bin 0 of stage 0: four uniform loads, two square roots).  The
//                                workgroups behind the tiles write the carrier records, one thread a selected channel.
//                                No LDS, no scratch, no atomics.
//   carrier_band_kernel<R>       cross_band_kernel on bank_band_walk<R>: one workgroup a selected channel, R = 2 (upper, lower) or
//                                4 (and s_am, s_pm in f64), the same thread stride, shuffle tree and order of the wavefronts.
// Built with -ffp-contract=off, as bank_readout.hip: every product rounds before it is added.
#include <hip/hip_runtime.h>

#include "carrier_readout.h"

namespace psdk {

template <int MODE>
__global__ __launch_bounds__(XREAD_THREADS) void carrier_stitch_kernel(const CarrierReadJob *__restrict__ jobs, uint32_t tiles, uint32_t tile_blocks,
                                                                       const CarrierOut out, const CarrierUnit *__restrict__ units, uint32_t n_units)
{
    if (blockIdx.x >= tile_blocks) { // (MODE == CREAD_AMPM with out.carrier alone)
        const uint32_t unit = (blockIdx.x - tile_blocks) * XREAD_THREADS + threadIdx.x;
        if (MODE == CREAD_AMPM && unit < n_units)
            carrier_record(units, unit, out.carrier);
        return;
    }
    const CarrierReadJob j = jobs[blockIdx.x / tiles];
    const uint32_t i = (blockIdx.x % tiles) * XREAD_THREADS + threadIdx.x;
    if (i >= j.bins_end - j.bins_start)
        return;
    carrier_element<MODE>(j, i, out, units);
}

template <uint32_t R, class Val>
__device__ __forceinline__ void carrier_band_block(const CarrierReadJob *__restrict__ jobs, const BankRow u, const BankBands &bands, const Val &val,
                                                   double *__restrict__ out)
{
    __shared__ double part[BANK_MAX_BANDS][R][BANK_BAND_THREADS / BANK_WAVE];
    double acc[R][BANK_MAX_BANDS];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r)
#pragma unroll
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
            acc[r][b] = 0.0;
    bank_band_walk<R>(jobs + u.job0, u.njobs, u.len, threadIdx.x, BANK_BAND_THREADS, bands, val, acc);
    const uint32_t lane = threadIdx.x % BANK_WAVE, wave = threadIdx.x / BANK_WAVE;
#pragma unroll
    for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
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
            for (uint32_t r = 0; r < R; ++r) {
                double sum = part[b][r][0];
#pragma unroll
                for (uint32_t w = 1; w < BANK_BAND_THREADS / BANK_WAVE; ++w)
                    sum += part[b][r][w];
                if (b < bands.n)
                    out[((size_t)blockIdx.x * bands.n + b) * R + r] = sum;
            }
    }
}

template <uint32_t R>
__global__ __launch_bounds__(BANK_BAND_THREADS) void carrier_band_kernel(const CarrierReadJob *__restrict__ jobs, const BankRow *__restrict__ units,
                                                                         const CarrierUnit *__restrict__ cunits, const BankBands bands,
                                                                         double *__restrict__ out)
{
    if (R == CREAD_ROWS)
        carrier_band_block<R>(jobs, units[blockIdx.x], bands, carrier_ampm_val(cunits[blockIdx.x]), out);
    else
        carrier_band_block<R>(jobs, units[blockIdx.x], bands, CarrierSideVal{}, out);
}

hipError_t launch_carrier_stitch(int mode, const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const CarrierOut &out,
                                 const CarrierUnit *d_units, uint32_t n_units, hipStream_t s)
{
    const bool rows = out.any_row() && n_jobs && max_bins, records = mode == CREAD_AMPM && out.carrier && n_units;
    if (!rows && !records)
        return hipSuccess;
    if (mode != CREAD_SIDES && mode != CREAD_SK && mode != CREAD_AMPM)
        return hipErrorInvalidValue;
    if ((rows && !d_jobs) || (mode == CREAD_AMPM && !d_units))
        return hipErrorInvalidValue;
    const uint32_t tiles = rows ? (max_bins + XREAD_THREADS - 1) / XREAD_THREADS : 0;
    const uint64_t tile_blocks = (uint64_t)tiles * n_jobs;
    const uint64_t blocks = tile_blocks + (records ? (n_units + XREAD_THREADS - 1) / XREAD_THREADS : 0);
    if (blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)blocks), block(XREAD_THREADS);
    if (mode == CREAD_SIDES)
        hipLaunchKernelGGL(carrier_stitch_kernel<CREAD_SIDES>, grid, block, 0, s, d_jobs, tiles, (uint32_t)tile_blocks, out, d_units, n_units);
    else if (mode == CREAD_SK)
        hipLaunchKernelGGL(carrier_stitch_kernel<CREAD_SK>, grid, block, 0, s, d_jobs, tiles, (uint32_t)tile_blocks, out, d_units, n_units);
    else
        hipLaunchKernelGGL(carrier_stitch_kernel<CREAD_AMPM>, grid, block, 0, s, d_jobs, tiles, (uint32_t)tile_blocks, out, d_units, n_units);
    return hipGetLastError();
}

hipError_t launch_carrier_band(uint32_t rows, const CarrierReadJob *d_jobs, const BankRow *d_units, const CarrierUnit *d_cunits, uint32_t n_units,
                               const BankBands &bands, double *d_out, hipStream_t s)
{
    if (n_units == 0 || bands.n == 0)
        return hipSuccess;
    if (!d_jobs || !d_units || !d_out || bands.n > BANK_MAX_BANDS || (rows != CREAD_SIDE_ROWS && rows != CREAD_ROWS) || (rows == CREAD_ROWS && !d_cunits))
        return hipErrorInvalidValue;
    if (rows == CREAD_ROWS)
        hipLaunchKernelGGL(carrier_band_kernel<CREAD_ROWS>, dim3(n_units), dim3(BANK_BAND_THREADS), 0, s, d_jobs, d_units, d_cunits, bands, d_out);
    else
        hipLaunchKernelGGL(carrier_band_kernel<CREAD_SIDE_ROWS>, dim3(n_units), dim3(BANK_BAND_THREADS), 0, s, d_jobs, d_units, d_cunits, bands, d_out);
    return hipGetLastError();
}

} // namespace psdk
