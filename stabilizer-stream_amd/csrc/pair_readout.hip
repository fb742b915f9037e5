// pair_readout.hip -- the kernels of the bank read-out of the zoom cross, IQ cross and zoom / IQ AM/PM cross objects (psdcpr_*;
// include/ext/psdcascade_pairread.h, arithmetic in pair_readout.h).
//
//   pair_stitch_kernel<MODE>   carrier_stitch_kernel's shape: one thread a bin, workgroup blockIdx.x < tile_blocks serves tile
//                              blockIdx.x % tiles of job blockIdx.x / tiles (jobs along x), the job uniform over the workgroup.
//                              A thread loads only the f64 rows its requested outputs need (the output pointers are kernel
//                              arguments: the choice is uniform; at most 8 loads in CSD mode, 8 of rows 4 ... 11 in AM/PM mode;
//                              consecutive threads on consecutive bins of a row: coalesced) and writes every requested output.
//                              AM/PM: the pair's unit record is workgroup-uniform too; every thread forms the carriers from it
//                              (bin 0 of stage 0: four uniform loads, two square roots).  The workgroups behind the tiles write
//                              the carrier records with the locks, one thread a selected pair.  No LDS, no scratch, no atomics.
//   pair_band_kernel<R, MODE>  carrier_band_kernel on bank_band_walk<R>: the same thread stride, shuffle tree and order of the
//                              wavefronts; workgroup (x, y) takes rows [y * R, y * R + R) of the eight of pair x.  Every row's sum is
//                              independent of the others, so R changes no bit.
// Built with -ffp-contract=off, as bank_readout.hip: every product rounds before it is added.
#include <hip/hip_runtime.h>

#include "pair_readout.h"

namespace psdk {

template <int MODE, class Out>
__global__ __launch_bounds__(XREAD_THREADS) void pair_stitch_kernel(const CarrierReadJob *__restrict__ jobs, uint32_t tiles, uint32_t tile_blocks,
                                                                    const Out out, const PairUnit *__restrict__ units, uint32_t n_units)
{
    if constexpr (MODE == PREAD_AMPM) {
        if (blockIdx.x >= tile_blocks) {
            const uint32_t unit = (blockIdx.x - tile_blocks) * XREAD_THREADS + threadIdx.x;
            if (unit < n_units)
                pair_record(units, unit, out.carrier);
            return;
        }
    }
    if (blockIdx.x >= tile_blocks)
        return;
    const CarrierReadJob j = jobs[blockIdx.x / tiles];
    const uint32_t i = (blockIdx.x % tiles) * XREAD_THREADS + threadIdx.x;
    if (i >= j.bins_end - j.bins_start)
        return;
    if constexpr (MODE == PREAD_AMPM)
        pair_ampm_element(j, i, out, units);
    else
        pair_csd_element(j, i, out);
}

template <uint32_t R, class Val>
__device__ __forceinline__ void pair_band_block(const CarrierReadJob *__restrict__ jobs, const BankRow u, const BankBands &bands, const Val &val,
                                                uint32_t row0, double *__restrict__ out)
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
                    out[((size_t)blockIdx.x * bands.n + b) * PREAD_BAND_ROWS + row0 + r] = sum;
            }
    }
}

template <uint32_t R, int MODE>
__global__ __launch_bounds__(BANK_BAND_THREADS) void pair_band_kernel(const CarrierReadJob *__restrict__ jobs, const BankRow *__restrict__ units,
                                                                      const PairUnit *__restrict__ punits, const BankBands bands,
                                                                      double *__restrict__ out)
{
    const uint32_t row0 = blockIdx.y * R;
    if constexpr (MODE == PREAD_AMPM)
        pair_band_block<R>(jobs, units[blockIdx.x], bands, PairAmPmVal{pair_split_of(punits[blockIdx.x]), row0}, row0, out);
    else
        pair_band_block<R>(jobs, units[blockIdx.x], bands, PairCsdVal{row0}, row0, out);
}

namespace {

// the grid of a stitch launch; false: too many workgroups
bool pair_grid(uint32_t n_jobs, uint32_t max_bins, bool rows, uint32_t record_units, uint32_t *tiles, uint32_t *tile_blocks, uint32_t *blocks)
{
    *tiles = rows ? (max_bins + XREAD_THREADS - 1) / XREAD_THREADS : 0;
    const uint64_t tb = (uint64_t)*tiles * n_jobs, all = tb + (record_units + XREAD_THREADS - 1) / XREAD_THREADS;
    if (all > 0x7FFFFFFFull)
        return false;
    *tile_blocks = (uint32_t)tb;
    *blocks = (uint32_t)all;
    return true;
}

} // namespace

hipError_t launch_pair_stitch_csd(const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const PairCsdOut &out, hipStream_t s)
{
    if (!out.any_row() || !n_jobs || !max_bins)
        return hipSuccess;
    uint32_t tiles, tile_blocks, blocks;
    if (!d_jobs || !pair_grid(n_jobs, max_bins, true, 0, &tiles, &tile_blocks, &blocks))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((pair_stitch_kernel<PREAD_CSD, PairCsdOut>), dim3(blocks), dim3(XREAD_THREADS), 0, s, d_jobs, tiles, tile_blocks, out,
                       (const PairUnit *)nullptr, 0u);
    return hipGetLastError();
}

hipError_t launch_pair_stitch_ampm(const CarrierReadJob *d_jobs, uint32_t n_jobs, uint32_t max_bins, const PairAmPmOut &out,
                                   const PairUnit *d_units, uint32_t n_units, hipStream_t s)
{
    const bool rows = out.any_row() && n_jobs && max_bins, records = out.carrier && n_units;
    if (!rows && !records)
        return hipSuccess;
    uint32_t tiles, tile_blocks, blocks;
    if ((rows && !d_jobs) || !d_units || !pair_grid(n_jobs, max_bins, rows, records ? n_units : 0, &tiles, &tile_blocks, &blocks))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((pair_stitch_kernel<PREAD_AMPM, PairAmPmOut>), dim3(blocks), dim3(XREAD_THREADS), 0, s, d_jobs, tiles, tile_blocks, out,
                       d_units, n_units);
    return hipGetLastError();
}

hipError_t launch_pair_band(int mode, const CarrierReadJob *d_jobs, const BankRow *d_units, const PairUnit *d_punits, uint32_t n_units,
                            const BankBands &bands, double *d_out, hipStream_t s)
{
    if (n_units == 0 || bands.n == 0)
        return hipSuccess;
    if (!d_jobs || !d_units || !d_out || bands.n > BANK_MAX_BANDS || (mode != PREAD_CSD && mode != PREAD_AMPM) || (mode == PREAD_AMPM && !d_punits))
        return hipErrorInvalidValue;
    constexpr uint32_t R = PREAD_BAND_KERNEL_ROWS;
    const dim3 grid(n_units, PREAD_BAND_ROWS / R), block(BANK_BAND_THREADS);
    if (mode == PREAD_AMPM)
        hipLaunchKernelGGL((pair_band_kernel<R, PREAD_AMPM>), grid, block, 0, s, d_jobs, d_units, d_punits, bands, d_out);
    else
        hipLaunchKernelGGL((pair_band_kernel<R, PREAD_CSD>), grid, block, 0, s, d_jobs, d_units, d_punits, bands, d_out);
    return hipGetLastError();
}

} // namespace psdk
