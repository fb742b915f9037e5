// bank_var.hip -- the kernel of the Var read-out (psdcv_*; include/psdcascade_var.h, arithmetic and order in bank_var.h).
//
//   bank_var_kernel  one workgroup of 256 threads a (row, tile of VAR_TAU_TILE = 4 taus); workgroup blockIdx.x serves tile
//                    blockIdx.x % tiles of row blockIdx.x / tiles (rows along x with the tiles: no 65535 limit on the rows).
//                    1. the limits clip / tau in f32 and the limit search (var_limit_walk), its minimum over the workgroup by a
//                       shuffle tree and LDS: E per descriptor and tau;
//                    2. rounds of 256 elements while one below the largest E is left (the trip count is uniform over the
//                       workgroup): thread t computes sin and w once a tau and a[e] of up to four descriptors, takes a[e-1] and
//                       f[e-1] from the lane below by one shuffle each, and adds its trapezoid into one of its 16 f64 sums;
//                    3. the band kernel's reduction: the shuffle tree in the wavefront, then the four wavefronts in order from
//                       LDS.  No atomics: the order is a function of the row's length alone.
//                    Lane 0 has no lane below.  Its a[e-1] is what lane 63 of the wavefront before computed in the same round (for
//                    wavefront 0: what lane 63 of wavefront 3 computed in the round before), and it is handed over through LDS
//                    behind the round's one barrier -- three buffers in turn, so that the writer of round i + 1 never meets the
//                    reader of round i.  A recomputation in lane 0 alone would give the same bits, but a branch that one lane takes
//                    costs the wavefront a second pass through the sine: the hand-over costs no sine at all.
// Compute-bound: one f64 sine a (element, tau), two powi a descriptor.  Built with -ffp-contract=off, as bank_readout.hip.
#include <hip/hip_runtime.h>

#include "bank_var.h"

namespace psdk {

namespace {

constexpr uint32_t WAVES = VAR_THREADS / BANK_WAVE;

template <class Src>
__device__ __forceinline__ void var_block(Src src, const VarDesc *__restrict__ d_vars, uint32_t nv, const float *__restrict__ taus, uint32_t nt,
                                          uint32_t tile, double *__restrict__ out)
{
    __shared__ uint32_t s_first[WAVES][VAR_MAX_VARS][VAR_TAU_TILE];
    __shared__ double s_edge_a[3][WAVES][VAR_TAU_TILE][VAR_MAX_VARS];
    __shared__ float s_edge_f[3][WAVES];
    __shared__ double s_part[VAR_MAX_VARS][VAR_TAU_TILE][WAVES];
    const uint32_t t = threadIdx.x, lane = t % BANK_WAVE, wave = t / BANK_WAVE, L = src.len, j0 = tile * VAR_TAU_TILE;

    VarDesc vars[VAR_MAX_VARS];
#pragma unroll
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
        vars[v] = d_vars[v < nv ? v : 0];
    float tau[VAR_TAU_TILE];
#pragma unroll
    for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
        tau[j] = taus[j0 + j < nt ? j0 + j : nt - 1]; // (a tile at the end repeats the last tau; nothing of it is stored)

    // 1. E[v][j]
    uint32_t E[VAR_MAX_VARS][VAR_TAU_TILE];
    {
        float lim[VAR_MAX_VARS][VAR_TAU_TILE];
#pragma unroll
        for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#pragma unroll
            for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
                lim[v][j] = vars[v].clip / tau[j];
                E[v][j] = L;
            }
        var_limit_walk(src, t, VAR_THREADS, vars, nv, lim, E);
#pragma unroll
        for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#pragma unroll
            for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
                uint32_t m = E[v][j];
#pragma unroll
                for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
                    m = min(m, (uint32_t)__shfl_down((int)m, off, BANK_WAVE));
                if (lane == 0)
                    s_first[wave][v][j] = m;
            }
        __syncthreads();
    }
    uint32_t e_max = 0;
#pragma unroll
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#pragma unroll
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
            uint32_t m = s_first[0][v][j];
#pragma unroll
            for (uint32_t w = 1; w < WAVES; ++w)
                m = min(m, s_first[w][v][j]);
            E[v][j] = v < nv ? m : 0;
            if (v < nv && m > vars[v].dc_cut)
                e_max = max(e_max, m);
        }

    // 2. the rounds
    double acc[VAR_MAX_VARS][VAR_TAU_TILE];
#pragma unroll
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#pragma unroll
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
            acc[v][j] = 0.0;
    uint32_t buf = 0; // the hand-over buffer of this round; the round before wrote (buf + 2) % 3
    for (uint32_t base = 0; base < e_max; base += VAR_THREADS) {
        const uint32_t e = base + t;
        float p = 0.0f, f = 0.0f;
        if (e < L)
            src.at(e, &p, &f);
        double a[VAR_TAU_TILE][VAR_MAX_VARS];
#pragma unroll
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
            var_terms(p, f, tau[j], vars, nv, a[j]);
        if (lane == BANK_WAVE - 1) {
#pragma unroll
            for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
#pragma unroll
                for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
                    s_edge_a[buf][wave][j][v] = a[j][v];
            s_edge_f[buf][wave] = f;
        }
        __syncthreads();
        const uint32_t eb = wave ? buf : (buf + 2) % 3, ew = wave ? wave - 1 : WAVES - 1; // where lane 0 finds element e - 1
        float f1 = __shfl_up(f, 1, BANK_WAVE);
        if (lane == 0)
            f1 = s_edge_f[eb][ew]; // (round 0 of wavefront 0 reads what nobody wrote: e = 0 has no element before and uses none)
#pragma unroll
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j)
#pragma unroll
            for (uint32_t v = 0; v < VAR_MAX_VARS; ++v) {
                double a1 = __shfl_up(a[j][v], 1, BANK_WAVE);
                if (lane == 0)
                    a1 = s_edge_a[eb][ew][j][v];
                acc[v][j] += var_trapezoid(a[j][v], a1, f, f1, e, vars[v].dc_cut, E[v][j]);
            }
        buf = buf == 2 ? 0 : buf + 1;
    }

    // 3. the sums
#pragma unroll
    for (uint32_t v = 0; v < VAR_MAX_VARS; ++v)
#pragma unroll
        for (uint32_t j = 0; j < VAR_TAU_TILE; ++j) {
            double x = acc[v][j];
#pragma unroll
            for (uint32_t off = BANK_WAVE / 2; off; off >>= 1)
                x += __shfl_down(x, off, BANK_WAVE);
            if (lane == 0)
                s_part[v][j][wave] = x;
        }
    __syncthreads();
    if (t < VAR_MAX_VARS * VAR_TAU_TILE) {
        const uint32_t v = t / VAR_TAU_TILE, j = t % VAR_TAU_TILE;
        double sum = s_part[v][j][0];
#pragma unroll
        for (uint32_t w = 1; w < WAVES; ++w)
            sum += s_part[v][j][w];
        if (v < nv && j0 + j < nt)
            out[(size_t)v * nt + j0 + j] = sum;
    }
}

} // namespace

__global__ __launch_bounds__(VAR_THREADS) void bank_var_kernel(const BankJob *__restrict__ jobs, const BankRow *__restrict__ rows,
                                                               const VarRow *__restrict__ vrows, const VarDesc *__restrict__ vars, uint32_t nv,
                                                               const float *__restrict__ taus, uint32_t nt, uint32_t tiles,
                                                               double *__restrict__ out)
{
    const uint32_t row = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    double *o = out + (size_t)row * nv * nt;
    if (vrows) {
        const VarRow r = vrows[row];
        var_block(VarRowSrc(r.psd, r.freq, r.len), vars, nv, taus, nt, tile, o);
    } else {
        const BankRow r = rows[row];
        var_block(VarJobSrc(jobs + r.job0, r.njobs, r.len), vars, nv, taus, nt, tile, o);
    }
}

hipError_t launch_bank_var(const BankJob *d_jobs, const BankRow *d_rows, const VarRow *d_vrows, uint32_t n_rows, const VarDesc *d_vars,
                           uint32_t nv, const float *d_taus, uint32_t nt, double *d_out, hipStream_t s)
{
    if (n_rows == 0)
        return hipSuccess;
    if (!d_vars || !d_taus || !d_out || nv == 0 || nv > VAR_MAX_VARS || nt == 0 || nt > VAR_MAX_TAUS || n_rows > BANK_MAX_ROWS ||
        (d_vrows ? (d_jobs || d_rows) : (!d_jobs || !d_rows)))
        return hipErrorInvalidValue;
    const uint32_t tiles = (nt + VAR_TAU_TILE - 1) / VAR_TAU_TILE; // (at most 1024 tiles x 65536 rows = 2^26 workgroups)
    hipLaunchKernelGGL(bank_var_kernel, dim3(n_rows * tiles), dim3(VAR_THREADS), 0, s, d_jobs, d_rows, d_vrows, d_vars, nv, d_taus, nt, tiles,
                       d_out);
    return hipGetLastError();
}

} // namespace psdk
