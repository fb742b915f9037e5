// cross.hip -- gfx950 kernels of the cross-spectral density cascade (psdc_cross_*, cross_runtime.cpp).
//
//   cross_kernel<N>    per segment of a (pair, stage): detrend each channel (src/psd.rs:75-113), window with the EWMA amplitude,
//                      transform, separate (cross_fft.h) and accumulate |X|^2, |Y|^2 and conj(X) Y over bins 0 ... N/2 into
//                      one partial row set per workgroup.  Two consecutive segments of ONE channel share a transform; the
//                      channels never share one (cross_fft.h says why).
//   cross_post_kernel  the round's epilogue: folds the partials into the f64 accumulators (g_total, src/psd.rs:218-233) in a
//                      fixed order and carries the stream tails into the other buffer.
// The /8 decimator is hbf_dec8_kernel (kernels.hip) through launch_dec, one job per channel.
#include "cross.h"
#include "cross_fft.h"

namespace psdk {

template <int N>
struct CrossCfg {
    using Plan = FftPlan<N>;
    static constexpr int E = Plan::E;
    static constexpr int TEAM = Plan::TEAM;
    static constexpr int BLOCK = TEAM > 128 ? TEAM : 128;
    static constexpr int TEAMS = BLOCK / TEAM;
    static constexpr int SPT = 2 * TEAMS; // segments per tile: one pair a team (fine tiles keep the workgroups of a launch even)
    static constexpr int WAVES = BLOCK / 64;
    static constexpr int H = N / 2 + 1;
    static constexpr int FRAME = LdsFrame<N>::SIZE;
    static_assert(E == 16, "cross kernel: sixteen elements a thread");
    static_assert(H <= FRAME, "partial rows reuse the frames' LDS");
};

__device__ __forceinline__ float cross_amp(const CrossJob &job, int step)
{
    const int m = step > job.is_m1 ? step : job.is_m1;
    const int na = job.nb - m;
    if (na <= 0)
        return 1.0f;
    return (float)exp2(0.5 * (double)na * job.log2_gamma);
}

template <int TEAM>
__device__ __forceinline__ void xteam_sync()
{
    if constexpr (TEAM <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int N, int P>
__device__ __forceinline__ void xfft_run(int t, cf *v, cf *frame, const cf *__restrict__ tw)
{
    using PI = PassInfo<N, P>;
    if constexpr (P == 0)
        xteam_sync<PI::TEAM>(); // the frame's previous readers (separation) are done
    xfft_pass<N, P>(t, v, frame, tw);
    xteam_sync<PI::TEAM>();
    if constexpr (!PI::LAST)
        xfft_run<N, P + 1>(t, v, frame, tw);
}

// Load, detrend, window one channel's segment pair (a = segment la, b = la + 1) into v, transform, and leave the spectrum of
// z = a + i b in natural order in `frame`.
template <int N>
__device__ __forceinline__ void cross_channel(const float *__restrict__ src, long long ofs_la, long long ofs_lb, bool act_a,
                                              bool act_b, int detrend, float ampa, float ampb, int t, int team, cf *frame,
                                              float *red, const float *__restrict__ win, const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using P0 = PassInfo<N, 0>;
    constexpr int E = Cfg::E, TEAM = Cfg::TEAM;
    float ra[E], rb[E];
#pragma unroll
    for (int i = 0; i < P0::NB; ++i)
#pragma unroll
        for (int m = 0; m < P0::R; ++m) {
            const int nidx = P0::elem(t, i, m);
            const float va = src[ofs_la + nidx], vb = src[ofs_lb + nidx];
            ra[i * P0::R + m] = act_a ? va : 0.0f;
            rb[i * P0::R + m] = act_b ? vb : 0.0f;
        }
    // detrend as welch_kernel: (x - o) - (m + n s)
    float oa = 0.0f, ob = 0.0f, ma = 0.0f, mb = 0.0f;
    slope2 sa = {0.0f, 0.0f}, sb = {0.0f, 0.0f};
    if (detrend == 1) { // Midpoint src/psd.rs:87-93
        const float va = src[ofs_la + N / 2], vb = src[ofs_lb + N / 2];
        oa = act_a ? va : 0.0f;
        ob = act_b ? vb : 0.0f;
    } else if (detrend == 2) { // Span :94-102
        const float a0 = src[ofs_la], a1 = src[ofs_la + N - 1], b0 = src[ofs_lb], b1 = src[ofs_lb + N - 1];
        if (act_a) {
            oa = a0;
            sa = span_slope(oa, a1, N);
        }
        if (act_b) {
            ob = b0;
            sb = span_slope(ob, b1, N);
        }
    } else if (detrend == 3) { // Mean :103-109: o = f32 mean, m = mean of x - o
        auto team_sum2 = [&](float &pa, float &pb) __attribute__((always_inline)) {
            constexpr int W = TEAM < 64 ? TEAM : 64;
#pragma unroll
            for (int o = W / 2; o > 0; o >>= 1) {
                pa += __shfl_xor(pa, o);
                pb += __shfl_xor(pb, o);
            }
            if constexpr (TEAM > 64) { // one team a workgroup: combine its wavefronts through LDS
                constexpr int WPT = TEAM / 64;
                const int w = threadIdx.x >> 6;
                if ((threadIdx.x & 63) == 0) {
                    red[2 * w] = pa;
                    red[2 * w + 1] = pb;
                }
                __syncthreads();
                pa = 0.0f;
                pb = 0.0f;
                for (int i = 0; i < WPT; ++i) {
                    pa += red[2 * (team * WPT + i)];
                    pb += red[2 * (team * WPT + i) + 1];
                }
                __syncthreads();
            }
        };
        float pa = 0.0f, pb = 0.0f;
#pragma unroll
        for (int s = 0; s < E; ++s) {
            pa += ra[s];
            pb += rb[s];
        }
        team_sum2(pa, pb);
        oa = pa / (float)N;
        ob = pb / (float)N;
        pa = 0.0f;
        pb = 0.0f;
#pragma unroll
        for (int s = 0; s < E; ++s) {
            pa += ra[s] - oa;
            pb += rb[s] - ob;
        }
        team_sum2(pa, pb);
        ma = pa / (float)N;
        mb = pb / (float)N;
    }
    cf v[E];
#pragma unroll
    for (int i = 0; i < P0::NB; ++i)
#pragma unroll
        for (int m = 0; m < P0::R; ++m) {
            const int s = i * P0::R + m;
            const int nidx = P0::elem(t, i, m);
            const float w = win[nidx];
            float a = ra[s], b = rb[s];
            if (detrend != 0) {
                a = fmaf(-(float)nidx, sa.lo, fmaf(-(float)nidx, sa.hi, a - oa)) - ma;
                b = fmaf(-(float)nidx, sb.lo, fmaf(-(float)nidx, sb.hi, b - ob)) - mb;
            }
            v[s].re = a * w * ampa;
            v[s].im = b * w * ampb;
        }
    xfft_run<N, 0>(t, v, frame, tw);
    store_natural<N>(t, v, frame);
}

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void cross_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                   const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using Bins = CrossBins<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, SPT = Cfg::SPT, H = Cfg::H, XB = Bins::XBINS;

    __shared__ cf frames[TEAMS * 2 * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    const int ji = job_of_unit(batch, (int)blockIdx.x, [](const CrossJob &j) { return j.block_begin; });
    const CrossJob &job = batch.jobs[ji];
    const int wb = blockIdx.x - job.block_begin;
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *fx = frames + team * 2 * Cfg::FRAME;
    cf *fy = fx + Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][4];
#pragma unroll
    for (int r = 0; r < XB; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            acc[r][c] = 0.0f;

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) {
        const int seg_lo = lt * SPT;
        const int seg_hi = min(job.nseg, seg_lo + SPT);
        const int npairs = (seg_hi - seg_lo + 1) >> 1;
        for (int p0 = 0; p0 < npairs; p0 += TEAMS) {
            const int la = seg_lo + 2 * (p0 + team);
            const bool act_a = la < seg_hi, act_b = la + 1 < seg_hi;
            // lanes without a segment read the job's first one (always inside the stream) and drop it
            const long long ofs_safe = job.seg0 * (long long)hop - job.src_base;
            const long long ofs_a = (job.seg0 + la) * (long long)hop - job.src_base;
            const long long ofs_la = act_a ? ofs_a : ofs_safe, ofs_lb = act_b ? ofs_a + hop : ofs_safe;
            float ampa = 1.0f, ampb = 1.0f;
            if (job.ewma) {
                ampa = cross_amp(job, job.step0 + la);
                ampb = cross_amp(job, job.step0 + la + 1);
            }
            cross_channel<N>(job.src[0], ofs_la, ofs_lb, act_a, act_b, detrend, ampa, ampb, t, team, fx, red, win, tw);
            cross_channel<N>(job.src[1], ofs_la, ofs_lb, act_a, act_b, detrend, ampa, ampb, t, team, fy, red, win, tw);
            xteam_sync<TEAM>();
#pragma unroll
            for (int r = 0; r < XB; ++r) {
                const int k = t + TEAM * r;
                if (k < H)
                    cross_bin<N>(k, fx, fy, act_b, acc[r]);
            }
        }
    }

    // combine the teams (fixed order) and write the workgroup's partial rows
    float *fq = reinterpret_cast<float *>(frames);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < XB; ++r) {
        const int k = t + TEAM * r;
        if (k < H)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                fq[(team * 4 + c) * H + k] = acc[r][c];
    }
    __syncthreads();
    float *out = job.partial + (size_t)wb * 4 * H;
    for (int e = threadIdx.x; e < 4 * H; e += Cfg::BLOCK) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < TEAMS; ++g)
            s += fq[g * 4 * H + e];
        out[e] = s;
    }
}

// fold: a workgroup takes FOLD_ELEMS consecutive elements of a job's partial rows; its FOLD_SLICES slices walk the partial list
// with stride FOLD_SLICES (f64 sums, workgroups in order) and are combined in slice order -- a fixed order: the same calls give
// the same bits
constexpr int FOLD_ELEMS = 32, FOLD_SLICES = 32, POST_THREADS = FOLD_ELEMS * FOLD_SLICES;

__global__ __launch_bounds__(POST_THREADS) void cross_post_kernel(const CrossPostBatch b)
{
    const int nfold = b.nfold * b.fold_xb;
    if ((int)blockIdx.x < nfold) {
        __shared__ double part[FOLD_SLICES][FOLD_ELEMS + 1];
        const CrossFoldJob &job = b.fold[blockIdx.x / b.fold_xb];
        const int lane = threadIdx.x % FOLD_ELEMS, slice = threadIdx.x / FOLD_ELEMS;
        const int e = (blockIdx.x % b.fold_xb) * FOLD_ELEMS + lane;
        const int rows = 4 * b.nbins;
        double s = 0.0;
        if (e < rows)
            for (int i = slice; i < job.nparts; i += FOLD_SLICES)
                s += (double)job.partial[(size_t)i * rows + e];
        part[slice][lane] = s;
        __syncthreads();
        if (slice == 0 && e < rows) {
            s = 0.0;
#pragma unroll
            for (int i = 0; i < FOLD_SLICES; ++i)
                s += part[i][lane];
            job.acc[e] = job.g_total * job.acc[e] + s;
        }
        return;
    }
    const int u = blockIdx.x - nfold; // tail workgroup -> its job (bisection over block_begin)
    int lo = 0, hi = b.ntail - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (u >= b.tail[mid].block_begin)
            lo = mid;
        else
            hi = mid - 1;
    }
    const CrossTailJob &tj = b.tail[lo];
    const long long i0 = (long long)(u - tj.block_begin) * CROSS_TAIL_CHUNK;
    const long long i1 = min(tj.count, i0 + CROSS_TAIL_CHUNK);
    for (long long i = i0 + threadIdx.x; i < i1; i += POST_THREADS)
        tj.dst[i] = tj.src[i];
}

int cross_fold_blocks(int nbins) { return (4 * nbins + FOLD_ELEMS - 1) / FOLD_ELEMS; }

int cross_block_threads(int n)
{
    switch (n) {
#define PSDK_CASE(NN) \
    case NN:          \
        return CrossCfg<NN>::BLOCK;
        PSDK_CASE(64)
        PSDK_CASE(128)
        PSDK_CASE(256)
        PSDK_CASE(512)
        PSDK_CASE(1024)
        PSDK_CASE(2048)
        PSDK_CASE(4096)
#undef PSDK_CASE
    default:
        return 0;
    }
}

bool cross_supported(int n) { return n >= 64 && n <= 4096 && (n & (n - 1)) == 0; }

int cross_segments_per_tile(int n)
{
    switch (n) {
#define PSDK_CASE(NN) \
    case NN:          \
        return CrossCfg<NN>::SPT;
        PSDK_CASE(64)
        PSDK_CASE(128)
        PSDK_CASE(256)
        PSDK_CASE(512)
        PSDK_CASE(1024)
        PSDK_CASE(2048)
        PSDK_CASE(4096)
#undef PSDK_CASE
    default:
        return 0;
    }
}

hipError_t launch_cross(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    switch (n) {
#define PSDK_CASE(NN)                                                                                                   \
    case NN:                                                                                                            \
        hipLaunchKernelGGL(cross_kernel<NN>, dim3(b.nblocks), dim3(CrossCfg<NN>::BLOCK), 0, s, b, win, tw);        \
        break;
        PSDK_CASE(64)
        PSDK_CASE(128)
        PSDK_CASE(256)
        PSDK_CASE(512)
        PSDK_CASE(1024)
        PSDK_CASE(2048)
        PSDK_CASE(4096)
#undef PSDK_CASE
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_cross_post(const CrossPostBatch &b, hipStream_t s)
{
    const int grid = b.nfold * b.fold_xb + b.tail_blocks;
    if (grid <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(cross_post_kernel, dim3(grid), dim3(POST_THREADS), 0, s, b);
    return hipGetLastError();
}

} // namespace psdk
