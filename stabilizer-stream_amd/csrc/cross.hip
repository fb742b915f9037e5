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
#include "segment_kernel.h"

namespace psdk {

template <int N>
__global__ __launch_bounds__(CrossCfg<N>::BLOCK) void cross_kernel(const CrossBatch batch, const float *__restrict__ win,
                                                                   const cf *__restrict__ tw)
{
    using Cfg = CrossCfg<N>;
    using Bins = CrossBins<N>;
    constexpr int TEAM = Cfg::TEAM, TEAMS = Cfg::TEAMS, SPT = Cfg::SPT, H = Cfg::H, XB = Bins::XBINS;

    __shared__ cf frames[TEAMS * 2 * Cfg::FRAME];
    __shared__ float red[Cfg::WAVES * 2];

    int wb;
    const CrossJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    cf *fx = frames + team * 2 * Cfg::FRAME;
    cf *fy = fx + Cfg::FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][4];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) {
        const int seg_lo = lt * SPT;
        const int seg_hi = min(job.nseg, seg_lo + SPT);
        const int npairs = (seg_hi - seg_lo + 1) >> 1;
        // This kernel keeps its own spelling of seg_pair and of OwnedCombine<H, 4, 4, TEAMS, TEAM> (segment_kernel.h; the host
        // check walks that layout as "cross").  Its speed follows its register allocation, at the limit of one wavefront a SIMD: with
        // the shared functions, or without the one-turn p0 loop, it computed the same bits 18 ... 24 % slower at N = 1024 ... 4096
        // (profiles/segment_skeleton_probe.json).
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
        const int rows = b.nrows * b.nbins;
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
            if (job.fresh)
                job.acc[e] = s;
            else
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

int cross_fold_blocks(int nrows, int nbins) { return (nrows * nbins + FOLD_ELEMS - 1) / FOLD_ELEMS; }

int cross_block_threads(int n) { return seg_supported(n) ? seg_block(n) : 0; }

bool cross_supported(int n) { return seg_supported(n); }

int cross_segments_per_tile(int n) { return seg_supported(n) ? seg_spt(n) : 0; }

hipError_t launch_cross(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    return seg_launch(n, b, win, tw, s, [](auto N) { return cross_kernel<decltype(N)::value>; });
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
