// csm.hip -- gfx950 kernel of the cross-spectral matrix cascade (psdc_csm_*, cross_runtime.cpp).
//
//   csm_kernel<N, M>   per segment of a (group, stage): every one of the M channels is detrended, windowed and transformed ONCE
//                      (cross_channel.h: two consecutive segments of one channel share a transform), then every product
//                      conj(X_a) X_b, a <= b, of bins 0 ... N/2 is accumulated (csm_fft.h) into one partial row set per
//                      workgroup, M x M real rows.
//
// Where the rows live: in registers, but of the whole workgroup and not of a team.  A workgroup is BLOCK = 256 threads: TEAMS
// transform teams, each with its own segment pair and M natural-order frames in LDS.  Once the frames stand, the SAME threads
// regroup for the products: thread pt of a product group owns bins pt + GS r and walks the frames of the group's teams in a
// fixed order.  A thread so keeps XB M^2 accumulators with XB = ceil((N/2 + 1) / 256) for N >= 512 (3 at N = 1024 where a
// team-owned layout as cross_kernel's needs 9): 48 registers at N = 1024 and M = 4 in place of 144, no accumulator in LDS, no
// atomics, and no combine across teams for N >= 512.  The LDS holds frames only: M x 8 KiB a wavefront whatever N, 128 KiB at
// M = 4 -- the same one wavefront a SIMD the transform's registers allow cross_kernel.  The price is two workgroup barriers a
// tile (frames complete / frames free) in place of the pair kernel's wavefront-local ones.
// The fold, the stream tails and the decimator are the pair object's kernels (cross.hip, kernels.hip).
#include "csm.h"
#include "segment_kernel.h"
#include "csm_fft.h"

namespace psdk {

template <int N, int M>
__global__ __launch_bounds__((CsmShape<N, M>::BLOCK)) void csm_kernel(const CsmBatch batch, const float *__restrict__ win,
                                                                    const cf *__restrict__ tw)
{
    using S = CsmShape<N, M>;
    constexpr int TEAM = S::TEAM, TEAMS = S::TEAMS, SPT = S::SPT, H = S::H, XB = S::XB, GS = S::GS, PG = S::PG, ROWS = S::ROWS,
                  FRAME = S::FRAME, BLOCK = S::BLOCK;

    __shared__ cf frames[TEAMS * M * FRAME];
    __shared__ float red[(BLOCK / 64) * 2];

    int wb;
    const CsmJob &job = seg_job(batch, wb);
    const int team = threadIdx.x / TEAM;
    const int t = threadIdx.x % TEAM;
    const int pg = threadIdx.x / GS;
    const int pt = threadIdx.x % GS;
    cf *fteam = frames + team * M * FRAME;
    const int hop = batch.hop;
    const int detrend = batch.detrend;

    float acc[XB][ROWS];
    zero_rows(acc);

    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) { // a tile: one segment pair a team
        const int seg_lo = lt * SPT;
        const int seg_hi = min(job.nseg, seg_lo + SPT);
        const SegPair sp = seg_pair(job, hop, seg_hi, seg_lo + 2 * team);
        float ampa = 1.0f, ampb = 1.0f;
        if (job.ewma) {
            ampa = cross_amp(job, job.step0 + sp.seg);
            ampb = cross_amp(job, job.step0 + sp.seg + 1);
        }
#pragma unroll
        for (int c = 0; c < M; ++c)
            cross_channel<N>(job.src[c], sp.ofs_a, sp.ofs_b, sp.act_a, sp.act_b, detrend, ampa, ampb, t, team, fteam + c * FRAME, red,
                             win, tw);
        __syncthreads(); // every team's frames stand
        for (int g = pg; g < TEAMS; g += PG) { // fixed order: the same calls give the same bits
            const int lg = seg_lo + 2 * g;
            if (lg >= seg_hi)
                break;
            const bool b_live = lg + 1 < seg_hi;
            const cf *fg = frames + g * M * FRAME;
#pragma unroll
            for (int r = 0; r < XB; ++r) {
                const int k = pt + GS * r;
                if (k < H)
                    csm_bin<N, M>(k, fg, FRAME, b_live, acc[r]);
            }
        }
        __syncthreads(); // the frames are free for the next tile's transforms
    }

    float *out = job.partial + (size_t)wb * ROWS * H;
    if constexpr (PG == 1) {
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = pt + GS * r;
            if (k < H)
#pragma unroll
                for (int c = 0; c < ROWS; ++c)
                    out[c * H + k] = acc[r][c];
        }
    } else { // combine the product groups (fixed order) through the frames' LDS, as the other kernels combine their teams
        seg_combine<OwnedCombine<H, ROWS, ROWS, PG, GS>, BLOCK>(frames, pg, pt, acc, out);
    }
}

// every (n, m) the object runs.  n = 4096 with m = 4 is left out: one team a workgroup leaves a thread 9 x 16 = 144 accumulators,
// and beside the transform that compiles to 256 + 256 registers and 132 bytes of scratch a lane
#define PSDK_CSM_CASES(X) \
    X(64, 2) X(64, 3) X(64, 4) X(128, 2) X(128, 3) X(128, 4) X(256, 2) X(256, 3) X(256, 4) X(512, 2) X(512, 3) X(512, 4) \
    X(1024, 2) X(1024, 3) X(1024, 4) X(2048, 2) X(2048, 3) X(2048, 4) X(4096, 2) X(4096, 3)

bool csm_supported(int n, int m)
{
#define X(NN, MM)             \
    if (n == NN && m == MM) \
        return true;
    PSDK_CSM_CASES(X)
#undef X
    return false;
}

int csm_segments_per_tile(int n, int m)
{
#define X(NN, MM)             \
    if (n == NN && m == MM) \
        return CsmShape<NN, MM>::SPT;
    PSDK_CSM_CASES(X)
#undef X
    return 0;
}

int csm_block_threads(int n, int m)
{
#define X(NN, MM)             \
    if (n == NN && m == MM) \
        return CsmShape<NN, MM>::BLOCK;
    PSDK_CSM_CASES(X)
#undef X
    return 0;
}

hipError_t launch_csm(int n, int m, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (b.nblocks <= 0)
        return hipSuccess;
#define X(NN, MM)                                                                                                     \
    if (n == NN && m == MM) {                                                                                         \
        hipLaunchKernelGGL((csm_kernel<NN, MM>), dim3(b.nblocks), dim3(CsmShape<NN, MM>::BLOCK), 0, s, b, win, tw); \
        return hipGetLastError();                                                                                     \
    }
    PSDK_CSM_CASES(X)
#undef X
    return hipErrorInvalidValue;
}

} // namespace psdk
