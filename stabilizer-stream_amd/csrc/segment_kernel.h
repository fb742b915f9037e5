// segment_kernel.h -- the skeleton the eight segment kernels share (cross, sk, zoom, zoom_sk, zoom_ampm, zoom_cross,
// zoom_ampm_cross, csm): which job a workgroup serves, which segment a team reads in a tile, and how the teams' accumulators are
// combined through the frames' LDS into the workgroup's partial rows.  A kernel keeps what is its own -- its LDS, its
// cross_channel call(s) and its per-bin accumulation -- and calls these in between.  (cross_kernel spells seg_pair and its
// 4-of-4 OwnedCombine out: cross.hip says why.  Changing a function here moves the register allocation of seven kernels that
// run one wavefront a SIMD: time them against the parent)
// The index arithmetic is PSDK_HD: tests/host/segment_kernel_check.cpp walks the tile loops and drives every thread through both
// phases of a combine on the CPU.  Barriers, blockIdx and the launch are in the device wrappers at the end.
#pragma once
#include <type_traits>

#include "cross_channel.h"
#ifdef __HIPCC__
#include "kernels.h" // job_of_unit
#endif

namespace psdk {

// ---- tile addressing -----------------------------------------------------------------------------------------------------------
// Offsets are into job.src[c]; seg is the (first) segment's index in the job: its EWMA weight is that of step job.step0 + seg
// (cross_amp, sk_weight).  A lane without a segment reads the job's first one (always inside the stream) and drops it.

// pair tile (cross, sk, csm): a team takes the segments la and la + 1 of a tile that ends before seg_hi
struct SegPair {
    long long ofs_a, ofs_b;
    bool act_a, act_b;
    int seg; // la; segment b is seg + 1
};
template <class Job>
PSDK_HD SegPair seg_pair(const Job &job, int hop, int seg_hi, int la)
{
    const bool act_a = la < seg_hi, act_b = la + 1 < seg_hi;
    const long long ofs_safe = job.seg0 * (long long)hop - job.src_base;
    const long long ofs = (job.seg0 + la) * (long long)hop - job.src_base;
    return {act_a ? ofs : ofs_safe, act_b ? ofs + hop : ofs_safe, act_a, act_b, la};
}

// one segment a team (the zoom kernels): tile lt gives team `team` the segment lt TEAMS + team
struct OneSeg {
    long long ofs;
    bool act;
    int seg;
};
template <int TEAMS, class Job>
PSDK_HD OneSeg one_seg(const Job &job, int hop, int lt, int team)
{
    const int seg = lt * TEAMS + team;
    const bool act = seg < job.nseg;
    return {(job.seg0 + (act ? seg : 0)) * (long long)hop - job.src_base, act, seg};
}

template <int A, int B>
PSDK_HD void zero_rows(float (&acc)[A][B])
{
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b)
            acc[a][b] = 0.0f;
}

// ---- the two-sided rows of the zoom kernels --------------------------------------------------------------------------------------
// Row r of a partial (and of a stage's accumulators) is value r >> 1 of a bin; even rows (upper) show transform bin k at index
// k = 0 ... N/2, odd rows (lower) bin (N - k) mod N.
PSDK_HD int two_sided_value(int row) { return row >> 1; }
template <int N>
PSDK_HD int two_sided_bin(int row, int k)
{
    return (row & 1) ? (N - k) & (N - 1) : k;
}

// ---- combine: the groups' accumulators through LDS, summed in ascending group order, one f32 sum an element ------------------------
// Both forms work in turns of as many rows as the LDS holds.  Turn p is two phases with a workgroup barrier in front of each:
// every thread stores its accumulators of the turn, then partial element e of the turn is summed over the groups.

// Owned bins: thread pt of group g holds acc[r][row] of bin k = pt + GS r <= H - 1, all ROWS rows; TURN rows go a turn, group g's
// row c of the turn at fq[(g TURN + c) H + k].  (The groups are the teams, or csm's product groups.)
template <int H, int ROWS, int TURN, int GROUPS, int GS>
struct OwnedCombine {
    static_assert(ROWS % TURN == 0, "whole turns");
    static constexpr int XB = (H + GS - 1) / GS, TURNS = ROWS / TURN, ELEMS = TURN * H, LDS_FLOATS = GROUPS * ELEMS;

    static PSDK_HD void store(float *fq, int g, int pt, int p, const float (&acc)[XB][ROWS])
    {
#pragma unroll
        for (int r = 0; r < XB; ++r) {
            const int k = pt + GS * r;
            if (k < H)
#pragma unroll
                for (int c = 0; c < TURN; ++c)
                    fq[g * ELEMS + (c * H + k)] = acc[r][TURN * p + c]; // (one base a thread, constants beside it)
        }
    }
    // element e < ELEMS of turn p: its sum, and where in the partial it goes
    static PSDK_HD int sum(const float *fq, int p, int e, float &s)
    {
        s = 0.0f;
#pragma unroll
        for (int g = 0; g < GROUPS; ++g)
            s += fq[g * ELEMS + e];
        return TURN * p * H + e;
    }
};

// Slot order: thread t of a team holds acc[q][s], value q of transform bin freq_of_slot<N>(t, s), all N bins; V values go a turn,
// team g's value j of the turn at fq[(g V + j) N + bin], and leave as the two-sided rows 2 V p ... 2 V p + 2 V - 1.
template <int N, int Q, int V>
struct SlotCombine {
    static_assert(Q % V == 0, "whole turns");
    using Cfg = CrossCfg<N>;
    static constexpr int E = Cfg::E, H = Cfg::H, TEAMS = Cfg::TEAMS, TURNS = Q / V, ELEMS = 2 * V * H, LDS_FLOATS = TEAMS * V * N;

    static PSDK_HD void store(float *fq, int team, int t, int p, const float (&acc)[Q][E])
    {
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int s = 0; s < E; ++s)
                fq[(team * V + j) * N + freq_of_slot<N>(t, s)] = acc[V * p + j][s];
    }
    static PSDK_HD int sum(const float *fq, int p, int e, float &s)
    {
        const int row = 2 * V * p + e / H, i = e % H;
        const int k = two_sided_bin<N>(row, i), j = two_sided_value(row) - V * p;
        s = 0.0f;
#pragma unroll
        for (int g = 0; g < TEAMS; ++g)
            s += fq[(g * V + j) * N + k];
        return row * H + i;
    }
};

#ifdef __HIPCC__
// ---- device wrappers ---------------------------------------------------------------------------------------------------------------

// the job of this workgroup, and in wb its index among the job's workgroups (CrossBatch and CsmBatch)
template <class Batch>
__device__ __forceinline__ const auto &seg_job(const Batch &batch, int &wb)
{
    const auto &job = batch.jobs[job_of_unit(batch, (int)blockIdx.x, [](const auto &j) { return j.block_begin; })];
    wb = blockIdx.x - job.block_begin;
    return job;
}

// all turns of a combine C: `lds` is the frames' LDS (C::LDS_FLOATS floats of it are used), (g, pt) the thread's group and place
// in it, out the workgroup's partial rows
template <class C, int BLOCK, class Acc>
__device__ __forceinline__ void seg_combine(void *lds, int g, int pt, const Acc &acc, float *out)
{
    float *fq = reinterpret_cast<float *>(lds);
#pragma unroll
    for (int p = 0; p < C::TURNS; ++p) {
        __syncthreads();
        C::store(fq, g, pt, p, acc);
        __syncthreads();
        for (int e = threadIdx.x; e < C::ELEMS; e += BLOCK) {
            float s;
            const int at = C::sum(fq, p, e, s);
            out[at] = s;
        }
    }
}
template <int N, int ROWS, int TURN, class Acc>
__device__ __forceinline__ void combine_owned(void *lds, int team, int t, const Acc &acc, float *out)
{
    using Cfg = CrossCfg<N>;
    seg_combine<OwnedCombine<Cfg::H, ROWS, TURN, Cfg::TEAMS, Cfg::TEAM>, Cfg::BLOCK>(lds, team, t, acc, out);
}
template <int N, int Q, int V, class Acc>
__device__ __forceinline__ void combine_slots(void *lds, int team, int t, const Acc &acc, float *out)
{
    seg_combine<SlotCombine<N, Q, V>, CrossCfg<N>::BLOCK>(lds, team, t, acc, out);
}

// launch kernel_of(N)<N> on b.nblocks workgroups of CrossCfg<N>::BLOCK threads, n one of the seven sizes:
//     return seg_launch(n, b, win, tw, s, [](auto N) { return cross_kernel<decltype(N)::value>; });
template <int N>
using SegSize = std::integral_constant<int, N>;
template <class Batch, class KernelOf>
hipError_t seg_launch(int n, const Batch &b, const float *win, const cf *tw, hipStream_t s, KernelOf kernel_of)
{
    if (b.nblocks <= 0)
        return hipSuccess;
    void (*k)(Batch, const float *, const cf *);
    switch (n) {
    case 64: k = kernel_of(SegSize<64>{}); break;
    case 128: k = kernel_of(SegSize<128>{}); break;
    case 256: k = kernel_of(SegSize<256>{}); break;
    case 512: k = kernel_of(SegSize<512>{}); break;
    case 1024: k = kernel_of(SegSize<1024>{}); break;
    case 2048: k = kernel_of(SegSize<2048>{}); break;
    case 4096: k = kernel_of(SegSize<4096>{}); break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3(b.nblocks), dim3(seg_block(n)), 0, s, b, win, tw);
    return hipGetLastError();
}
#endif // __HIPCC__

} // namespace psdk
