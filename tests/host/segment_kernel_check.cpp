// Host check of stabilizer-stream_amd/csrc/segment_kernel.h: the skeleton the eight segment kernels share, off the GPU.
//
// Tile addressing.  For every N = 64 ... 4096 in the shape of the team kernels (CrossCfg<N>: 32 ... 1 teams), and for every
// (N, M) of csm_kernel in its own shape (CsmShape<N, M>: up to 64 teams), nseg in {1, 2, SPT - 1, SPT, SPT + 1, 3 SPT + 1} and
// nblocks in {1, 2, ntiles}, every (workgroup, tile, team) is walked as the kernels' loops walk them, through seg_pair (cross, sk,
// csm) and through one_seg (the zoom kernels).  The segment a lane reads is taken from its OFFSET, not from
// the loop indices: every segment of the job must come exactly once, at (seg0 + j) hop - src_base, with the EWMA step step0 + j;
// a lane without a segment must read N samples that start inside the job's first segment and end inside the job's span.
// csm's product loop is walked beside it, thread by thread: every bin 0 ... N/2 of every team that holds a segment must be taken
// by exactly one thread, with b_live as seg_pair says, and where there is one product group every partial element is stored once.
//
// Combine.  For each kernel's parameter set at every size (the kernels' own constants; csm at every shape with more than one
// product group) every
// thread's accumulators hold a value that is a function of (group, row, bin) alone -- random mantissas over 24 binades, so an f32
// sum depends on its order -- and accumulators of bins a thread does not own hold NaN.  Turn by turn, on an array of the size of
// the kernel's LDS with guards around it and NaN inside it, every thread runs the store phase, then every partial element the sum
// phase: each [row][k], k <= N/2, must be written exactly once with the groups' values of that (row, bin) summed in ascending
// group order, the two-sided rows reading bin (N - k) mod N in their odd rows; the guards must stay as they were.
//
// `--shapes` prints the workgroup shape of every instance instead (tests/test_segment_instances_host.py holds its table to it).
// -DSEGK_SEED=1 / 2 seeds one mistake into the way THIS program calls the header (1: a lane without a segment takes its offset
// from the previous job's base; 2: the sum phase is always handed turn 0) and the program must then fail: tests/test_segment_kernel_host.py
// builds both, beside the plain build and one with -fsanitize=address,undefined.
// Build: g++ -O2 -std=c++17 -I<csrc> segment_kernel_check.cpp
#include "segment_kernel.h"

#include "csm_fft.h"
#include "sk_fft.h"
#include "zoom_ampm_cross_fft.h"
#include "zoom_ampm_fft.h"
#include "zoom_cross_fft.h"
#include "zoom_sk_fft.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace psdk;

#ifndef SEGK_SEED
#define SEGK_SEED 0
#endif

static int g_fail = 0;
static void fail(const char *fmt, ...)
{
    if (++g_fail > 20)
        return;
    va_list ap;
    va_start(ap, fmt);
    printf("FAIL ");
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
}

// ---- tile addressing -----------------------------------------------------------------------------------------------------------
struct Job { // the fields of CrossJob / CsmJob the addressing reads
    long long src_base, seg0;
    int nseg, ntiles, nblocks, step0;
};

struct Walk {
    const Job &job;
    int n, hop;
    std::vector<int> seen;
    long long lanes = 0, idle = 0;
    Walk(const Job &j, int n_, int hop_) : job(j), n(n_), hop(hop_), seen(j.nseg, 0) {}
    long long first() const { return job.seg0 * hop - job.src_base; }
    void lane(const char *form, long long ofs, bool act, int step)
    {
        ++lanes;
        if (!act) {
            ++idle;
            // N samples from ofs: they start inside the first segment and end inside the job's span
            if (ofs < first() || ofs >= first() + n || ofs + n > first() + (long long)(job.nseg - 1) * hop + n)
                fail("%s N=%d nseg=%d nblocks=%d: a lane without a segment reads at %lld, the job's first segment is at %lld", form, n,
                     job.nseg, job.nblocks, ofs, first());
            return;
        }
        const long long abs0 = ofs + job.src_base;
        const long long j = abs0 / hop - job.seg0;
        if (abs0 % hop != 0 || j < 0 || j >= job.nseg) {
            fail("%s N=%d nseg=%d nblocks=%d: offset %lld is no segment of the job", form, n, job.nseg, job.nblocks, ofs);
            return;
        }
        ++seen[j];
        if (step != job.step0 + (int)j)
            fail("%s N=%d nseg=%d: segment %lld takes the EWMA step %d, not %d", form, n, job.nseg, j, step, job.step0 + (int)j);
    }
    void done(const char *form)
    {
        for (int j = 0; j < job.nseg; ++j)
            if (seen[j] != 1)
                fail("%s N=%d nseg=%d nblocks=%d: segment %d taken %d times", form, n, job.nseg, job.nblocks, j, seen[j]);
    }
};

// TEAMS teams a workgroup, SPT segments a pair tile; zoom: walk the one-segment form beside the pair form (the team kernels' shape)
template <int N, int TEAMS, int SPT>
static void walk_addressing(bool zoom, long long &lanes, long long &idle)
{
    const int hop = N / 2 + 3; // no multiple of anything
    const Job prev = {1000, 40, 9, 1, 1, 3};
    for (int nseg : {1, 2, SPT - 1, SPT, SPT + 1, 3 * SPT + 1}) {
        if (nseg < 1)
            continue;
        for (int form = 0; form < (zoom ? 2 : 1); ++form) {
            const int per_tile = form == 0 ? SPT : TEAMS;
            const int ntiles = (nseg + per_tile - 1) / per_tile;
            for (int nblocks : {1, 2, ntiles}) {
                if (nblocks > ntiles)
                    continue;
                const Job job = {777LL * hop - 5, 777, nseg, ntiles, nblocks, 11}; // the first segment 5 samples into the buffer
                Job wrong = job;
                wrong.src_base = prev.src_base;
                Walk w(job, N, hop);
                const char *name = form == 0 ? "seg_pair" : "one_seg";
                for (int wb = 0; wb < job.nblocks; ++wb)
                    for (int lt = wb; lt < job.ntiles; lt += job.nblocks) // the kernels' tile loop
                        for (int team = 0; team < TEAMS; ++team) {
                            if (form == 0) {
                                const int seg_lo = lt * SPT;
                                const int seg_hi = std::min(job.nseg, seg_lo + SPT);
                                SegPair sp = seg_pair(job, hop, seg_hi, seg_lo + 2 * team);
#if SEGK_SEED == 1
                                const SegPair bad = seg_pair(wrong, hop, seg_hi, seg_lo + 2 * team);
                                sp.ofs_a = sp.act_a ? sp.ofs_a : bad.ofs_a;
                                sp.ofs_b = sp.act_b ? sp.ofs_b : bad.ofs_b;
#endif
                                if (sp.act_b && !sp.act_a)
                                    fail("seg_pair N=%d: segment b without segment a", N);
                                w.lane(name, sp.ofs_a, sp.act_a, job.step0 + sp.seg);
                                w.lane(name, sp.ofs_b, sp.act_b, job.step0 + sp.seg + 1);
                            } else {
                                OneSeg sg = one_seg<TEAMS>(job, hop, lt, team);
#if SEGK_SEED == 1
                                sg.ofs = sg.act ? sg.ofs : one_seg<TEAMS>(wrong, hop, lt, team).ofs;
#endif
                                w.lane(name, sg.ofs, sg.act, job.step0 + sg.seg);
                            }
                        }
                w.done(name);
                lanes += w.lanes;
                idle += w.idle;
                (void)wrong;
            }
        }
    }
}

template <int N>
static void check_addressing(long long &lanes, long long &idle)
{
    using Cfg = CrossCfg<N>;
    static_assert(Cfg::TEAMS == seg_teams(N) && Cfg::SPT == seg_spt(N) && Cfg::BLOCK == seg_block(N) && Cfg::TEAM == seg_team(N), "one shape");
    walk_addressing<N, Cfg::TEAMS, Cfg::SPT>(true, lanes, idle);
}

// ---- combine ---------------------------------------------------------------------------------------------------------------------
// the value of (group, row, bin): a mantissa and one of 24 binades from a hash of the three
static float value_of(int g, int row, int bin)
{
    uint32_t h = (uint32_t)g * 0x9E3779B1u ^ (uint32_t)row * 0x85EBCA77u ^ (uint32_t)bin * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return std::ldexp(1.0f + (float)(h & 0xFFFF) / 65536.0f, (int)((h >> 16) % 24) - 12);
}
static float sum_of(int groups, int row, int bin)
{
    volatile float s = 0.0f; // ascending, one f32 sum
    for (int g = 0; g < groups; ++g)
        s = s + value_of(g, row, bin);
    return s;
}

constexpr int GUARD = 4096;
constexpr uint32_t GUARD_BITS = 0x7FC0DEADu;
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// drive combine C (OwnedCombine or SlotCombine) for a workgroup of `groups` groups of `gs` threads through all its turns.
// fill(g, pt, acc) sets a thread's accumulators, bin_of(row, i) is the bin partial element [row][i] must hold, rows x h the partial
template <class C, class Acc, class Fill, class BinOf>
static void drive(const char *name, int n, int lds_floats, int groups, int gs, int rows, int h, Fill fill, BinOf bin_of)
{
    if (C::LDS_FLOATS > lds_floats)
        fail("%s N=%d: a turn takes %d floats of LDS, the kernel's frames hold %d", name, n, C::LDS_FLOATS, lds_floats);
    const int block = groups * gs;
    float guard;
    std::memcpy(&guard, &GUARD_BITS, 4);
    std::vector<float> lds((size_t)lds_floats + 2 * GUARD, guard);
    float *fq = lds.data() + GUARD;
    std::vector<float> out((size_t)rows * h, guard);
    std::vector<int> wrote((size_t)rows * h, 0);
    for (int p = 0; p < C::TURNS; ++p) {
        std::fill(fq, fq + lds_floats, NAN); // what a turn does not store it must not read
        for (int tid = 0; tid < block; ++tid) {
            Acc acc;
            fill(tid / gs, tid % gs, acc.a);
            C::store(fq, tid / gs, tid % gs, p, acc.a);
        }
        for (int i = 0; i < GUARD; ++i)
            if (!same_bits(lds[i], guard) || !same_bits(lds[(size_t)GUARD + lds_floats + i], guard)) {
                fail("%s N=%d turn %d: a store outside the kernel's %d floats of LDS", name, n, p, lds_floats);
                break;
            }
        for (int tid = 0; tid < block; ++tid)
            for (int e = tid; e < C::ELEMS; e += block) { // the wrapper's loop
                float s;
                const int at = C::sum(fq, SEGK_SEED == 2 ? 0 : p, e, s);
                if (at < 0 || at >= rows * h) {
                    fail("%s N=%d turn %d: element %d goes to %d, outside the partial", name, n, p, e, at);
                    continue;
                }
                ++wrote[at];
                out[at] = s;
            }
    }
    for (int row = 0; row < rows; ++row)
        for (int i = 0; i < h; ++i) {
            const int at = row * h + i;
            if (wrote[at] != 1)
                fail("%s N=%d: partial [%d][%d] written %d times", name, n, row, i, wrote[at]);
            else if (!same_bits(out[at], sum_of(groups, bin_of(row, i).first, bin_of(row, i).second)))
                fail("%s N=%d: partial [%d][%d] is %g, the groups' values in ascending order sum to %g", name, n, row, i, out[at],
                     sum_of(groups, bin_of(row, i).first, bin_of(row, i).second));
        }
}

template <int A, int B>
struct Acc2 {
    float a[A][B];
};

// owned bins: row `row` of bin k is value (row, k); rows are plain
template <int H, int ROWS, int TURN, int GROUPS, int GS>
static void check_owned(const char *name, int n, int lds_floats)
{
    using C = OwnedCombine<H, ROWS, TURN, GROUPS, GS>;
    drive<C, Acc2<C::XB, ROWS>>(
        name, n, lds_floats, GROUPS, GS, ROWS, H,
        [](int g, int pt, float(&acc)[C::XB][ROWS]) {
            for (int r = 0; r < C::XB; ++r)
                for (int c = 0; c < ROWS; ++c)
                    acc[r][c] = pt + GS * r < H ? value_of(g, c, pt + GS * r) : NAN;
        },
        [](int row, int i) { return std::make_pair(row, i); });
}

// slot order: value q of transform bin j is value (q, j); row r shows value r >> 1, odd rows bin (N - i) mod N
template <int N, int Q, int V>
static void check_slots(const char *name, int lds_floats)
{
    using C = SlotCombine<N, Q, V>;
    using Cfg = CrossCfg<N>;
    drive<C, Acc2<Q, C::E>>(
        name, N, lds_floats, Cfg::TEAMS, Cfg::TEAM, 2 * Q, Cfg::H,
        [](int g, int t, float(&acc)[Q][C::E]) {
            for (int q = 0; q < Q; ++q)
                for (int s = 0; s < C::E; ++s)
                    acc[q][s] = value_of(g, q, freq_of_slot<N>(t, s));
        },
        [](int row, int i) { return std::make_pair(row / 2, row % 2 ? (N - i) % N : i); });
    for (int row = 0; row < 2 * Q; ++row)
        for (int i = 0; i < Cfg::H; ++i)
            if (two_sided_value(row) != row / 2 || two_sided_bin<N>(row, i) != (row % 2 ? (N - i) % N : i))
                fail("two_sided N=%d: row %d index %d", N, row, i);
}

template <int N>
static void check_combines()
{
    using Cfg = CrossCfg<N>;
    constexpr int H = Cfg::H, TEAMS = Cfg::TEAMS, TEAM = Cfg::TEAM;
    constexpr int ONE = TEAMS * Cfg::FRAME * 2, TWO = 2 * ONE; // floats of `frames`: one frame a team, or two
    check_owned<H, 4, 4, TEAMS, TEAM>("cross", N, TWO);
    check_owned<H, SK_ROWS, SK_ROWS, TEAMS, TEAM>("sk", N, ONE);
    check_owned<H, ZAMPM_ROWS, 2, TEAMS, TEAM>("zoom_ampm", N, ONE);
    check_owned<H, ZXAMPM_ROWS, ZXAMPM_TURN, TEAMS, TEAM>("zoom_ampm_cross", N, TWO);
    check_slots<N, 1, 1>("zoom", ONE);
    check_slots<N, ZSK_Q, ZSK_Q>("zoom_sk", ONE);
    check_slots<N, ZCROSS_Q, 2>("zoom_cross", ONE);
    for (int r = 0; r < SK_ROWS; ++r) // sk's element function is the owned-bin layout of one group
        for (int k = 0; k < H; ++k)
            if (sk_row_at<N>(r, k) != r * H + k)
                fail("sk_row_at N=%d", N);
}

// csm_kernel<N, M>: its tiles, its product loop thread by thread (csm.hip: thread pt of product group pg takes the bins
// pt + GS r of the teams pg, pg + PG, ... that hold a segment), and the combine of its product groups where it has more than one
template <int N, int M>
static int check_csm(long long &lanes, long long &idle)
{
    using S = CsmShape<N, M>;
    static_assert(S::TEAM == seg_team(N) && S::TEAMS * S::TEAM == S::BLOCK && S::PG * S::GS == S::BLOCK, "whole teams, whole groups");
    char name[32];
    snprintf(name, sizeof name, "csm m=%d", M);
    walk_addressing<N, S::TEAMS, S::SPT>(false, lanes, idle);
    for (int nseg : {1, 2, S::SPT - 1, S::SPT}) { // one tile: the teams with a segment, and the odd last one
        std::vector<int> taken((size_t)S::TEAMS * S::H, 0);
        const Job job = {0, 0, nseg, 1, 1, 0};
        for (int tid = 0; tid < S::BLOCK; ++tid) {
            const int pg = tid / S::GS, pt = tid % S::GS;
            for (int g = pg; g < S::TEAMS; g += S::PG) {
                const int lg = 2 * g;
                if (lg >= nseg)
                    break;
                const SegPair sp = seg_pair(job, N / 2, nseg, 2 * g);
                if (!sp.act_a || sp.act_b != (lg + 1 < nseg))
                    fail("%s N=%d nseg=%d: the product loop and the tile disagree on team %d", name, N, nseg, g);
                for (int r = 0; r < S::XB; ++r)
                    if (pt + S::GS * r < S::H)
                        ++taken[(size_t)g * S::H + pt + S::GS * r];
            }
        }
        for (int g = 0; g < S::TEAMS; ++g)
            for (int k = 0; k < S::H; ++k)
                if (taken[(size_t)g * S::H + k] != (2 * g < nseg ? 1 : 0))
                    fail("%s N=%d nseg=%d: bin %d of team %d taken %d times", name, N, nseg, k, g, taken[(size_t)g * S::H + k]);
    }
    if constexpr (S::PG > 1)
        check_owned<S::H, S::ROWS, S::ROWS, S::PG, S::GS>(name, N, S::TEAMS * M * S::FRAME * 2);
    return S::PG > 1;
}

#define SEGK_SIZES(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)
#define SEGK_CSM(X) \
    X(64, 2) X(64, 3) X(64, 4) X(128, 2) X(128, 3) X(128, 4) X(256, 2) X(256, 3) X(256, 4) X(512, 2) X(512, 3) X(512, 4) \
    X(1024, 2) X(1024, 3) X(1024, 4) X(2048, 2) X(2048, 3) X(2048, 4) X(4096, 2) X(4096, 3)

static void print_shapes()
{
#define X(NN) printf("team %d teams %d block %d\n", NN, seg_teams(NN), seg_block(NN));
    SEGK_SIZES(X)
#undef X
#define X(NN, MM)                                                                                                          \
    printf("csm %d %d block %d teams %d spt %d pg %d gs %d\n", NN, MM, CsmShape<NN, MM>::BLOCK, CsmShape<NN, MM>::TEAMS, \
           CsmShape<NN, MM>::SPT, CsmShape<NN, MM>::PG, CsmShape<NN, MM>::GS);
    SEGK_CSM(X)
#undef X
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--shapes")) {
        print_shapes();
        return 0;
    }
    long long lanes = 0, idle = 0;
    int sizes = 0, shapes = 0, grouped = 0;
#define X(NN) check_addressing<NN>(lanes, idle);
    SEGK_SIZES(X)
#undef X
#define X(NN)             \
    check_combines<NN>(); \
    ++sizes;
    SEGK_SIZES(X)
#undef X
#define X(NN, MM)                               \
    grouped += check_csm<NN, MM>(lanes, idle); \
    ++shapes;
    SEGK_CSM(X)
#undef X
    printf("addressing: %lld lanes walked, %lld without a segment\n", lanes, idle);
    printf("combine: 7 team kernels at %d sizes, N = 64 ... 4096, and csm at %d shapes (N, M), %d of them with product groups\n", sizes,
           shapes, grouped);
    if (g_fail) {
        printf("segment_kernel_check: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("segment_kernel_check (seed %d): OK\n", SEGK_SEED);
    return 0;
}
