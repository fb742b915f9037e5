// waterfall_plan_check.cpp -- csrc/waterfall_plan.h against its definition, exhaustively over small numbers: every span
// [s0, s1) with s0 = 0 ... 40 and s1 = s0 ... s0 + 40, every B = 2 ... 9 and K = 1 ... 5, and every sequence of three consecutive
// spans [0, a), [a, b), [b, c) with c <= 40 (what three rounds of a stage make).  Per span: every segment lies in exactly one
// piece, no piece crosses a block, the pieces are in segment order, slot = block mod K, and `fresh` is set exactly on the piece
// that holds a block's first segment.  Per sequence: every block started gets `fresh` exactly once, on its first segment, and a
// model ring folded piece by piece (fresh overwrites, else adds) holds exactly the newest min(K, started) blocks with their counts.
// Stand-alone (no HIP): tests/test_waterfall_host.py builds it plainly and with -fsanitize=address,undefined.
#include "waterfall_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace psdk;

static long long checks = 0;

#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                                \
            printf(__VA_ARGS__);                                                                                       \
            printf("\n");                                                                                              \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

static std::vector<WfPiece> cut(uint64_t s0, uint64_t s1, uint32_t B, uint32_t K)
{
    std::vector<WfPiece> out;
    wf_cut(s0, s1, B, K, [&](const WfPiece &p) { out.push_back(p); });
    return out;
}

static void check_span(uint64_t s0, uint64_t s1, uint32_t B, uint32_t K)
{
    const std::vector<WfPiece> ps = cut(s0, s1, B, K);
    uint64_t at = s0;
    for (const WfPiece &p : ps) {
        CHECK(p.seg0 == at, "span [%llu, %llu) B %u K %u: piece at %llu, expected %llu (order / cover)", (unsigned long long)s0,
              (unsigned long long)s1, B, K, (unsigned long long)p.seg0, (unsigned long long)at);
        CHECK(p.nseg >= 1 && p.nseg <= B, "piece of %u segments", p.nseg);
        const uint64_t b = p.seg0 / B;
        CHECK((p.seg0 + p.nseg - 1) / B == b, "piece [%llu, +%u) crosses a block of %u", (unsigned long long)p.seg0, p.nseg, B);
        CHECK(p.slot == b % K, "slot %u of block %llu, K %u", p.slot, (unsigned long long)b, K);
        CHECK(p.fresh == (p.seg0 % B == 0), "fresh %d on a piece at segment %llu, B %u", (int)p.fresh, (unsigned long long)p.seg0, B);
        at += p.nseg;
    }
    CHECK(at == s1 || (ps.empty() && s0 >= s1), "span [%llu, %llu) ends at %llu", (unsigned long long)s0, (unsigned long long)s1,
          (unsigned long long)at);
    // at most one piece a block: a block's segments of one span are consecutive
    for (size_t i = 1; i < ps.size(); ++i)
        CHECK(ps[i].seg0 / B == ps[i - 1].seg0 / B + 1, "two pieces of one block, or a block skipped");
}

static void check_sequence(uint64_t a, uint64_t b, uint64_t c, uint32_t B, uint32_t K)
{
    struct Slot {
        long long block = -1;
        uint32_t count = 0;
    };
    std::vector<Slot> ring(K);
    std::vector<int> fresh_seen(c / B + 2, 0);
    const uint64_t cuts[4] = {0, a, b, c};
    for (int r = 0; r < 3; ++r)
        for (const WfPiece &p : cut(cuts[r], cuts[r + 1], B, K)) {
            const uint64_t blk = p.seg0 / B;
            if (p.fresh) {
                ++fresh_seen[blk];
                CHECK(p.seg0 == blk * B, "fresh off a block's first segment");
                ring[p.slot] = Slot{(long long)blk, p.nseg};
            } else {
                CHECK(ring[p.slot].block == (long long)blk, "a piece of block %llu adds to a slot that holds block %lld",
                      (unsigned long long)blk, ring[p.slot].block);
                ring[p.slot].count += p.nseg;
            }
        }
    const uint64_t started = wf_blocks_started(c, B);
    CHECK(started == (c + B - 1) / B, "blocks started");
    for (uint64_t blk = 0; blk < fresh_seen.size(); ++blk)
        CHECK(fresh_seen[blk] == (blk < started ? 1 : 0), "block %llu fresh %d times (started %llu)", (unsigned long long)blk,
              fresh_seen[blk], (unsigned long long)started);
    const uint64_t valid = started < K ? started : K;
    for (uint64_t i = 0; i < valid; ++i) {
        const uint64_t blk = started - 1 - i;
        const uint32_t want = i == 0 ? wf_newest_count(c, B) : B;
        CHECK(ring[blk % K].block == (long long)blk && ring[blk % K].count == want, "slot %llu holds block %lld count %u, expected %llu count %u",
              (unsigned long long)(blk % K), ring[blk % K].block, ring[blk % K].count, (unsigned long long)blk, want);
    }
    CHECK(c == 0 ? wf_newest_count(c, B) == 0 : (wf_newest_count(c, B) >= 1 && wf_newest_count(c, B) <= B), "newest count");
}

int main()
{
    for (uint32_t B = 2; B <= 9; ++B)
        for (uint32_t K = 1; K <= 5; ++K) {
            for (uint64_t s0 = 0; s0 <= 40; ++s0)
                for (uint64_t s1 = s0; s1 <= s0 + 40; ++s1)
                    check_span(s0, s1, B, K);
            for (uint64_t a = 0; a <= 40; ++a)
                for (uint64_t b = a; b <= 40; ++b)
                    for (uint64_t c = b; c <= 40; ++c)
                        check_sequence(a, b, c, B, K);
        }
    // large indices: the arithmetic is 64-bit
    check_span(((uint64_t)1 << 40) + 3, ((uint64_t)1 << 40) + 100, 7, 5);
    check_span((uint64_t)5 << 24, ((uint64_t)7 << 24) + 1, 1u << 24, 3);
    printf("waterfall_plan_check: %lld checks\nOK\n", checks);
    return 0;
}
