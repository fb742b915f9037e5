// waterfall_robust_emul.cpp -- csrc/waterfall_robust.h on the host: what one thread of wf_robust_kernel computes, over model
// rings, against a sort-based restatement, bit for bit.
//   * a model ring of K slots is filled block by block (slot = block mod K; a slot's set is S1 of every side, then S2 of every
//     side), with the partial newest block present or absent; wf_robust_rows picks the considered rows, wf_robust_bin reduces them
//   * the restatement gathers the considered rows into vectors, sorts them and states the header's semantics
//     (include/psdcascade_robust.h) directly: median from the sorted values, min / max from their ends, NaN if any value is one;
//     the excised mean by a plain loop over the rows in order
//   * cases: R = 1 ... 9 and 64; before and after the ring wraps; all rows equal; many ties; all rows zero; NaN in one row at some
//     bins; +inf in a row; limits -inf / +inf; max_rows below the rows held; outputs skipped (want_median / want_sk off)
// With a file name as its argument the program also writes every case's considered rows and outputs there (a flat binary record a
// case), which tests/test_waterfall_robust_host.py compares with numpy.
// Stand-alone (no HIP): tests/test_waterfall_robust_host.py builds it plainly and with -fsanitize=address,undefined.
#include "waterfall_robust.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
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

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

enum Fill { RANDOM, EQUAL, TIES, ZERO, NAN_ROW, INF_ROW };

struct Case {
    const char *name;
    uint32_t K, B, newest, max_rows, sides, nb;
    uint64_t started;
    Fill fill;
    double lo, hi;
};

static FILE *dump = nullptr;
static std::mt19937_64 rng(20261021);

template <class T>
static void put(const T *p, size_t n)
{
    if (dump && fwrite(p, sizeof(T), n, dump) != n) {
        printf("FAIL: short write\n");
        exit(1);
    }
}

// S1 and S2 of block b at (side, bin): a function of the case alone, so the restatement does not read the ring
static void moments(const Case &c, uint64_t b, uint32_t side, uint32_t k, uint64_t special, double *s1, double *s2)
{
    std::mt19937_64 r(b * 1000003u + side * 7919u + k * 31u + 17u);
    std::uniform_real_distribution<double> mant(1.0, 2.0), u(0.0, 1.0);
    double v = std::ldexp(mant(r), (int)(r() % 40) - 20);
    if (c.fill == EQUAL)
        v = 3.25 + k;
    if (c.fill == TIES)
        v = 1.0 + (double)(r() % 3); // three values over all rows
    if (c.fill == ZERO)
        v = 0.0;
    double w = v * v / c.B * (1.0 + 2.5 * u(r)); // SK between 0 and 2.5 (B + 1) / (B - 1)
    if (c.fill == NAN_ROW && b == special && k % 3 == 0)
        v = w = std::nan("");
    if (c.fill == INF_ROW && b == special && k % 2 == 1) {
        v = std::numeric_limits<double>::infinity();
        w = k % 4 == 1 ? v : w;
    }
    *s1 = v;
    *s2 = w;
}

static void run(const Case &c)
{
    const size_t set = (size_t)2 * c.sides * c.nb;
    std::vector<double> ring((size_t)c.K * set, -7.0); // (a slot never written would show as a negative value)
    uint64_t last = 0;
    const uint32_t R = wf_robust_rows(c.started, c.newest, c.B, c.K, c.max_rows, &last);
    const bool partial = c.started && c.newest < c.B;
    const uint64_t complete = c.started - (partial ? 1 : 0);
    const uint32_t held = (uint32_t)std::min<uint64_t>(c.started, c.K) - (partial ? 1 : 0);
    CHECK(R == std::min(std::min(c.max_rows, held), WF_ROBUST_MAX_ROWS), "%s: R = %u", c.name, R);
    if (R)
        CHECK(last == complete - 1, "%s: last = %llu", c.name, (unsigned long long)last);
    const uint64_t special = R ? last - R / 2 : 0; // the block that holds the NaN or the +inf
    for (uint64_t b = c.started > 2 * (uint64_t)c.K ? c.started - 2 * c.K : 0; b < c.started; ++b)
        for (uint32_t side = 0; side < c.sides; ++side)
            for (uint32_t k = 0; k < c.nb; ++k) {
                double s1, s2;
                moments(c, b, side, k, special, &s1, &s2);
                if (b + 1 == c.started && partial) // the partial newest block: small values that would win every minimum
                    s1 = s2 = 1e-300;
                ring[(b % c.K) * set + (size_t)side * c.nb + k] = s1;
                ring[(b % c.K) * set + (size_t)(c.sides + side) * c.nb + k] = s2;
            }
    const double g = (double)0.0123f;
    const uint32_t hdr[4] = {R, c.sides * c.nb, c.B, 0};
    const double par[3] = {g, c.lo, c.hi};
    put(hdr, 4);
    put(par, 3);
    std::vector<double> V((size_t)R * c.sides * c.nb), W(V.size());
    std::vector<float> med(c.sides * c.nb), mn(med.size()), mx(med.size()), exc(med.size());
    std::vector<uint32_t> kept(med.size());
    for (uint32_t side = 0; side < c.sides; ++side)
        for (uint32_t k = 0; k < c.nb; ++k) {
            if (!R)
                continue;
            WfRobustRows w;
            w.ring = ring.data();
            w.last = last;
            w.K = c.K;
            w.R = R;
            w.set = set;
            w.o1 = (size_t)side * c.nb + k;
            w.o2 = (size_t)(c.sides + side) * c.nb + k;
            const WfRobustBin got = wf_robust_bin(w, c.B, g, c.lo, c.hi, true, true);
            // the restatement
            std::vector<double> v(R), s2(R);
            bool nan = false;
            for (uint32_t r = 0; r < R; ++r) {
                moments(c, last - (R - 1) + r, side, k, special, &v[r], &s2[r]);
                nan = nan || std::isnan(v[r]);
                V[((size_t)r * c.sides + side) * c.nb + k] = v[r];
                W[((size_t)r * c.sides + side) * c.nb + k] = s2[r];
            }
            double sum = 0.0;
            uint32_t nk = 0;
            for (uint32_t r = 0; r < R; ++r) {
                const double m = (double)c.B;
                const double sk = v[r] == 0.0 ? std::nan("") : (m + 1.0) / (m - 1.0) * (m * s2[r] / (v[r] * v[r]) - 1.0);
                if (!std::isnan(sk) && c.lo <= sk && sk <= c.hi) {
                    ++nk;
                    sum += v[r];
                }
            }
            float want_med = std::nanf(""), want_min = want_med, want_max = want_med;
            if (!nan) {
                std::sort(v.begin(), v.end());
                const double m = R & 1 ? v[(R - 1) / 2] : 0.5 * (v[R / 2 - 1] + v[R / 2]);
                want_med = (float)(m * g);
                want_min = (float)(v.front() * g);
                want_max = (float)(v.back() * g);
            }
            const float want_exc = nk ? (float)((sum / (double)nk) * g) : std::nanf("");
            CHECK(same_bits(got.median, want_med), "%s side %u bin %u: median %a against %a", c.name, side, k, (double)got.median, (double)want_med);
            CHECK(same_bits(got.min, want_min), "%s side %u bin %u: min %a against %a", c.name, side, k, (double)got.min, (double)want_min);
            CHECK(same_bits(got.max, want_max), "%s side %u bin %u: max %a against %a", c.name, side, k, (double)got.max, (double)want_max);
            CHECK(same_bits(got.excised, want_exc), "%s side %u bin %u: excised %a against %a", c.name, side, k, (double)got.excised, (double)want_exc);
            CHECK(got.kept == nk, "%s side %u bin %u: kept %u against %u", c.name, side, k, got.kept, nk);
            if (c.fill == ZERO)
                CHECK(got.median == 0.0f && got.min == 0.0f && got.max == 0.0f && got.kept == 0 && std::isnan(got.excised), "%s: zeros", c.name);
            if (c.fill == EQUAL)
                CHECK(same_bits(got.median, got.min) && same_bits(got.median, got.max), "%s: ties", c.name);
            // the outputs not asked for cost nothing and change nothing of the others
            const WfRobustBin a = wf_robust_bin(w, c.B, g, c.lo, c.hi, false, true), b2 = wf_robust_bin(w, c.B, g, c.lo, c.hi, true, false);
            CHECK(same_bits(a.min, got.min) && same_bits(a.max, got.max) && same_bits(a.excised, got.excised) && a.kept == got.kept,
                  "%s: without the median", c.name);
            CHECK(same_bits(b2.min, got.min) && same_bits(b2.max, got.max) && same_bits(b2.median, got.median), "%s: without the SK", c.name);
            const size_t o = (size_t)side * c.nb + k;
            med[o] = got.median, mn[o] = got.min, mx[o] = got.max, exc[o] = got.excised, kept[o] = got.kept;
        }
    put(V.data(), V.size());
    put(W.data(), W.size());
    if (R) {
        put(med.data(), med.size());
        put(mn.data(), mn.size());
        put(mx.data(), mx.size());
        put(exc.data(), exc.size());
        put(kept.data(), kept.size());
    }
    printf("case %s: K=%u started=%llu newest=%u/%u max_rows=%u -> R=%u\n", c.name, c.K, (unsigned long long)c.started, c.newest, c.B,
           c.max_rows, R);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !(dump = fopen(argv[1], "wb"))) {
        printf("FAIL: cannot write %s\n", argv[1]);
        return 1;
    }
    const double inf = std::numeric_limits<double>::infinity();
    const uint32_t all = 0xFFFFFFFFu;
    std::vector<std::string> names;
    names.reserve(64);
    for (uint32_t R : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 64u}) {
        names.push_back("R=" + std::to_string(R) + " unwrapped");
        run(Case{names.back().c_str(), R + 3, 8, 8, all, 1, 37, R, RANDOM, 0.6, 1.6});
        names.push_back("R=" + std::to_string(R) + " wrapped partial");
        run(Case{names.back().c_str(), R + 1, 4, 3, all, 2, 19, 3 * (uint64_t)R + 5, RANDOM, 0.6, 1.6});
        names.push_back("R=" + std::to_string(R) + " ties");
        run(Case{names.back().c_str(), R, 4, 4, all, 1, 11, 2 * (uint64_t)R + 1, TIES, 0.0, 2.0});
    }
    run(Case{"unwrapped partial", 12, 8, 5, all, 1, 33, 7, RANDOM, 0.6, 1.6});
    run(Case{"unwrapped complete", 12, 8, 8, all, 1, 33, 7, RANDOM, 0.6, 1.6});
    run(Case{"wrapped partial", 12, 8, 1, all, 2, 33, 31, RANDOM, 0.6, 1.6});
    run(Case{"wrapped complete", 12, 8, 8, all, 2, 33, 31, RANDOM, 0.6, 1.6});
    run(Case{"max_rows 5 of 12", 12, 8, 8, 5, 1, 33, 31, RANDOM, 0.6, 1.6});
    run(Case{"max_rows 6 of 11", 12, 8, 2, 6, 1, 33, 31, RANDOM, 0.6, 1.6});
    run(Case{"max_rows 0", 12, 8, 8, 0, 1, 5, 31, RANDOM, 0.6, 1.6});
    run(Case{"first block partial", 12, 8, 3, all, 1, 5, 1, RANDOM, 0.6, 1.6});
    run(Case{"nothing yet", 12, 8, 0, all, 1, 5, 0, RANDOM, 0.6, 1.6});
    run(Case{"depth 1 partial", 1, 8, 3, all, 1, 5, 9, RANDOM, 0.6, 1.6});
    run(Case{"depth 1 complete", 1, 8, 8, all, 1, 5, 9, RANDOM, 0.6, 1.6});
    run(Case{"all equal odd", 7, 4, 4, all, 1, 17, 20, EQUAL, -inf, inf});
    run(Case{"all equal even", 8, 4, 4, all, 2, 17, 20, EQUAL, -inf, inf});
    run(Case{"all zero", 6, 4, 4, all, 2, 17, 9, ZERO, -inf, inf});
    run(Case{"nan row odd", 9, 4, 4, all, 1, 17, 30, NAN_ROW, -inf, inf});
    run(Case{"nan row even", 8, 4, 4, all, 1, 17, 30, NAN_ROW, 0.6, 1.6});
    run(Case{"inf row odd", 9, 4, 4, all, 1, 17, 30, INF_ROW, -inf, inf});
    run(Case{"inf row even", 4, 4, 4, all, 1, 17, 30, INF_ROW, -inf, inf});
    run(Case{"inf row R=2", 2, 4, 4, all, 1, 17, 30, INF_ROW, -inf, inf});
    run(Case{"limits -inf..1", 12, 8, 8, all, 1, 33, 31, RANDOM, -inf, 1.0});
    run(Case{"limits 1..inf", 12, 8, 8, all, 1, 33, 31, RANDOM, 1.0, inf});
    run(Case{"limits -inf..inf", 12, 8, 8, all, 1, 33, 31, RANDOM, -inf, inf});
    run(Case{"limits empty", 12, 8, 8, all, 1, 33, 31, RANDOM, 100.0, 200.0});
    run(Case{"past 2^32 blocks", 5, 8, 2, all, 1, 9, ((uint64_t)1 << 33) + 3, RANDOM, 0.6, 1.6});
    {
        uint64_t last;
        CHECK(wf_robust_rows(10000, 4, 4, 8192, 0xFFFFFFFFu, &last) == WF_ROBUST_MAX_ROWS && last == 9999, "the cap of 4096 rows");
        CHECK(wf_robust_rows(10000, 3, 4, 8192, 0xFFFFFFFFu, &last) == WF_ROBUST_MAX_ROWS && last == 9998, "the cap of 4096 rows");
    }
    if (dump)
        fclose(dump);
    printf("waterfall_robust_emul: %lld checks\nOK\n", checks);
    return 0;
}
