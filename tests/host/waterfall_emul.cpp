// waterfall_emul.cpp -- csrc/waterfall_read.h on the host: the ring-order map and the per-element arithmetic of wf_image_kernel.
//   * order map: a model ring filled block by block (slot = block mod K, each slot tagged with its block) is read back through
//     wf_row_slot for started < K, = K, = K + 1 and = 3 K + 2, for every K = 1 ... 9 and every row count nr = 1 ... valid:
//     row r must be block started - nr + r, rows oldest first, the last one the newest block.
//   * psd: wf_psd against (float)(s1 * (double)gsc) over magnitudes from 1e-30 to 1e30, bit for bit.
//   * sk: wf_sk against the f64 formula (M + 1) / (M - 1) (M S2 / S1^2 - 1) rounded once; NaN at count 0 and 1 and at S1 == 0;
//     0 for a constant periodogram; about 1 for an exponential one.
// Stand-alone (no HIP): tests/test_waterfall_host.py builds it plainly and with -fsanitize=address,undefined.
#include "waterfall_read.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

static void order_case(uint32_t K, uint64_t started, const char *what)
{
    std::vector<long long> ring(K, -1); // the block a slot holds
    for (uint64_t b = started > 2 * (uint64_t)K ? started - 2 * K : 0; b < started; ++b) // (older blocks are overwritten anyway)
        ring[b % K] = (long long)b;
    const uint32_t valid = wf_valid_rows(started, K);
    CHECK(valid == (started < K ? started : K), "%s: valid rows %u", what, valid);
    for (uint32_t nr = 1; nr <= valid; ++nr)
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t slot = wf_row_slot(started, K, nr, r);
            CHECK(slot < K, "%s: slot %u of a ring of %u", what, slot, K);
            const uint64_t want = started - nr + r;
            CHECK(wf_row_block(started, nr, r) == want && ring[slot] == (long long)want,
                  "%s K %u started %llu nr %u: row %u reads slot %u holding block %lld, expected block %llu", what, K,
                  (unsigned long long)started, nr, r, slot, ring[slot], (unsigned long long)want);
        }
    printf("order %s K=%u started=%llu valid=%u\n", what, K, (unsigned long long)started, valid);
}

int main()
{
    for (uint32_t K = 1; K <= 9; ++K) {
        if (K > 1)
            order_case(K, K - 1, "started<K");
        order_case(K, K, "started=K");
        order_case(K, K + 1, "started=K+1");
        order_case(K, 3 * (uint64_t)K + 2, "started=3K+2");
    }
    order_case(5, ((uint64_t)1 << 33) + 3, "past 2^32 blocks");
    CHECK(wf_valid_rows(0, 4) == 0, "an empty ring has rows");

    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> mant(1.0, 2.0);
    std::uniform_int_distribution<int> ex(-100, 100);
    for (int i = 0; i < 200000; ++i) {
        const double s1 = std::ldexp(mant(rng), ex(rng));
        const float gsc = (float)std::ldexp(mant(rng), ex(rng) / 4);
        const float want = (float)(s1 * (double)gsc);
        CHECK(same_bits(wf_psd(s1, gsc), want), "psd of %a * %a", s1, (double)gsc);
    }
    CHECK(wf_psd(0.0, 3.0f) == 0.0f, "psd of nothing");
    printf("psd 200000 elements bit-equal to (float)(s1 * (double)gsc)\n");

    double worst = 0.0;
    for (int i = 0; i < 200000; ++i) {
        const uint32_t count = 2 + (uint32_t)(rng() % 5000);
        const double s1 = std::ldexp(mant(rng), ex(rng) / 4) * count;
        const double s2 = s1 * s1 / count * (1.0 + 2.0 * (mant(rng) - 1.0)); // R = M S2 / S1^2 in [1, 3)
        const double m = (double)count;
        const double ref = (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0);
        const float got = wf_sk(count, s1, s2);
        CHECK(same_bits(got, (float)ref), "sk count %u s1 %a s2 %a: %a against %a", count, s1, s2, (double)got, ref);
        worst = std::fmax(worst, std::fabs((double)got - ref) / std::fmax(std::fabs(ref), 1e-30));
    }
    printf("sk 200000 elements: one rounding of the f64 formula, worst relative distance to it %.3g\n", worst);
    for (uint32_t count : {0u, 1u}) {
        CHECK(std::isnan(wf_sk(count, 1.0, 1.0)), "count %u is a number", count);
        CHECK(std::isnan(wf_sk(count, 0.0, 0.0)), "count %u without power is a number", count);
    }
    CHECK(std::isnan(wf_sk(2, 0.0, 0.0)) && std::isnan(wf_sk(100, 0.0, 1.0)), "S1 == 0 is a number");
    CHECK(!std::isnan(wf_sk(2, 1.0, 1.0)), "count 2 is NaN");
    // a constant periodogram P: S1 = M P, S2 = M P^2 reads 0; a NaN moment stays a NaN (it is not hidden)
    CHECK(wf_sk(64, 64 * 3.0, 64 * 9.0) == 0.0f, "a line does not read 0");
    CHECK(std::isnan(wf_sk(64, std::nan(""), 1.0)), "a NaN moment reads a number");
    printf("sk NaN at count<2 and S1==0\n");
    printf("waterfall_emul: %lld checks\nOK\n", checks);
    return 0;
}
