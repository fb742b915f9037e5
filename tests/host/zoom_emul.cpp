// Host side of stabilizer-stream_amd/csrc/zoom_lo.h, the local oscillator of the zoom cascade (the same source the device runs).
//   zoom_emul check                              zoom_lo against f64 cos / sin of the same 32-bit-truncated phase: every octant
//                                                boundary +-1 step (of the 32-bit phase), 2^21 random 64-bit phases and a sweep of
//                                                each octant; the quarter turns exactly.  Prints the worst error, "OK" if <= 2^-23.
//   zoom_emul mix FTW PHASE0 IN.f32 OUT.f32      the mixer: sample j of IN with phase PHASE0 + FTW j mod 2^64; OUT holds every I,
//                                                then every Q (what zoom_mix_kernel stores into the two stage-0 streams)
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> zoom_emul.cpp (tests/test_zoom_host.py does).
#include "zoom_lo.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
using namespace psdk;

static double worst = 0.0;
static uint64_t worst_at = 0, n_checked = 0;

static void one(uint64_t phase)
{
    float c, s;
    zoom_lo(phase, c, s);
    const double a = 2.0 * M_PI * (double)(uint32_t)(phase >> 32) / 4294967296.0;
    const double e = std::max(std::fabs((double)c - cos(a)), std::fabs((double)s - sin(a)));
    if (e > worst) {
        worst = e;
        worst_at = phase;
    }
    ++n_checked;
}

static int check()
{
    bool exact = true;
    const float want[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
    for (int q = 0; q < 4; ++q)
        for (uint64_t low : {(uint64_t)0, (uint64_t)1, (uint64_t)0xFFFFFFFFu}) { // (bits below the top 32 do not count)
            float c, s;
            zoom_lo(((uint64_t)q << 62) | low, c, s);
            if (!(c == want[q][0] && s == want[q][1])) {
                printf("quarter turn %d: (%.9g, %.9g)\n", q, c, s);
                exact = false;
            }
        }
    for (uint32_t o = 0; o < 8; ++o)
        for (int d = -64; d <= 64; ++d) // the boundaries, +-1 step and the low-bit split around them
            one((uint64_t)((o << 29) + (uint32_t)d) << 32);
    std::mt19937_64 rng(12345);
    for (int i = 0; i < (1 << 21); ++i)
        one(rng());
    for (uint32_t o = 0; o < 8; ++o)
        for (uint32_t i = 0; i < (1u << 17); ++i) // a sweep of each octant with every low-bit pattern
            one((uint64_t)((o << 29) + i * 4099u) << 32);
    const double bound = 1.0 / 8388608.0; // 2^-23
    printf("zoom_lo: %" PRIu64 " phases, worst |error| %.4g = 2^%.2f at phase 0x%016" PRIx64 " (bound 2^-23 = %.4g)\n", n_checked, worst,
           log2(worst), worst_at, bound);
    if (!exact || !(worst <= bound)) {
        printf("FAILED\n");
        return 1;
    }
    printf("OK\n");
    return 0;
}

static int mix(const char *ftw_s, const char *ph_s, const char *in, const char *out)
{
    const uint64_t ftw = strtoull(ftw_s, nullptr, 0), phase0 = strtoull(ph_s, nullptr, 0);
    FILE *f = fopen(in, "rb");
    if (!f)
        return 2;
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    std::vector<float> x(len), iq(2 * len);
    if (fread(x.data(), sizeof(float), len, f) != len)
        return 2;
    fclose(f);
    for (size_t j = 0; j < len; ++j)
        zoom_mix(x[j], phase0 + ftw * (uint64_t)j, iq[j], iq[len + j]);
    f = fopen(out, "wb");
    if (!f || fwrite(iq.data(), sizeof(float), 2 * len, f) != 2 * len)
        return 2;
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "check"))
        return check();
    if (argc == 6 && !strcmp(argv[1], "mix"))
        return mix(argv[2], argv[3], argv[4], argv[5]);
    fprintf(stderr, "usage: zoom_emul check | mix FTW PHASE0 IN.f32 OUT.f32\n");
    return 2;
}
