// Host side of stabilizer-stream_amd/csrc/iq_lo.h, the complex mixer of the IQ cascade (the same source the device runs).
//   iq_emul mix FTW PHASE0 I.f32 Q.f32 OUT.f32   the mixer: complex sample j of (I, Q) with phase PHASE0 + FTW j mod 2^64; OUT holds
//                                                every I', then every Q' (what iq_mix_kernel stores into the two stage-0 streams)
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I<csrc> iq_emul.cpp (tests/test_iq_host.py does).
#include "iq_lo.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace psdk;

static bool read_f32(const char *path, std::vector<float> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return false;
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f) / sizeof(float);
    fseek(f, 0, SEEK_SET);
    v.resize(len);
    const bool ok = fread(v.data(), sizeof(float), len, f) == len;
    fclose(f);
    return ok;
}

static int mix(const char *ftw_s, const char *ph_s, const char *in_i, const char *in_q, const char *out)
{
    const uint64_t ftw = strtoull(ftw_s, nullptr, 0), phase0 = strtoull(ph_s, nullptr, 0);
    std::vector<float> xi, xq;
    if (!read_f32(in_i, xi) || !read_f32(in_q, xq) || xi.size() != xq.size())
        return 2;
    const size_t len = xi.size();
    std::vector<float> iq(2 * len);
    for (size_t j = 0; j < len; ++j)
        iq_mix(xi[j], xq[j], phase0 + ftw * (uint64_t)j, iq[j], iq[len + j]);
    FILE *f = fopen(out, "wb");
    if (!f || fwrite(iq.data(), sizeof(float), 2 * len, f) != 2 * len)
        return 2;
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "mix"))
        return mix(argv[2], argv[3], argv[4], argv[5], argv[6]);
    fprintf(stderr, "usage: iq_emul mix FTW PHASE0 I.f32 Q.f32 OUT.f32\n");
    return 2;
}
