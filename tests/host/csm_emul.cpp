// Host check of stabilizer-stream_amd/csrc/csm_fft.h: the matrix kernel's per-bin arithmetic (separate + every product of one bin
// of M channels) on frames made by the team transform of cross_fft.h, against a direct f64 DFT, for M = 2, 3, 4.  Channels
// 1e4 apart in scale: an entry S_ab is held to eps |X_a| |X_b|, its OWN scale.  The row layout (a M + a: S_aa; a < b: a M + b
// Re, b M + a Im) is checked as written, and M = 2 against cross_bin value for value.
// Build: g++ -O2 -std=c++17 -I<csrc> csm_emul.cpp (tests/test_csm_host.py does).
#include "csm_fft.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>
using namespace psdk;
using cd = std::complex<double>;

template <int N, int P>
static void passes(std::vector<std::vector<cf>> &regs, cf *frame, const std::vector<cf> &tw)
{
    for (int t = 0; t < FftPlan<N>::TEAM; ++t)
        xfft_pass<N, P>(t, regs[t].data(), frame, tw.data());
    if constexpr (P + 1 < FftPlan<N>::NPASS)
        passes<N, P + 1>(regs, frame, tw);
}

template <int N>
static void team_fft(const std::vector<cf> &z, cf *frame, const std::vector<cf> &tw)
{
    using P0 = PassInfo<N, 0>;
    constexpr int TEAM = FftPlan<N>::TEAM, E = FftPlan<N>::E;
    std::vector<std::vector<cf>> regs(TEAM, std::vector<cf>(E));
    for (int t = 0; t < TEAM; ++t)
        for (int i = 0; i < P0::NB; ++i)
            for (int m = 0; m < P0::R; ++m)
                regs[t][i * P0::R + m] = z[P0::elem(t, i, m)];
    passes<N, 0>(regs, frame, tw);
    for (int t = 0; t < TEAM; ++t)
        store_natural<N>(t, regs[t].data(), frame);
}

static std::vector<cd> dft(const std::vector<float> &x)
{
    const int n = (int)x.size();
    std::vector<cd> X(n / 2 + 1);
    for (int k = 0; k <= n / 2; ++k) {
        cd s = 0;
        for (int j = 0; j < n; ++j)
            s += (double)x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % n) / n);
        X[k] = s;
    }
    return X;
}

template <int N, int M>
static bool check(std::mt19937_64 &rng, bool b_live, bool spread)
{
    using S = CsmShape<N, M>;
    static_assert(S::XB * S::GS >= S::H && S::PG * S::GS == S::BLOCK && S::TEAMS * S::TEAM == S::BLOCK, "every bin has one owner");
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    const double scales[4] = {1.0, spread ? 1e-4 : 0.7, spread ? 1e4 : 1.3, spread ? 3e-2 : 0.9};
    constexpr int FR = LdsFrame<N>::SIZE;
    std::vector<cf> frames((size_t)M * FR);
    std::vector<std::vector<cd>> XA(M), XB(M);
    double norm[M];
    for (int c = 0; c < M; ++c) {
        std::vector<float> a(N), b(N);
        std::vector<cf> z(N);
        for (int j = 0; j < N; ++j) {
            a[j] = (float)(scales[c] * nd(rng));
            b[j] = b_live ? (float)(scales[c] * nd(rng)) : 0.0f;
            z[j] = {a[j], b[j]};
        }
        team_fft<N>(z, frames.data() + (size_t)c * FR, tw);
        XA[c] = dft(a);
        XB[c] = dft(b);
        norm[c] = 0;
        for (int k = 0; k <= N / 2; ++k)
            norm[c] = std::max(norm[c], std::abs(XA[c][k]) + std::abs(XB[c][k]));
    }
    double worst = 0;
    bool same2 = true;
    for (int k = 0; k <= N / 2; ++k) {
        float acc[M * M];
        for (int i = 0; i < M * M; ++i)
            acc[i] = 0.0f;
        csm_bin<N, M>(k, frames.data(), FR, b_live, acc);
        for (int a = 0; a < M; ++a)
            for (int b = a; b < M; ++b) {
                const cd want = std::conj(XA[a][k]) * XA[b][k] + std::conj(XB[a][k]) * XB[b][k];
                const cd got = a == b ? cd(acc[a * M + a], 0.0) : cd(acc[a * M + b], acc[b * M + a]);
                worst = std::max(worst, std::abs(got - want) / (norm[a] * norm[b]));
            }
        if constexpr (M == 2) { // the pair kernel's values, in the order xx, re, im, yy
            float p[4] = {0, 0, 0, 0};
            cross_bin<N>(k, frames.data(), frames.data() + FR, b_live, p);
            same2 = same2 && p[0] == acc[0] && p[1] == acc[3] && p[2] == acc[1] && p[3] == acc[2];
        }
    }
    const bool ok = worst < 2e-6 && same2; // a few eps (log2 N) of each entry's own scale, as cross_emul.cpp
    printf("N=%5d M=%d b_live=%d spread=%d  worst entry error %.2e  %s\n", N, M, (int)b_live, (int)spread, worst, ok ? "ok" : "FAIL");
    return ok;
}

template <int N>
static bool check_all(std::mt19937_64 &rng)
{
    bool ok = true;
    ok &= check<N, 2>(rng, true, true) && check<N, 2>(rng, false, false);
    ok &= check<N, 3>(rng, true, true) && check<N, 3>(rng, false, false);
    ok &= check<N, 4>(rng, true, true) && check<N, 4>(rng, false, false);
    return ok;
}

int main()
{
    std::mt19937_64 rng(424242);
    bool ok = true;
    ok &= check_all<64>(rng);
    ok &= check_all<128>(rng);
    ok &= check_all<256>(rng);
    ok &= check_all<512>(rng);
    ok &= check_all<1024>(rng);
    ok &= check_all<2048>(rng);
    ok &= check<4096, 2>(rng, true, true) && check<4096, 3>(rng, true, true);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
