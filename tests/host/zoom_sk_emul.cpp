// Host check of stabilizer-stream_amd/csrc/zoom_sk_fft.h: the zoom spectral kurtosis kernel's per-slot arithmetic -- P = |Z|^2,
// (w P) and (w P) P of the sixteen bins a thread holds after the team transform of cross_fft.h -- and the (slot -> row, bin) map
// of the four partial rows, lane by lane as zoom_sk_kernel<N> walks them, against a direct f64 DFT of the complex segment.
// N = 64 and 1024, random complex segments: weight 1 at three input scales, the EWMA weights sk_weight gives for gamma = 1/2 down
// to 2^-100 (its square and its reciprocal leave f32, so squaring the weighted periodogram or dividing by the weight fails here),
// and an inactive team (a segment of zeros under any weight adds exact zeros).
// Every (row, bin) of the four rows must be written exactly once, upper k from FFT index k and lower k from (N - k) mod N.
//
// Bounds: those tests/host/sk_emul.cpp holds -- P within 2e-6 of w nx^2, P^2 within 4e-6 of w nx^4, nx the largest |Z| of the
// segment's bins.
// Build: g++ -O2 -std=c++17 -I<csrc> zoom_sk_emul.cpp (tests/test_zoom_sk_host.py does, and once more with
// -fsanitize=address,undefined).
#include "segment_kernel.h"
#include "zoom_sk_fft.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>
using namespace psdk;
using cd = std::complex<double>;

template <int N, int P>
static void passes(std::vector<std::vector<cf>> &regs, std::vector<cf> &frame, const std::vector<cf> &tw)
{
    for (int t = 0; t < FftPlan<N>::TEAM; ++t)
        xfft_pass<N, P>(t, regs[t].data(), frame.data(), tw.data());
    if constexpr (P + 1 < FftPlan<N>::NPASS)
        passes<N, P + 1>(regs, frame, tw);
}

// the team transform of z (pass-0 register slots loaded as the kernel loads them); the bins stay in the lanes' registers, slot s
// of lane t holding bin freq_of_slot<N>(t, s), as cross_channel<N, true, true> hands them back
template <int N>
static std::vector<std::vector<cf>> team_fft(const std::vector<cf> &z, const std::vector<cf> &tw)
{
    using P0 = PassInfo<N, 0>;
    constexpr int TEAM = FftPlan<N>::TEAM, E = FftPlan<N>::E;
    std::vector<std::vector<cf>> regs(TEAM, std::vector<cf>(E));
    std::vector<cf> frame(LdsFrame<N>::SIZE);
    for (int t = 0; t < TEAM; ++t)
        for (int i = 0; i < P0::NB; ++i)
            for (int m = 0; m < P0::R; ++m)
                regs[t][i * P0::R + m] = z[P0::elem(t, i, m)];
    passes<N, 0>(regs, frame, tw);
    return regs;
}

static std::vector<cd> dft(const std::vector<cf> &z)
{
    const int n = (int)z.size();
    std::vector<cd> Z(n);
    for (int k = 0; k < n; ++k) {
        cd s = 0;
        for (int j = 0; j < n; ++j)
            s += cd(z[j].re, z[j].im) * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % n) / n);
        Z[k] = s;
    }
    return Z;
}

// the EWMA fields of a segment job, as sk_weight reads them
struct WJob {
    double log2_gamma;
    int nb, is_m1;
};

struct Worst {
    double p = 0, p2 = 0;
};

template <int N>
static bool check(std::mt19937_64 &rng, float w, bool active, double scale, Worst &worst)
{
    constexpr int TEAM = FftPlan<N>::TEAM, E = FftPlan<N>::E, H = N / 2 + 1;
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<cf> z(N);
    for (int j = 0; j < N; ++j) // a team without a segment transforms zeros (cross_channel drops what it loaded)
        z[j] = active ? cf{(float)(scale * nd(rng)), (float)(scale * nd(rng))} : cf{0.0f, 0.0f};
    const auto regs = team_fft<N>(z, tw);
    const auto Z = dft(z);
    double nx = 0;
    for (int k = 0; k < N; ++k)
        nx = std::max(nx, std::abs(Z[k]));
    // one team's region of the frames' LDS as the kernel fills it: [ZSK_Q][N] floats, moment q of bin k at q N + k; `from` is
    // the FFT index the value was computed from
    std::vector<float> fq((size_t)ZSK_Q * N, -1.0f);
    std::vector<int> from((size_t)ZSK_Q * N, -1), wrote((size_t)ZSK_Q * N, 0);
    for (int t = 0; t < TEAM; ++t)
        for (int s = 0; s < E; ++s) {
            float a1 = 0.0f, a2 = 0.0f;
            zoom_sk_slot(regs[t][s], w, a1, a2);
            const int k = freq_of_slot<N>(t, s);
            if (k < 0 || k >= N)
                return false;
            fq[k] = a1;
            fq[N + k] = a2;
            from[k] = from[N + k] = k;
            ++wrote[k];
            ++wrote[N + k];
        }
    bool ok = std::all_of(wrote.begin(), wrote.end(), [](int c) { return c == 1; });
    // the partial rows as the kernel's combine loop reads them
    std::vector<float> part((size_t)ZSK_ROWS * H, -1.0f);
    std::vector<int> seen((size_t)ZSK_ROWS * H, 0), src((size_t)ZSK_ROWS * H, -1);
    for (int e = 0; e < ZSK_ROWS * H; ++e) {
        const int row = e / H;
        const int k = two_sided_bin<N>(row, e - row * H);
        const int q = two_sided_value(row);
        if (k < 0 || k >= N || q < 0 || q >= ZSK_Q)
            return false;
        part[e] = fq[(size_t)q * N + k];
        src[e] = from[(size_t)q * N + k];
        ++seen[e];
    }
    ok = ok && std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; });
    double e1 = 0, e2 = 0;
    for (int row = 0; row < ZSK_ROWS; ++row)
        for (int k = 0; k < H; ++k) {
            const int idx = (row & 1) ? (N - k) % N : k; // upper k from index k, lower k from (N - k) mod N
            const bool second = row >= 2;                // rows 0, 1: S1; rows 2, 3: S2
            const float got = part[(size_t)row * H + k];
            if (src[(size_t)row * H + k] != idx) {
                printf("N=%5d row %d bin %d from FFT index %d, not %d: WRONG\n", N, row, k, src[(size_t)row * H + k], idx);
                ok = false;
            }
            const double p = std::norm(Z[idx]);
            if (!active) {
                ok = ok && got == 0.0f;
                continue;
            }
            const double want = second ? (double)w * p * p : (double)w * p;
            const double err = std::fabs((double)got - want) / ((double)w * (second ? nx * nx * nx * nx : nx * nx));
            (second ? e2 : e1) = std::max(second ? e2 : e1, err);
            ok = ok && std::isfinite(got) && (want == 0.0 || got > 0.0f);
        }
    worst.p = std::max(worst.p, e1);
    worst.p2 = std::max(worst.p2, e2);
    ok = ok && e1 <= 2e-6 && e2 <= 4e-6;
    printf("N=%5d w=%-9.3g active=%d scale=%-6g  P %.2e  P^2 %.2e  %s\n", N, w, (int)active, scale, e1, e2, ok ? "ok" : "FAIL");
    return ok;
}

template <int N>
static bool check_all(std::mt19937_64 &rng)
{
    bool ok = true;
    // the weights as the kernel gets them: gamma = 1/2, a job of 101 segments behind the boxcar regime
    const WJob job{-1.0, 101, 0};
    const float w_new = sk_weight(job, 101), w_prev = sk_weight(job, 100), w_mid = sk_weight(job, 81), w_old = sk_weight(job, 1);
    ok = ok && w_new == 1.0f && w_prev == 0.5f && w_mid == ldexpf(1.0f, -20) && w_old == ldexpf(1.0f, -100);
    ok = ok && w_old * w_old == 0.0f;               // its square is gone in f32 ...
    ok = ok && !std::isfinite(1.0f / w_old / w_old); // ... and so is what a division by it would need
    ok = ok && sk_weight(job, 102) == 1.0f;          // a team past the job's last segment: weight 1 on zeros
    if (!ok)
        printf("N=%5d weights WRONG\n", N);
    Worst worst;
    ok &= check<N>(rng, 1.0f, true, 1.0, worst);
    ok &= check<N>(rng, 1.0f, true, 1e-3, worst);
    ok &= check<N>(rng, 1.0f, true, 1e3, worst);
    ok &= check<N>(rng, w_prev, true, 1.0, worst);
    ok &= check<N>(rng, w_mid, true, 1.0, worst);
    ok &= check<N>(rng, w_old, true, 1.0, worst);
    ok &= check<N>(rng, w_old, true, 1e3, worst);
    ok &= check<N>(rng, 1.0f, false, 1.0, worst);
    ok &= check<N>(rng, w_old, false, 1.0, worst);
    printf("zoom_sk N=%d worst %.3e bound %.1e (P)\n", N, worst.p, 2e-6);
    printf("zoom_sk N=%d worst %.3e bound %.1e (P2)\n", N, worst.p2, 4e-6);
    return ok;
}

int main()
{
    std::mt19937_64 rng(20261019);
    bool ok = true;
    ok &= check_all<64>(rng);
    ok &= check_all<1024>(rng);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
