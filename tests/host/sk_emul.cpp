// Host check of stabilizer-stream_amd/csrc/sk_fft.h: the spectral kurtosis kernel's per-bin arithmetic -- separation of a packed
// segment pair, P = |X|^2 and P^2 of both segments, the averaging weights and the row layout -- on the natural-order frame the
// team transform of cross_fft.h leaves, lane by lane as sk_kernel<N> walks it, against a direct f64 DFT.  N = 64 and 1024,
// random packed segment pairs, with weight 1 (boxcar) and with EWMA weights from sk_weight, among them 2^-100: its square and
// its reciprocal's product with a squared value leave f32, so an implementation that squares the weighted periodogram or
// divides by the weight fails here.  The odd last segment (b_live = false) is checked too.
//
// Bounds.  tests/host/cross_emul.cpp holds |X|^2 of a separated bin to 2e-6 of nx^2, nx the largest |Xa| + |Xb| over the bins
// (the separation's error is of the pair's scale).  P is that value: the same bound, times the weight.  P^2 doubles a relative
// error: 4e-6 of nx^4, times the weight.
// Build: g++ -O2 -std=c++17 -I<csrc> sk_emul.cpp (tests/test_sk_host.py does, and once more with -fsanitize=address,undefined).
#include "sk_fft.h"

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

// the team transform of z (pass-0 register slots loaded as the kernel loads them), natural order in `frame`
template <int N>
static void team_fft(const std::vector<cf> &z, std::vector<cf> &frame, const std::vector<cf> &tw)
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
        store_natural<N>(t, regs[t].data(), frame.data());
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

// the EWMA fields of a segment job, as sk_weight reads them
struct WJob {
    double log2_gamma;
    int nb, is_m1;
};

struct Worst {
    double p = 0, p2 = 0;
};

template <int N>
static bool check(std::mt19937_64 &rng, float wa, float wb, bool b_live, double scale, Worst &worst)
{
    constexpr int TEAM = FftPlan<N>::TEAM, H = N / 2 + 1, XB = CrossBins<N>::XBINS;
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<float> a(N), b(N);
    std::vector<cf> z(N), frame(LdsFrame<N>::SIZE);
    for (int j = 0; j < N; ++j) {
        a[j] = (float)(scale * nd(rng));
        b[j] = b_live ? (float)(scale * nd(rng)) : 0.0f;
        z[j] = {a[j], b[j]};
    }
    team_fft<N>(z, frame, tw);
    const auto A = dft(a), B = dft(b);
    double nx = 0;
    for (int k = 0; k < H; ++k)
        nx = std::max(nx, std::abs(A[k]) + std::abs(B[k]));
    // every lane's bins as the kernel owns them: k = t + TEAM r; the partial rows through sk_row_at
    std::vector<float> part((size_t)SK_ROWS * H, -1.0f);
    std::vector<int> seen((size_t)SK_ROWS * H, 0);
    for (int t = 0; t < TEAM; ++t)
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k >= H)
                continue;
            float acc[SK_ROWS] = {0.0f, 0.0f};
            sk_bin<N>(k, frame.data(), wa, wb, b_live, acc);
            for (int c = 0; c < SK_ROWS; ++c) {
                const int e = sk_row_at<N>(c, k);
                if (e < 0 || e >= SK_ROWS * H)
                    return false;
                part[e] = acc[c];
                ++seen[e];
            }
        }
    bool ok = std::all_of(seen.begin(), seen.end(), [](int s) { return s == 1; }); // one owner an element
    const double wmax = std::max((double)wa, b_live ? (double)wb : 0.0);
    double e1 = 0, e2 = 0;
    for (int k = 0; k < H; ++k) {
        const double pa = std::norm(A[k]), pb = b_live ? std::norm(B[k]) : 0.0;
        const double s1 = (double)wa * pa + (double)wb * pb, s2 = (double)wa * pa * pa + (double)wb * pb * pb;
        e1 = std::max(e1, std::fabs((double)part[k] - s1) / (wmax * nx * nx));         // row 0 at [0, H)
        e2 = std::max(e2, std::fabs((double)part[H + k] - s2) / (wmax * nx * nx * nx * nx)); // row 1 at [H, 2 H)
        ok = ok && std::isfinite(part[k]) && std::isfinite(part[H + k]) && (s2 == 0.0 || part[H + k] > 0.0f);
    }
    worst.p = std::max(worst.p, e1);
    worst.p2 = std::max(worst.p2, e2);
    ok = ok && e1 <= 2e-6 && e2 <= 4e-6;
    printf("N=%5d wa=%-9.3g wb=%-9.3g b_live=%d scale=%-6g  P %.2e  P^2 %.2e  %s\n", N, wa, wb, (int)b_live, scale, e1, e2,
           ok ? "ok" : "FAIL");
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
    const WJob boxcar{-1.0, 5, 7}; // every step still inside the boxcar regime: nb - max(step, is_m1) <= 0
    ok = ok && sk_weight(boxcar, 1) == 1.0f && sk_weight(boxcar, 5) == 1.0f;
    if (!ok)
        printf("N=%5d weights WRONG\n", N);
    Worst worst;
    ok &= check<N>(rng, 1.0f, 1.0f, true, 1.0, worst);
    ok &= check<N>(rng, 1.0f, 1.0f, true, 1e-3, worst);
    ok &= check<N>(rng, 1.0f, 1.0f, true, 1e3, worst);
    ok &= check<N>(rng, 1.0f, 1.0f, false, 1.0, worst);
    ok &= check<N>(rng, w_prev, w_new, true, 1.0, worst);
    ok &= check<N>(rng, w_mid, w_mid, true, 1.0, worst);
    ok &= check<N>(rng, w_old, w_old, true, 1.0, worst);
    ok &= check<N>(rng, w_old, w_old, true, 1e3, worst);
    ok &= check<N>(rng, w_old, 1.0f, false, 1.0, worst);
    printf("sk N=%d worst %.3e bound %.1e (P)\n", N, worst.p, 2e-6);
    printf("sk N=%d worst %.3e bound %.1e (P2)\n", N, worst.p2, 4e-6);
    return ok;
}

int main()
{
    std::mt19937_64 rng(20261018);
    bool ok = true;
    ok &= check_all<64>(rng);
    ok &= check_all<1024>(rng);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
