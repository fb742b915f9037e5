// Host emulation of stabilizer-stream_amd/csrc/cross_fft.h: runs the cross kernel's team transform, natural-order store and
// two-for-one separation lane by lane on the CPU and checks every separated bin of both segments of both channels, and the
// accumulated products, against a direct f64 DFT.  Channels of very different scale are used: a channel must not inherit
// the other's rounding.  Build: g++ -O2 -std=c++17 -I<csrc> cross_emul.cpp (tests/test_cross_host.py does).
#include "cross_fft.h"

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

static std::vector<cd> dft(const std::vector<double> &x)
{
    const int n = (int)x.size();
    std::vector<cd> X(n / 2 + 1);
    for (int k = 0; k <= n / 2; ++k) {
        cd s = 0;
        for (int j = 0; j < n; ++j)
            s += x[j] * std::polar(1.0, -2.0 * M_PI * (double)((long long)j * k % n) / n);
        X[k] = s;
    }
    return X;
}

template <int N>
static bool check(std::mt19937_64 &rng, double scale_y, bool b_live)
{
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<float> xa(N), xb(N), ya(N), yb(N);
    for (int j = 0; j < N; ++j) {
        xa[j] = (float)nd(rng);
        xb[j] = b_live ? (float)nd(rng) : 0.0f;
        ya[j] = (float)(scale_y * nd(rng));
        yb[j] = b_live ? (float)(scale_y * nd(rng)) : 0.0f;
    }
    std::vector<cf> zx(N), zy(N), fx(LdsFrame<N>::SIZE), fy(LdsFrame<N>::SIZE);
    for (int j = 0; j < N; ++j) {
        zx[j] = {xa[j], xb[j]};
        zy[j] = {ya[j], yb[j]};
    }
    team_fft<N>(zx, fx, tw);
    team_fft<N>(zy, fy, tw);
    auto D = [](const std::vector<float> &v) { return dft(std::vector<double>(v.begin(), v.end())); };
    const auto XA = D(xa), XB = D(xb), YA = D(ya), YB = D(yb);
    double nx = 0, ny = 0;
    for (int k = 0; k <= N / 2; ++k) {
        nx = std::max(nx, std::abs(XA[k]) + std::abs(XB[k]));
        ny = std::max(ny, std::abs(YA[k]) + std::abs(YB[k]));
    }
    double ex = 0, ey = 0, exx = 0, eyy = 0, exy = 0;
    for (int k = 0; k <= N / 2; ++k) {
        const int kn = (N - k) & (N - 1);
        cf a, b, c, d;
        separate(fx[LdsFrame<N>::at(k)], fx[LdsFrame<N>::at(kn)], a, b);
        separate(fy[LdsFrame<N>::at(k)], fy[LdsFrame<N>::at(kn)], c, d);
        ex = std::max({ex, std::abs(cd(a.re, a.im) - XA[k]) / nx, b_live ? std::abs(cd(b.re, b.im) - XB[k]) / nx : 0.0});
        ey = std::max({ey, std::abs(cd(c.re, c.im) - YA[k]) / ny, b_live ? std::abs(cd(d.re, d.im) - YB[k]) / ny : 0.0});
        float acc[4] = {0, 0, 0, 0};
        cross_bin<N>(k, fx.data(), fy.data(), b_live, acc);
        const double pxx = std::norm(XA[k]) + std::norm(XB[k]), pyy = std::norm(YA[k]) + std::norm(YB[k]);
        const cd pxy = std::conj(XA[k]) * YA[k] + std::conj(XB[k]) * YB[k];
        exx = std::max(exx, std::abs(acc[0] - pxx) / (nx * nx));
        eyy = std::max(eyy, std::abs(acc[1] - pyy) / (ny * ny));
        exy = std::max(exy, std::abs(cd(acc[2], acc[3]) - pxy) / (nx * ny));
    }
    // f32 transform: errors of a few eps (log2 N) of the channel's OWN scale
    const double tol = 2e-6;
    const bool ok = ex < tol && ey < tol && exx < tol && eyy < tol && exy < tol;
    printf("N=%5d scale_y=%-7g b_live=%d  sep err x %.2e y %.2e  |X|^2 %.2e |Y|^2 %.2e XY %.2e  %s\n", N, scale_y, (int)b_live, ex, ey,
           exx, eyy, exy, ok ? "ok" : "FAIL");
    return ok;
}

template <int N>
static bool check_all(std::mt19937_64 &rng)
{
    bool ok = true;
    for (double s : {1.0, 1e-4, 1e4})
        ok &= check<N>(rng, s, true);
    ok &= check<N>(rng, 1.0, false);
    return ok;
}

int main()
{
    std::mt19937_64 rng(12345);
    bool ok = true;
    ok &= check_all<64>(rng);
    ok &= check_all<128>(rng);
    ok &= check_all<256>(rng);
    ok &= check_all<512>(rng);
    ok &= check_all<1024>(rng);
    ok &= check_all<2048>(rng);
    ok &= check_all<4096>(rng);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
