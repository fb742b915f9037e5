// Host check of stabilizer-stream_amd/csrc/zoom_ampm_fft.h: the AM/PM kernel's per-bin arithmetic -- |Z_k|^2, |Z_(N-k)|^2 and the
// complementary product Z_k Z_(N-k) -- on the frame the team transform of cross_fft.h leaves after store_natural, lane by lane as
// zoom_ampm_kernel<N> walks its bins (k = t + TEAM r <= N/2, CrossBins<N>), against a direct f64 DFT of the complex segment.
// N = 64 and 1024, random complex segments: amplitude 1 at three input scales, the EWMA amplitudes sqrt(w) the kernel puts on the
// samples down to 2^-50 (w = 2^-100: every row is bilinear in Z, so the weight never has to be applied to a product), and an
// inactive team (a segment of zeros adds exact zeros).
// Every (row, bin) of the four rows must be written exactly once; rows 2 and 3 at bin k must be the product of FFT indices k and
// (N - k) mod N (at k = 0 and N/2: the square of that bin), which random data tells from any other pairing.
//
// Bounds: rows 0 and 1 within 2e-6 nx^2 (tests/host/cross_emul.cpp's bound), rows 2 and 3 within 4e-6 nx^2 (a sum of two
// products of that size), nx the largest |Z| of the segment's bins.
// Build: g++ -O2 -std=c++17 -I<csrc> zoom_ampm_emul.cpp (tests/test_zoom_ampm_host.py does, and once more with
// -fsanitize=address,undefined).
#include "zoom_ampm_fft.h"

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

// the team transform of z (pass-0 register slots loaded as the kernel loads them), then every lane's store_natural: the frame as
// the kernel's readers find it, exactly LdsFrame<N>::SIZE elements
template <int N>
static std::vector<cf> team_frame(const std::vector<cf> &z, const std::vector<cf> &tw)
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
    for (int t = 0; t < TEAM; ++t)
        store_natural<N>(t, regs[t].data(), frame.data());
    return frame;
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

struct Worst {
    double p = 0, c = 0;
};

template <int N>
static bool check(std::mt19937_64 &rng, float amp, bool active, double scale, Worst &worst)
{
    constexpr int TEAM = FftPlan<N>::TEAM, H = N / 2 + 1, XB = CrossBins<N>::XBINS;
    static_assert(CrossBins<N>::H == H, "the bins a thread owns are 0 ... N/2");
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<cf> z(N);
    for (int j = 0; j < N; ++j) { // a team without a segment transforms zeros; the amplitude goes on the samples in f32
        const float re = (float)(scale * nd(rng)), im = (float)(scale * nd(rng));
        z[j] = active ? cf{re * amp, im * amp} : cf{0.0f, 0.0f};
    }
    const auto frame = team_frame<N>(z, tw);
    const auto Z = dft(z);
    double nx = 0;
    for (int k = 0; k < N; ++k)
        nx = std::max(nx, std::abs(Z[k]));
    // the four rows of a partial as the lanes' accumulators fill them: row c of bin k from acc[c] of the lane that owns k
    std::vector<float> part((size_t)ZAMPM_ROWS * H, -1.0f);
    std::vector<int> wrote((size_t)ZAMPM_ROWS * H, 0);
    for (int t = 0; t < TEAM; ++t)
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k >= H)
                continue;
            if (ampm_partner<N>(k) != (N - k) % N)
                return false;
            float acc[ZAMPM_ROWS] = {0.0f, 0.0f, 0.0f, 0.0f};
            ampm_bin<N>(k, frame.data(), acc);
            for (int c = 0; c < ZAMPM_ROWS; ++c) {
                part[(size_t)c * H + k] = acc[c];
                ++wrote[(size_t)c * H + k];
            }
        }
    bool ok = std::all_of(wrote.begin(), wrote.end(), [](int c) { return c == 1; });
    if (!ok)
        printf("N=%5d a (row, bin) written twice or never: WRONG\n", N);
    double e1 = 0, e2 = 0;
    for (int k = 0; k < H; ++k) {
        const int kn = (N - k) % N;
        const cd comp = Z[k] * Z[kn]; // no conjugate
        const double want[ZAMPM_ROWS] = {std::norm(Z[k]), std::norm(Z[kn]), comp.real(), comp.imag()};
        for (int c = 0; c < ZAMPM_ROWS; ++c) {
            const float got = part[(size_t)c * H + k];
            if (!active) {
                ok = ok && got == 0.0f;
                continue;
            }
            const double err = std::fabs((double)got - want[c]) / (nx * nx);
            (c < 2 ? e1 : e2) = std::max(c < 2 ? e1 : e2, err);
            ok = ok && std::isfinite(got);
        }
        if (active && (k == 0 || k == N / 2)) // the product is Z_k^2 there and both power rows are one bin
            ok = ok && part[k] == part[(size_t)H + k];
    }
    worst.p = std::max(worst.p, e1);
    worst.c = std::max(worst.c, e2);
    ok = ok && e1 <= 2e-6 && e2 <= 4e-6;
    printf("N=%5d amp=%-9.3g active=%d scale=%-6g  power %.2e  comp %.2e  %s\n", N, amp, (int)active, scale, e1, e2, ok ? "ok" : "FAIL");
    return ok;
}

template <int N>
static bool check_all(std::mt19937_64 &rng)
{
    bool ok = true;
    Worst worst;
    const float a_prev = (float)std::exp2(-0.5), a_mid = ldexpf(1.0f, -10), a_old = ldexpf(1.0f, -50);
    ok &= check<N>(rng, 1.0f, true, 1.0, worst);
    ok &= check<N>(rng, 1.0f, true, 1e-3, worst);
    ok &= check<N>(rng, 1.0f, true, 1e3, worst);
    ok &= check<N>(rng, a_prev, true, 1.0, worst);
    ok &= check<N>(rng, a_mid, true, 1.0, worst);
    ok &= check<N>(rng, a_old, true, 1.0, worst);
    ok &= check<N>(rng, a_old, true, 1e3, worst);
    ok &= check<N>(rng, 1.0f, false, 1.0, worst);
    ok &= check<N>(rng, a_old, false, 1.0, worst);
    printf("zoom_ampm N=%d worst %.3e bound %.1e (power)\n", N, worst.p, 2e-6);
    printf("zoom_ampm N=%d worst %.3e bound %.1e (comp)\n", N, worst.c, 4e-6);
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
