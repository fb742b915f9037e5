// Host check of stabilizer-stream_amd/csrc/zoom_ampm_cross_fft.h: the AM/PM cross kernel's per-bin arithmetic -- the zoom cross
// object's eight values of bins k and (N - k) mod N and the two complementary products Z_a[k] Z_b[N-k], Z_a[N-k] Z_b[k] -- on the
// two frames the team transform of cross_fft.h leaves after store_natural, lane by lane as zoom_ampm_cross_kernel<N> walks its
// bins (k = t + TEAM r <= N/2, CrossBins<N>), against direct f64 DFTs of the two complex segments.
// N = 64 and 1024, random complex segments: amplitude 1 at three input scales, the EWMA amplitudes sqrt(w) the kernel puts on the
// samples down to 2^-50 (every row is bilinear in Z, so the weight never has to be applied to a product), and an inactive team (a
// segment of zeros adds exact zeros).
// Every (row, bin) of the twelve rows must be written exactly once; rows 8 ... 11 at bin k must be the products of FFT indices
// (k, kn) and (kn, k), kn = (N - k) mod N, which random data tells from any other pairing, and equal each other at k = 0 and N/2.
//
// Bounds: rows 0 ... 3 within 2e-6 nx^2 (tests/host/cross_emul.cpp's bound), rows 4 ... 11 within 4e-6 nx^2 (a sum of two
// products of that size), nx the largest |Z| of the two segments' bins: tests/host/zoom_ampm_emul.cpp's bounds for the same sums.
// Build: g++ -O2 -std=c++17 -I<csrc> zoom_ampm_cross_emul.cpp (tests/test_zoom_ampm_cross_host.py does, and once more with
// -fsanitize=address,undefined).
#include "zoom_ampm_cross_fft.h"

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
    constexpr int TEAM = FftPlan<N>::TEAM, H = N / 2 + 1, XB = CrossBins<N>::XBINS, R = ZXAMPM_ROWS;
    static_assert(CrossBins<N>::H == H, "the bins a thread owns are 0 ... N/2");
    static_assert(R == 12 && R % ZXAMPM_TURN == 0, "twelve rows, a whole number of turns");
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<cf> za(N), zb(N);
    for (auto *z : {&za, &zb})
        for (int j = 0; j < N; ++j) { // a team without a segment transforms zeros; the amplitude goes on the samples in f32
            const float re = (float)(scale * nd(rng)), im = (float)(scale * nd(rng));
            (*z)[j] = active ? cf{re * amp, im * amp} : cf{0.0f, 0.0f};
        }
    const auto fa = team_frame<N>(za, tw), fb = team_frame<N>(zb, tw);
    const auto A = dft(za), B = dft(zb);
    double nx = 0;
    for (int k = 0; k < N; ++k)
        nx = std::max({nx, std::abs(A[k]), std::abs(B[k])});
    // the twelve rows of a partial as the lanes' accumulators fill them: row c of bin k from acc[c] of the lane that owns k
    std::vector<float> part((size_t)R * H, -1.0f);
    std::vector<int> wrote((size_t)R * H, 0);
    for (int t = 0; t < TEAM; ++t)
        for (int r = 0; r < XB; ++r) {
            const int k = t + TEAM * r;
            if (k >= H)
                continue;
            if (xampm_partner<N>(k) != (N - k) % N)
                return false;
            float acc[R] = {};
            ampm_cross_bin<N>(k, fa.data(), fb.data(), acc);
            for (int c = 0; c < R; ++c) {
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
        const cd up = std::conj(A[k]) * B[k], lo = std::conj(A[kn]) * B[kn]; // the zoom cross object's sign; lower not conjugated
        const cd cab = A[k] * B[kn], cba = A[kn] * B[k];                      // no conjugate
        const double want[R] = {std::norm(A[k]), std::norm(A[kn]), std::norm(B[k]), std::norm(B[kn]), up.real(), lo.real(),
                                up.imag(),       lo.imag(),        cab.real(),      cab.imag(),       cba.real(), cba.imag()};
        for (int c = 0; c < R; ++c) {
            const float got = part[(size_t)c * H + k];
            if (!active) {
                ok = ok && got == 0.0f;
                continue;
            }
            const double err = std::fabs((double)got - want[c]) / (nx * nx);
            (c < 4 ? e1 : e2) = std::max(c < 4 ? e1 : e2, err);
            ok = ok && std::isfinite(got);
        }
        if (active && (k == 0 || k == N / 2)) // kn == k: upper and lower rows are one bin, and cab == cba
            for (int c = 0; c < 8; c += 2)
                ok = ok && part[(size_t)c * H + k] == part[(size_t)(c + 1) * H + k];
        if (active && (k == 0 || k == N / 2))
            ok = ok && part[(size_t)8 * H + k] == part[(size_t)10 * H + k] && part[(size_t)9 * H + k] == part[(size_t)11 * H + k];
    }
    worst.p = std::max(worst.p, e1);
    worst.c = std::max(worst.c, e2);
    ok = ok && e1 <= 2e-6 && e2 <= 4e-6;
    printf("N=%5d amp=%-9.3g active=%d scale=%-6g  auto %.2e  cross %.2e  %s\n", N, amp, (int)active, scale, e1, e2, ok ? "ok" : "FAIL");
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
    printf("zoom_ampm_cross N=%d worst %.3e bound %.1e (auto)\n", N, worst.p, 2e-6);
    printf("zoom_ampm_cross N=%d worst %.3e bound %.1e (cross)\n", N, worst.c, 4e-6);
    return ok;
}

int main()
{
    std::mt19937_64 rng(20261020);
    bool ok = true;
    ok &= check_all<64>(rng);
    ok &= check_all<1024>(rng);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
