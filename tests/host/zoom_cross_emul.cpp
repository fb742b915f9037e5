// Host check of stabilizer-stream_amd/csrc/zoom_cross_fft.h: the zoom cross kernel's per-bin arithmetic on the registers the team
// transform of cross_fft.h leaves (no natural-order store, as the kernel), against a direct f64 DFT of the same complex inputs,
// for N = 64 and 1024.  Two channels of random complex samples, channel b = 0.6 a + noise at another scale, so S_ab is neither
// 0 nor sqrt(S_aa S_bb).  Each of the four values of every bin j = 0 ... N - 1 is compared with the f64 product, and the eight
// rows are then read through two_sided_bin / two_sided_value (segment_kernel.h) and compared with the row table of include/psdcascade.h
// written out here: S_aa, S_bb, Re S_ab, Im S_ab, each upper (bin k) and lower (bin (N - k) mod N, not conjugated).
//
// Bound.  With eps = 2^-23 and R_a, R_b the rms of |Z_a|, |Z_b| over the bins (what an averaged S_aa, S_bb of this input reads:
// sqrt(S_aa S_bb) = R_a R_b), a value's error is at most |e_a| |Z_b| + |Z_a| |e_b| + the product's own rounding.  The transform's
// error e of a bin is the sum of about 2 N log2 N roundings of at most eps / 2 of values of the bins' scale: a standard
// deviation of about 0.6 eps sqrt(log2 N) R; five deviations at the worst of 4 N values, against |Z| <= 4 R (Rayleigh, N bins),
// give 2 x 3 eps sqrt(log2 N) R x 4 R = 24 sqrt(log2 N) eps R_a R_b: 76 eps at N = 1024.  Asserted: 8 log2 N eps R_a R_b
// (48 eps at N = 64, 80 eps at N = 1024) for every value; the auto values use R_a R_a and R_b R_b.
// Build: g++ -O2 -std=c++17 -I<csrc> zoom_cross_emul.cpp (tests/test_zoom_cross_host.py does).
#include "segment_kernel.h"
#include "zoom_cross_fft.h"

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

// the team transform of z: regs[t][s] is bin freq_of_slot<N>(t, s), as cross_channel<N, true, true> hands it back
template <int N>
static std::vector<std::vector<cf>> team_fft(const std::vector<cf> &z, const std::vector<cf> &tw)
{
    using P0 = PassInfo<N, 0>;
    constexpr int TEAM = FftPlan<N>::TEAM, E = FftPlan<N>::E;
    std::vector<cf> frame(LdsFrame<N>::SIZE);
    std::vector<std::vector<cf>> regs(TEAM, std::vector<cf>(E));
    for (int t = 0; t < TEAM; ++t)
        for (int i = 0; i < P0::NB; ++i)
            for (int m = 0; m < P0::R; ++m)
                regs[t][i * P0::R + m] = z[P0::elem(t, i, m)];
    passes<N, 0>(regs, frame.data(), tw);
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

template <int N>
static bool check(std::mt19937_64 &rng, double scale_b)
{
    constexpr int TEAM = FftPlan<N>::TEAM, E = FftPlan<N>::E, H = N / 2 + 1;
    static_assert(E == 16 && TEAM * E == N, "sixteen bins a thread");
    std::normal_distribution<double> nd;
    std::vector<cf> tw(N);
    for (int j = 0; j < N; ++j)
        tw[j] = {(float)cos(-2.0 * M_PI * j / N), (float)sin(-2.0 * M_PI * j / N)};
    std::vector<cf> za(N), zb(N);
    for (int j = 0; j < N; ++j) {
        za[j] = {(float)nd(rng), (float)nd(rng)};
        zb[j] = {(float)(scale_b * (0.6 * za[j].re + 0.8 * nd(rng))), (float)(scale_b * (0.6 * za[j].im + 0.8 * nd(rng)))};
    }
    const auto ra = team_fft<N>(za, tw), rb = team_fft<N>(zb, tw);
    const auto ZA = dft(za), ZB = dft(zb);
    double pa = 0, pb = 0;
    for (int j = 0; j < N; ++j) {
        pa += std::norm(ZA[j]) / N;
        pb += std::norm(ZB[j]) / N;
    }
    const double Ra = sqrt(pa), Rb = sqrt(pb);
    const double scale[ZCROSS_Q] = {Ra * Ra, Rb * Rb, Ra * Rb, Ra * Rb};
    // the kernel's accumulators: acc[q][slot] of every thread, from zero, one segment
    std::vector<float> val((size_t)ZCROSS_Q * N, 0.0f); // val[q N + bin]
    std::vector<int> seen(N, 0);
    for (int t = 0; t < TEAM; ++t) {
        float acc[ZCROSS_Q * E] = {};
        for (int s = 0; s < E; ++s)
            zoom_cross_bin(ra[t][s], rb[t][s], acc + s, E);
        for (int s = 0; s < E; ++s) {
            const int bin = freq_of_slot<N>(t, s);
            ++seen[bin];
            for (int q = 0; q < ZCROSS_Q; ++q)
                val[(size_t)q * N + bin] = acc[q * E + s];
        }
    }
    bool ok = true;
    double worst[ZCROSS_Q] = {0, 0, 0, 0};
    const double eps = ldexp(1.0, -23);
    for (int j = 0; j < N; ++j) {
        ok = ok && seen[j] == 1; // every bin has one owner
        const cd x = std::conj(ZA[j]) * ZB[j];
        const double want[ZCROSS_Q] = {std::norm(ZA[j]), std::norm(ZB[j]), x.real(), x.imag()};
        for (int q = 0; q < ZCROSS_Q; ++q)
            worst[q] = std::max(worst[q], std::fabs((double)val[(size_t)q * N + j] - want[q]) / (eps * scale[q]));
    }
    // the rows, as the kernel's last loop reads them, against the table of the header
    bool rows_ok = true;
    for (int row = 0; row < ZCROSS_ROWS; ++row)
        for (int k = 0; k < H; ++k) {
            const float got = val[(size_t)two_sided_value(row) * N + two_sided_bin<N>(row, k)];
            const int j = (row % 2 == 0) ? k : (N - k) % N; // upper: bin k; lower: bin N - k
            const int q = row / 2;                          // rows 0, 1 S_aa; 2, 3 S_bb; 4, 5 Re S_ab; 6, 7 Im S_ab
            rows_ok = rows_ok && got == val[(size_t)q * N + j];
        }
    const double bound = 8.0 * log2((double)N);
    const double w = *std::max_element(worst, worst + ZCROSS_Q);
    ok = ok && rows_ok && w <= bound;
    printf("N=%5d scale_b=%g  worst error in eps sqrt(S_aa S_bb): S_aa %.2f  S_bb %.2f  Re S_ab %.2f  Im S_ab %.2f  (bound %.0f)  rows %s  %s\n",
           N, scale_b, worst[0], worst[1], worst[2], worst[3], bound, rows_ok ? "ok" : "WRONG", ok ? "ok" : "FAIL");
    printf("zoom_cross N=%d worst %.3f bound %.1f\n", N, w, bound);
    return ok;
}

int main()
{
    std::mt19937_64 rng(20261017);
    bool ok = true;
    ok &= check<64>(rng, 1.0);
    ok &= check<64>(rng, 1e-4);
    ok &= check<1024>(rng, 1.0);
    ok &= check<1024>(rng, 1e4);
    printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
