// bank_var_check.cpp -- csrc/bank_var.h on the CPU: the limit search, the exact fold, the terms and the sum in bank_var_kernel's
// order (bank_var_row_host), over the job table (VarJobSrc) and over the stitched row (VarRowSrc).  Stand-alone (no library, no
// device):
//
//   bank_var_check            built-in cases; asserts
//   bank_var_check IN OUT     cases from IN (written by tests/test_bank_var_host.py, which gets the Breaks from the library's
//                             host-only stitch); rows, frequencies and variances to OUT
//
// IN:  u32 cases; a case: u32 n, stages, breaks, vars, taus, 0; f32 nenbw, power; u64 count64[stages]; psdc_break[breaks];
//      f32 spectra[stages][n/2 + 1]; {i32 x_exp, sinx_exp; f32 clip; u32 dc_cut}[vars]; f32 tau[taus]
// OUT: a case: u64 L; f32 psd[L]; f32 freq[L]; f64 var[vars][taus]
#include "../../include/psdcascade.h"
#include "bank_var.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace psdk;

static long checks = 0;
#define CHECK(c)                                                                   \
    do {                                                                           \
        ++checks;                                                                  \
        if (!(c)) {                                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);                    \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

static float gain(uint32_t n, uint64_t count, float nenbw, float power) { return (float)((uint64_t)(n / 2u) * count) * nenbw * power; }

struct Bank { // one row of a bank: its accumulators, its jobs and the row they stitch to
    std::vector<std::vector<float>> acc;
    std::vector<BankJob> jobs;
    std::vector<float> psd, freq;
    uint32_t len = 0;
};

static void make_row(Bank &b, uint32_t n, const std::vector<uint64_t> &count64, const std::vector<psdc_break> &breaks,
                     const std::vector<float> &spectra, float nenbw, float power)
{
    const size_t bins = n / 2 + 1;
    b.acc.resize(count64.size());
    for (size_t s = 0; s < b.acc.size(); ++s) // memory of its own a stage: the sanitizer sees a read past a row
        b.acc[s].assign(spectra.begin() + s * bins, spectra.begin() + (s + 1) * bins);
    const BankRow r = bank_row_jobs(
        breaks.data(), breaks.size(), 0, b.jobs, [&](uint32_t s) { return (const float *)b.acc[s].data(); },
        [&](uint32_t s) { return gain(n, count64[s], nenbw, power); });
    b.len = r.len;
    for (const BankJob &j : b.jobs)
        for (uint32_t k = j.bins_start; k < j.bins_end; ++k) {
            b.psd.push_back(bank_psd(j, k));
            b.freq.push_back(bank_freq(j, k));
        }
    CHECK(b.psd.size() == b.len);
}

// the definition in sequence: skip dc_cut, take while f <= lim, fold the trapezoids.  *sum_abs = the sum of |t|, *E_out = E
static double sequential(const float *p, const float *f, size_t L, const VarDesc &d, float tau, double *sum_abs, size_t *E_out)
{
    const float lim = d.clip / tau;
    double sum = 0.0, a1 = 0.0, f1 = 0.0, abs_sum = 0.0;
    size_t e = d.dc_cut;
    for (; e < L; ++e) {
        if (!(f[e] <= lim))
            break;
        const double x = (double)f[e] * (double)tau, w = M_PI * x;
        double r = fmod(x, 2.0), sign = 1.0;
        if (r > 1.0) {
            r -= 1.0;
            sign = -1.0;
        }
        if (r > 0.5)
            r = 1.0 - r;
        const double s = sign * sin(M_PI * r);
        const double a = (((double)p[e] * (double)f[e]) * (double)f[e]) * (var_powi(s, d.sinx_exp) * var_powi(w, d.x_exp));
        const double t = (a + a1) * ((double)f[e] - f1);
        sum += t;
        abs_sum += fabs(t);
        a1 = a;
        f1 = f[e];
    }
    *sum_abs = abs_sum;
    *E_out = e < L ? e : (d.dc_cut < L ? L : d.dc_cut);
    return sum;
}

static bool close_to(double got, double want, double sum_abs, size_t L)
{
    if (std::isnan(want) || std::isnan(got))
        return std::isnan(want) && std::isnan(got);
    return fabs(got - want) <= (double)(L + 64) * ldexp(1.0, -52) * sum_abs;
}

// both accessors give the same bits; each result within the bound of the sequential fold
static std::vector<double> both(const Bank &b, const std::vector<VarDesc> &vars, const std::vector<float> &taus)
{
    const uint32_t nv = (uint32_t)vars.size(), nt = (uint32_t)taus.size();
    std::vector<double> by_jobs((size_t)nv * nt, -1.0), by_rows((size_t)nv * nt, -2.0);
    bank_var_row_host(VarJobSrc(b.jobs.data(), (uint32_t)b.jobs.size(), b.len), vars.data(), nv, taus.data(), nt, by_jobs.data());
    bank_var_row_host(VarRowSrc(b.psd.data(), b.freq.data(), b.len), vars.data(), nv, taus.data(), nt, by_rows.data());
    CHECK(memcmp(by_jobs.data(), by_rows.data(), sizeof(double) * nv * nt) == 0);
    for (uint32_t v = 0; v < nv; ++v)
        for (uint32_t j = 0; j < nt; ++j) {
            double sum_abs = 0.0;
            size_t E = 0;
            const double want = sequential(b.psd.data(), b.freq.data(), b.len, vars[v], taus[j], &sum_abs, &E);
            CHECK(close_to(by_jobs[(size_t)v * nt + j], want, sum_abs, b.len));
        }
    return by_jobs;
}

static const VarDesc AVAR{-2, 4, FLT_MAX, 2}, MVAR{-4, 6, FLT_MAX, 2}, FVAR{-2, 4, 1.0f, 2};

// A row on which every sum is exact: sinx_exp = x_exp = 0 make the term factor 1.0, p a small integer and f[e] = e + 1 make every
// a[e] and t[e] an integer below 2^53.  The kernel's order must then give the sequential sum exactly: an element of [dc_cut, E) left
// out, or one taken twice, changes it.
static void exact_rows()
{
    for (uint32_t L : {1u, 2u, 63u, 64u, 65u, 255u, 256u, 257u, 300u, 512u, 777u}) {
        std::vector<float> p(L), f(L);
        for (uint32_t e = 0; e < L; ++e) {
            p[e] = (float)(1 + (e * 7919u) % 1000u);
            f[e] = (float)(e + 1);
        }
        for (uint32_t dc : {0u, 1u, 2u, 64u, 255u, 256u, L - 1, L, L + 5}) {
            // tau = 1 and clip = E_want exactly: f[e] = e + 1 <= E_want holds for e < E_want
            for (uint32_t E_want : {0u, 1u, dc, dc + 1, 64u, 256u, 257u, L - 1, L, L + 9}) {
                const VarDesc d{0, 0, (float)E_want, dc};
                const float tau = 1.0f;
                double out = -1.0, sum_abs = 0.0;
                size_t E = 0;
                bank_var_row_host(VarRowSrc(p.data(), f.data(), L), &d, 1, &tau, 1, &out);
                const double want = sequential(p.data(), f.data(), L, d, tau, &sum_abs, &E);
                CHECK(out == want);
                CHECK(E == (dc >= L ? dc : (E_want < dc ? dc : (E_want < L ? E_want : L))));
                if (dc >= L || E_want <= dc)
                    CHECK(out == 0.0);
                else
                    CHECK(out > 0.0);
            }
        }
        // one element alone holds power: it shows in t[e0] and t[e0 + 1], once each
        if (L == 300)
            for (uint32_t e0 = 0; e0 < L; ++e0) {
                std::vector<float> q(L, 0.0f);
                q[e0] = 3.0f;
                const VarDesc d{0, 0, FLT_MAX, 2};
                const float tau = 1.0f;
                double out = -1.0;
                bank_var_row_host(VarRowSrc(q.data(), f.data(), L), &d, 1, &tau, 1, &out);
                const double a = 3.0 * (double)(e0 + 1) * (double)(e0 + 1);
                // f[e] - f[e-1] = 1, but at e = dc_cut the difference is f[dc_cut] - 0 = 3
                const double want = e0 < 2 ? 0.0 : (e0 == 2 ? 3.0 * a : a) + (e0 + 1 < L ? a : 0.0);
                CHECK(out == want);
            }
    }
}

static void fold()
{
    // var_sinpi's reduction IS fmod, and the fold agrees with the sine of the reduced argument bit for bit
    for (int i = 0; i < 200000; ++i) {
        const double x = ldexp((double)(float)(0.37 * i + 1e-3 * (i % 17)), (i % 40) - 20) * (double)(float)(1.0 + 0.001 * (i % 7));
        double r = fmod(x, 2.0), sign = 1.0;
        CHECK(x - 2.0 * trunc(0.5 * x) == r);
        if (r > 1.0) {
            r -= 1.0;
            sign = -1.0;
        }
        if (r > 0.5)
            r = 1.0 - r;
        CHECK(M_PI * r >= 0.0 && M_PI * r <= 1.5707963267948968);
        CHECK(var_sinpi(x) == sign * sin(M_PI * r));
    }
    CHECK(var_sinpi(0.0) == 0.0 && var_sinpi(0.5) == 1.0 && var_sinpi(1.5) == -1.0 && var_sinpi(1e15) == 0.0);
    CHECK(var_powi(3.0, 4) == 81.0 && var_powi(2.0, -2) == 0.25 && var_powi(5.0, 0) == 1.0 && var_powi(2.0, 16) == 65536.0);
    CHECK(std::isinf(var_powi(0.0, -2)));
}

static void builtin()
{
    fold();
    exact_rows();
    // the reference's test vector (src/var.rs): 0.13478442 there in f32, 0.134782674 by the definition
    {
        const float p[5] = {1000.0f, 100.0f, 1.2f, 3.4f, 5.6f}, f[5] = {0.0f, 1.0f, 3.0f, 6.0f, 9.0f}, tau = 2.7f;
        double out = 0.0, sum_abs = 0.0;
        size_t E = 0;
        bank_var_row_host(VarRowSrc(p, f, 5), &AVAR, 1, &tau, 1, &out);
        CHECK(fabs(out - 0.134782674) <= 1e-9 && fabs(out - 0.13478442) <= 1e-5);
        CHECK(close_to(out, sequential(p, f, 5, AVAR, tau, &sum_abs, &E), sum_abs, 5) && E == 5);
        // dc_cut = 0 on a row that starts at f = 0: 0 * inf = NaN, and it stays
        const VarDesc d0{-2, 4, FLT_MAX, 0};
        bank_var_row_host(VarRowSrc(p, f, 5), &d0, 1, &tau, 1, &out);
        CHECK(std::isnan(out));
    }
    // three stages of n = 64 as the stitch lays them out with the default options (bins [0, 25), [4, 25), [4, 33): f rises along the
    // row) and with keep_overlap (bins [0, 33), [1, 33), [1, 33): f steps back at both seams)
    for (int overlap = 0; overlap < 2; ++overlap) {
        const uint64_t lo[2][3] = {{0, 4, 4}, {0, 1, 1}}, hi[2][3] = {{25, 25, 33}, {33, 33, 33}};
        std::vector<psdc_break> breaks;
        uint64_t start = 0;
        for (int i = 0; i < 3; ++i) {
            psdc_break b{};
            b.start = start;
            b.include = 1;
            b.bins_start = lo[overlap][i];
            b.bins_end = hi[overlap][i];
            b.fft_size = 64;
            b.decimation = 1ull << (3 * (2 - i));
            breaks.push_back(b);
            start += b.bins_end - b.bins_start;
        }
        std::vector<float> spectra(3 * 33);
        for (size_t k = 0; k < spectra.size(); ++k)
            spectra[k] = 1.0f + (float)(k % 7);
        Bank b;
        make_row(b, 64, {100, 12, 1}, breaks, spectra, 1.5f, 0.25f);
        const uint32_t L = b.len, seam = (uint32_t)(hi[overlap][0] - lo[overlap][0]);
        CHECK(L == start && b.freq[0] == 0.0f && b.freq[L - 1] == 0.5f);
        CHECK(overlap ? b.freq[seam] < b.freq[seam - 1] : b.freq[seam] > b.freq[seam - 1]);
        // with clip = 1, tau = 1 / lim: E at dc_cut (lim below f[2]), inside the first job, on the seam (where f rises across it: behind
        // a step back the seam cannot be the first violation), at L, and no limit at all
        const float f2 = b.freq[2], f10 = b.freq[10], fs = b.freq[seam - 1];
        const std::vector<float> taus = {1.0f / (0.5f * f2), 1.0f / (0.5f * (f10 + b.freq[11])), overlap ? 1.0f / (0.5f * (f10 + b.freq[11])) : 1.0f / (0.5f * (fs + b.freq[seam])), 2.0f, 0.5f,
                                         2.7f, 64.0f};
        const size_t E_want[5] = {2, 11, overlap ? 11 : seam, L, L};
        for (int j = 0; j < 5; ++j) {
            double sum_abs = 0.0;
            size_t E = 0;
            sequential(b.psd.data(), b.freq.data(), L, FVAR, taus[j], &sum_abs, &E);
            CHECK(E == E_want[j]);
            // E as the kernel finds it: the limit walk of 256 threads, then the minimum
            const float lim[VAR_MAX_VARS][VAR_TAU_TILE] = {{FVAR.clip / taus[j], FVAR.clip / taus[j], FVAR.clip / taus[j], FVAR.clip / taus[j]}};
            uint32_t least = L;
            for (uint32_t t = 0; t < VAR_THREADS; ++t) {
                uint32_t first[VAR_MAX_VARS][VAR_TAU_TILE];
                for (auto &row : first)
                    for (uint32_t &x : row)
                        x = L;
                var_limit_walk(VarJobSrc(b.jobs.data(), (uint32_t)b.jobs.size(), L), t, VAR_THREADS, &FVAR, 1, lim, first);
                CHECK(first[0][0] == first[0][3]);
                least = first[0][0] < least ? first[0][0] : least;
            }
            CHECK(least == E_want[j]);
        }
        const std::vector<double> r = both(b, {AVAR, MVAR, FVAR}, taus);
        CHECK(r[2 * taus.size() + 0] == 0.0 && r[2 * taus.size() + 1] > 0.0 && r[5] > 0.0 && r[taus.size() + 5] > 0.0);
        if (overlap) { // the elements behind the first violation do not count, though their f is below the limit again
            const float tau = 1.0f / (0.5f * (b.freq[20] + b.freq[21]));
            CHECK(b.freq[seam + 1] <= 1.0f / tau);
            double whole = 0.0, cut = 0.0;
            bank_var_row_host(VarJobSrc(b.jobs.data(), (uint32_t)b.jobs.size(), L), &FVAR, 1, &tau, 1, &whole);
            bank_var_row_host(VarJobSrc(b.jobs.data(), (uint32_t)b.jobs.size(), 21), &FVAR, 1, &tau, 1, &cut);
            CHECK(whole == cut && whole > 0.0);
        }
        // dc_cut at and behind the end, one descriptor of four empty, an odd number of taus
        const std::vector<double> r2 = both(b, {VarDesc{-2, 4, FLT_MAX, L}, AVAR, VarDesc{-2, 4, FLT_MAX, L + 5}, VarDesc{-4, 6, 1.0f, 0}}, {1.0f, 3.0f, 9.0f, 27.0f, 81.0f});
        for (int j = 0; j < 5; ++j)
            CHECK(r2[j] == 0.0 && r2[10 + j] == 0.0 && r2[5 + j] > 0.0 && std::isnan(r2[15 + j]));
    }
    // an empty row
    {
        Bank b;
        make_row(b, 64, {}, {}, {}, 1.5f, 0.25f);
        const std::vector<double> r = both(b, {AVAR, FVAR}, {1.0f, 2.0f, 3.0f});
        for (double x : r)
            CHECK(x == 0.0);
    }
}

template <class T>
static void take(FILE *f, T *dst, size_t count)
{
    if (count && fread(dst, sizeof(T), count, f) != count) {
        printf("FAIL short input\n");
        exit(1);
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        builtin();
        printf("bank_var_check: %ld checks OK\n", checks);
        return 0;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        printf("FAIL cannot open the files\n");
        return 1;
    }
    uint32_t cases = 0;
    take(in, &cases, 1);
    for (uint32_t ci = 0; ci < cases; ++ci) {
        uint32_t head[6];
        take(in, head, 6);
        const uint32_t n = head[0];
        CHECK(head[1] <= 64 && head[2] <= 64 && head[3] >= 1 && head[3] <= VAR_MAX_VARS && head[4] >= 1 && head[4] <= VAR_MAX_TAUS && n >= 2 &&
              n <= (1u << 20));
        float nenbw = 0, power = 0;
        take(in, &nenbw, 1);
        take(in, &power, 1);
        std::vector<uint64_t> count64(head[1]);
        take(in, count64.data(), head[1]);
        std::vector<psdc_break> breaks(head[2]);
        take(in, breaks.data(), head[2]);
        std::vector<float> spectra((size_t)head[1] * (n / 2 + 1));
        take(in, spectra.data(), spectra.size());
        std::vector<VarDesc> vars(head[3]);
        take(in, vars.data(), head[3]);
        std::vector<float> taus(head[4]);
        take(in, taus.data(), head[4]);
        Bank b;
        make_row(b, n, count64, breaks, spectra, nenbw, power);
        const std::vector<double> r = both(b, vars, taus);
        const uint64_t L = b.len;
        fwrite(&L, sizeof L, 1, out);
        if (L) {
            fwrite(b.psd.data(), sizeof(float), L, out);
            fwrite(b.freq.data(), sizeof(float), L, out);
        }
        fwrite(r.data(), sizeof(double), r.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) {
        printf("FAIL cannot write the output\n");
        return 1;
    }
    printf("bank_var_check: %u cases, %ld checks OK\n", cases, checks);
    return 0;
}
