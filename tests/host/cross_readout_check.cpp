// cross_readout_check.cpp -- csrc/cross_readout.h on the CPU: the job table from Break lists, the per-element functions of
// cross_stitch_kernel over every job (tile by tile, as the kernel's grid walks them; the pair form with its six outputs and the
// matrix form with m * m rows), the band sums as cross_band_kernel orders them, and the argument rules that need no object.
// Stand-alone (no library, no device):
//
//   cross_readout_check            built-in cases; asserts that the jobs write every element of a row exactly once and nothing else
//   cross_readout_check IN OUT     cases from IN (written by tests/test_cross_readout_host.py, which gets the Breaks from the
//                                  library's host-only stitch), rows, frequencies, coherence, H1 and band sums to OUT
//
// IN:  u32 cases; a case: u32 n, stages, breaks, bands, rows; f32 nenbw, power; u64 count64[stages]; psdc_break[breaks];
//      f64 acc[stages][rows][n/2 + 1]; f32 bands[bands][2]
// OUT: a case: u64 L; f32 row[rows][L]; f32 freq[L]; and for rows == 4 (a pair: xx, yy, re, im) f64 coherence[L];
//      f64 transfer[L][2]; f64 band[bands][4]
#include "../../include/psdcascade.h"
#include "cross_readout.h"

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

struct Case {
    uint32_t n = 0, rows = 4;
    float nenbw = 0, power = 0;
    std::vector<uint64_t> count64;
    std::vector<psdc_break> breaks;
    std::vector<double> acc; // [stages][rows][n/2 + 1]
    BankBands bands{};
};

struct Result {
    size_t len = 0;
    std::vector<float> rows, freq; // [rows][len], [len]
    std::vector<double> coherence, transfer;
    double band[XREAD_PAIR_ROWS][BANK_MAX_BANDS];
};

// PsdStage::gain in f32, as the library's stage_gain forms it
static float gain(uint32_t n, uint64_t count, float nenbw, float power) { return (float)((uint64_t)(n / 2u) * count) * nenbw * power; }

static const float F_MARK = -77.0f;
static const double D_MARK = -99.0;

// a buffer of `units` rows of `stride` elements with a few behind the last one, all marked
template <class T>
static std::vector<T> marked(size_t units, size_t stride, T mark)
{
    return std::vector<T>(units * stride + 9, mark);
}

// every element of [unit * stride, unit * stride + len) * width is written, nothing else is
template <class T>
static void check_written(const std::vector<T> &v, size_t unit, size_t stride, size_t len, size_t width, T mark)
{
    for (size_t e = 0; e < v.size(); ++e) {
        const bool inside = e >= unit * stride * width && e < (unit * stride + len) * width;
        CHECK(inside == (memcmp(&v[e], &mark, sizeof(T)) != 0));
    }
}

static Result run(const Case &c, uint32_t unit, size_t stride, size_t units)
{
    const uint32_t bins = c.n / 2 + 1;
    // every stage's accumulator in memory of its own, so that the sanitizer sees a read past it
    std::vector<std::vector<double>> acc(c.count64.size());
    for (size_t s = 0; s < acc.size(); ++s)
        acc[s].assign(c.acc.begin() + s * c.rows * bins, c.acc.begin() + (s + 1) * c.rows * bins);
    std::vector<CrossReadJob> jobs;
    const BankRow u = cross_row_jobs(
        c.breaks.data(), c.breaks.size(), unit, c.rows, bins, jobs, [&](uint32_t s) { return (const double *)acc[s].data(); },
        [&](uint32_t s) { return gain(c.n, c.count64[s], c.nenbw, c.power); });
    CHECK(u.job0 == 0 && u.njobs == jobs.size());
    uint32_t max_bins = 0;
    for (const CrossReadJob &j : jobs)
        max_bins = j.bins_end - j.bins_start > max_bins ? j.bins_end - j.bins_start : max_bins;
    const uint32_t tiles = (max_bins + XREAD_THREADS - 1) / XREAD_THREADS;
    std::vector<int> hits(units * stride, 0);
    Result out;
    out.len = u.len;
    const bool pair = c.rows == XREAD_PAIR_ROWS;
    std::vector<float> sxx = marked(units, stride, F_MARK), syy = sxx, freq = sxx, sxy = marked(units, 2 * stride, F_MARK);
    std::vector<double> coh = marked(units, stride, D_MARK), tr = marked(units, 2 * stride, D_MARK);
    std::vector<float> rows = marked(units * c.rows, stride, F_MARK), rfreq = sxx;
    const CrossPairOut po{sxx.data(), syy.data(), sxy.data(), freq.data(), coh.data(), tr.data(), stride};
    // the stitch kernel's grid: tiles x jobs workgroups of XREAD_THREADS threads
    for (uint32_t block = 0; block < tiles * jobs.size(); ++block)
        for (uint32_t t = 0; t < XREAD_THREADS; ++t) {
            const CrossReadJob &j = jobs[block / tiles];
            const uint32_t i = (block % tiles) * XREAD_THREADS + t;
            if (i >= j.bins_end - j.bins_start)
                continue;
            const size_t o = (size_t)j.row * stride + j.start + i;
            CHECK(o < hits.size());
            ++hits[o];
            if (pair)
                cross_pair_element(j, i, po);
            cross_rows_element(j, i, rows.data(), rfreq.data(), stride);
        }
    for (size_t o = 0; o < hits.size(); ++o) // the unit's elements once each, nothing else
        CHECK(hits[o] == (o >= (size_t)unit * stride && o < (size_t)unit * stride + u.len ? 1 : 0));
    check_written(rfreq, unit, stride, u.len, 1, F_MARK);
    for (uint32_t r = 0; r < c.rows; ++r) {
        const float *p = rows.data() + ((size_t)unit * c.rows + r) * stride;
        out.rows.insert(out.rows.end(), p, p + u.len);
    }
    for (size_t e = 0; e < rows.size(); ++e) { // (the marks: no stitched value is -77)
        const size_t row = stride ? e / stride : units * c.rows, col = stride ? e % stride : 0;
        CHECK((rows[e] != F_MARK) == (row / c.rows == unit && col < u.len));
    }
    out.freq.assign(rfreq.begin() + (size_t)unit * stride, rfreq.begin() + (size_t)unit * stride + u.len);
    for (uint32_t r = 0; r < XREAD_PAIR_ROWS; ++r)
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
            out.band[r][b] = 0.0;
    if (pair) {
        check_written(sxx, unit, stride, u.len, 1, F_MARK);
        check_written(syy, unit, stride, u.len, 1, F_MARK);
        check_written(sxy, unit, stride, u.len, 2, F_MARK);
        check_written(freq, unit, stride, u.len, 1, F_MARK);
        check_written(coh, unit, stride, u.len, 1, D_MARK);
        check_written(tr, unit, stride, u.len, 2, D_MARK);
        const size_t o = (size_t)unit * stride;
        for (size_t e = 0; e < u.len; ++e) { // the pair form's rows are the matrix form's
            CHECK(memcmp(&sxx[o + e], &out.rows[e], 4) == 0 && memcmp(&syy[o + e], &out.rows[u.len + e], 4) == 0);
            CHECK(memcmp(&sxy[2 * (o + e)], &out.rows[2 * u.len + e], 4) == 0 && memcmp(&sxy[2 * (o + e) + 1], &out.rows[3 * u.len + e], 4) == 0);
            CHECK(memcmp(&freq[o + e], &out.freq[e], 4) == 0);
        }
        out.coherence.assign(coh.begin() + o, coh.begin() + o + u.len);
        out.transfer.assign(tr.begin() + 2 * o, tr.begin() + 2 * (o + u.len));
        // each output alone writes the same bytes
        std::vector<double> coh2 = marked(units, stride, D_MARK);
        const CrossPairOut only{nullptr, nullptr, nullptr, nullptr, coh2.data(), nullptr, stride};
        for (const CrossReadJob &j : jobs)
            for (uint32_t i = 0; i < j.bins_end - j.bins_start; ++i)
                cross_pair_element(j, i, only);
        CHECK(memcmp(coh2.data(), coh.data(), sizeof(double) * coh.size()) == 0);
        cross_band_pair_host(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, out.band);
    }
    return out;
}

static Case builtin_case(uint32_t rows)
{
    // three stages of n = 64 as the stitch lays them out with the default options: bins [0, 25) of the deepest, then [4, 25), then
    // [4, 33) of stage 0
    Case c;
    c.n = 64;
    c.rows = rows;
    c.nenbw = 1.5f;
    c.power = 0.25f;
    c.count64 = {100, 12, 1};
    const uint64_t lo[3] = {0, 4, 4}, hi[3] = {25, 25, 33};
    uint64_t start = 0;
    for (int i = 0; i < 3; ++i) {
        psdc_break b{};
        b.start = start;
        b.include = 1;
        b.bins_start = lo[i];
        b.bins_end = hi[i];
        b.fft_size = 64;
        b.decimation = 1ull << (3 * (2 - i));
        c.breaks.push_back(b);
        start += hi[i] - lo[i];
    }
    c.acc.resize((size_t)3 * rows * 33);
    for (size_t k = 0; k < c.acc.size(); ++k)
        c.acc[k] = 1.0 + (double)(k % 7) + 1e-9 * (double)k;
    c.bands.n = 2;
    c.bands.lo[0] = 0.0f;
    c.bands.hi[0] = 1.0f;
    c.bands.lo[1] = 0.3f;
    c.bands.hi[1] = 0.2999f; // (holds nothing)
    return c;
}

static void builtin()
{
    Case c = builtin_case(4);
    const size_t len = 25 + 21 + 29;
    // y = 2 x in every bin: coherence 1, H1 = 2 + 0i; then the zero paths
    const size_t bins = 33;
    for (size_t s = 0; s < 3; ++s)
        for (size_t k = 0; k < bins; ++k) {
            double *a = &c.acc[s * 4 * bins];
            a[bins + k] = 4.0 * a[k];
            a[2 * bins + k] = 2.0 * a[k];
            a[3 * bins + k] = 0.0;
        }
    c.acc[(2 * 4 + 0) * bins + 3] = 0.0; // xx of the deepest stage's bin 3: element 3
    c.acc[(2 * 4 + 1) * bins + 5] = 0.0; // yy of its bin 5: element 5
    const Result r = run(c, 1, len + 5, 3);
    CHECK(r.len == len && r.freq[0] == 0.0f && r.freq[len - 1] == 0.5f);
    for (size_t e = 0; e < len; ++e) {
        if (e == 3) {
            CHECK(std::isnan(r.coherence[e]) && std::isnan(r.transfer[2 * e]) && std::isnan(r.transfer[2 * e + 1]));
        } else if (e == 5) {
            CHECK(std::isnan(r.coherence[e]) && r.transfer[2 * e] == 2.0 && r.transfer[2 * e + 1] == 0.0);
        } else {
            CHECK(r.coherence[e] == 1.0 && r.transfer[2 * e] == 2.0 && r.transfer[2 * e + 1] == 0.0);
        }
    }
    for (uint32_t row = 0; row < 4; ++row) { // the trapezoids of each row in sequence
        double whole = 0.0, p1 = 0.0, f1 = 0.0;
        for (size_t k = 0; k < len; ++k) {
            whole += 0.5 * ((double)r.rows[row * len + k] + p1) * ((double)r.freq[k] - f1);
            p1 = r.rows[row * len + k];
            f1 = r.freq[k];
        }
        CHECK(r.band[row][1] == 0.0);
        CHECK(std::fabs(r.band[row][0] - whole) <= 1e-12 * std::fabs(whole));
        CHECK(row == 3 ? r.band[row][0] == 0.0 : r.band[row][0] > 0.0);
    }
    // an excluded middle stage leaves two jobs; no stage at all leaves an empty unit
    c.breaks[1].include = 0;
    c.breaks[2].start = c.breaks[1].start;
    CHECK(run(c, 0, 64, 1).len == 25 + 29);
    c.breaks.clear();
    const Result r3 = run(c, 0, 4, 2);
    CHECK(r3.len == 0 && r3.band[0][0] == 0.0);
    for (uint32_t m = 2; m <= 4; ++m) { // the matrix form: m * m rows
        const Case g = builtin_case(m * m);
        const Result rg = run(g, 2, len, 3);
        CHECK(rg.len == len && rg.rows.size() == (size_t)m * m * len);
        CHECK(rg.rows[0] == (float)g.acc[(size_t)2 * m * m * 33] * (1.0f / (gain(64, 1, 1.5f, 0.25f) * 64.0f)));
    }
    // the argument rules that need no object
    size_t lens[1];
    BankBands bb{};
    const float two[4] = {0.0f, 0.1f, 0.2f, 0.3f}, nan[2] = {NAN, 0.2f}, rev[2] = {0.2f, 0.1f}, many[18] = {};
    double sums[8];
    auto is = [](const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; };
    CHECK(is(cross_read_layout_refusal(lens, nullptr, nullptr), nullptr) && is(cross_read_layout_refusal(lens, lens, lens), nullptr));
    CHECK(is(cross_read_layout_refusal(nullptr, lens, lens), "null lens"));
    CHECK(is(cross_read_layout_refusal(lens, nullptr, lens), "breaks without n_breaks"));
    CHECK(is(cross_read_band_refusal(two, 2, sums, false, &bb), nullptr) && bb.n == 2 && bb.lo[1] == 0.2f && bb.hi[1] == 0.3f);
    CHECK(is(cross_read_band_refusal(nullptr, 0, nullptr, true, &bb), nullptr) && bb.n == 0);
    CHECK(is(cross_read_band_refusal(many, 9, sums, true, &bb), "more than 8 bands"));
    CHECK(is(cross_read_band_refusal(nullptr, 2, sums, true, &bb), "n_bands without a band list"));
    CHECK(is(cross_read_band_refusal(nan, 1, sums, true, &bb), "a band with NaN or lo > hi"));
    CHECK(is(cross_read_band_refusal(rev, 1, sums, true, &bb), "a band with NaN or lo > hi"));
    CHECK(is(cross_read_band_refusal(two, 2, nullptr, true, &bb), "bands without a band output"));
    CHECK(is(cross_read_band_refusal(nullptr, 0, sums, true, &bb), "a band output without bands"));
    CHECK(is(cross_read_band_refusal(nullptr, 0, nullptr, false, &bb), "no output"));
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
        printf("cross_readout_check: %ld checks OK\n", checks);
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
        uint32_t head[5];
        take(in, head, 5);
        Case c;
        c.n = head[0];
        c.rows = head[4];
        CHECK(head[1] <= 64 && head[2] <= 64 && head[3] <= BANK_MAX_BANDS && c.n >= 2 && c.n <= (1u << 20) && c.rows >= 1 && c.rows <= XREAD_MAX_ROWS);
        take(in, &c.nenbw, 1);
        take(in, &c.power, 1);
        c.count64.resize(head[1]);
        take(in, c.count64.data(), head[1]);
        c.breaks.resize(head[2]);
        take(in, c.breaks.data(), head[2]);
        c.acc.resize((size_t)head[1] * c.rows * (c.n / 2 + 1));
        take(in, c.acc.data(), c.acc.size());
        float bands[2 * BANK_MAX_BANDS];
        take(in, bands, 2 * head[3]);
        c.bands.n = head[3];
        for (uint32_t b = 0; b < head[3]; ++b) {
            c.bands.lo[b] = bands[2 * b];
            c.bands.hi[b] = bands[2 * b + 1];
        }
        size_t len = 0;
        for (const psdc_break &b : c.breaks)
            if (b.include)
                len += b.bins_end - b.bins_start;
        const Result r = run(c, ci % 3, len + ci % 5, 3);
        CHECK(r.len == len);
        const uint64_t L = len;
        fwrite(&L, sizeof L, 1, out);
        if (len) {
            fwrite(r.rows.data(), sizeof(float), r.rows.size(), out);
            fwrite(r.freq.data(), sizeof(float), len, out);
        }
        if (c.rows == XREAD_PAIR_ROWS) {
            if (len) {
                fwrite(r.coherence.data(), sizeof(double), len, out);
                fwrite(r.transfer.data(), sizeof(double), 2 * len, out);
            }
            for (uint32_t b = 0; b < head[3]; ++b)
                for (uint32_t row = 0; row < XREAD_PAIR_ROWS; ++row)
                    fwrite(&r.band[row][b], sizeof(double), 1, out);
        }
    }
    fclose(in);
    if (fclose(out) != 0) {
        printf("FAIL cannot write the output\n");
        return 1;
    }
    printf("cross_readout_check: %u cases, %ld checks OK\n", cases, checks);
    return 0;
}
