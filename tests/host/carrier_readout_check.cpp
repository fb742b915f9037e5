// carrier_readout_check.cpp -- csrc/carrier_readout.h on the CPU: the job and unit tables from Break lists, the per-element
// function of carrier_stitch_kernel<MODE> over every job (tile by tile, as the kernel's grid walks them, with the record blocks
// behind the tiles), the band sums as carrier_band_kernel<R> orders them, and the argument rules that need no object.
// Stand-alone (no library, no device):
//
//   carrier_readout_check            built-in cases; asserts that the jobs write every element of a row exactly once and nothing else
//   carrier_readout_check IN OUT     cases from IN (written by tests/test_carrier_readout_host.py and tests/test_gpu_carrier_readout.py,
//                                    which get the Breaks from the library), every output to OUT
//
// IN:  u32 cases; a case: u32 n, stages, breaks, bands, mode (0 sides, 1 SK, 2 AM/PM), given, count0; f32 nenbw, power;
//      f64 carrier re, im (read when given != 0); u64 count64[stages]; psdc_break[breaks]; f64 acc[stages][rows][n/2 + 1]
//      (rows = 2 for sides, else 4); f32 bands[bands][2]
// OUT: a case: u64 L; f32 upper[L], lower[L], freq[L]; SK: f64 sk_upper[L], sk_lower[L]; AM/PM: f64 s_am[L], s_pm[L],
//      s_ampm[L][2], carrier[4]; sides: f64 band[bands][2]; AM/PM: f64 band[bands][4]
#include "../../include/psdcascade.h"
#include "carrier_readout.h"

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
    uint32_t n = 0, mode = 0, given = 0, count0 = 0;
    float nenbw = 0, power = 0;
    double are = 0, aim = 0;
    std::vector<uint64_t> count64;
    std::vector<psdc_break> breaks;
    std::vector<double> acc; // [stages][rows][n/2 + 1]
    BankBands bands{};
    uint32_t rows() const { return mode == CREAD_SIDES ? CREAD_SIDE_ROWS : CREAD_ROWS; }
};

struct Result {
    size_t len = 0;
    std::vector<float> upper, lower, freq;
    std::vector<double> a, b, c; // SK: sk_upper, sk_lower; AM/PM: s_am, s_pm, s_ampm
    double carrier[4];
    double band[CREAD_ROWS][BANK_MAX_BANDS];
};

// PsdStage::gain in f32, as the library's stage_gain forms it
static float gain(uint32_t n, uint64_t count, float nenbw, float power) { return (float)((uint64_t)(n / 2u) * count) * nenbw * power; }

static const float F_MARK = -77.0f;
static const double D_MARK = -99.0;

template <class T>
static std::vector<T> marked(size_t units, size_t stride, T mark)
{
    return std::vector<T>(units * stride + 9, mark);
}

// every element of [unit * stride, unit * stride + len) * width is written, nothing else is (no value is a mark)
template <class T>
static void check_written(const std::vector<T> &v, size_t unit, size_t stride, size_t len, size_t width, T mark)
{
    for (size_t e = 0; e < v.size(); ++e) {
        const bool inside = e >= unit * stride * width && e < (unit * stride + len) * width;
        CHECK(inside == (memcmp(&v[e], &mark, sizeof(T)) != 0));
    }
}

struct Buffers {
    std::vector<float> upper, lower, freq;
    std::vector<double> a, b, c, carrier;
    Buffers(size_t units, size_t stride)
        : upper(marked(units, stride, F_MARK)), lower(upper), freq(upper), a(marked(units, stride, D_MARK)), b(a),
          c(marked(units, 2 * stride, D_MARK)), carrier(marked(units, 4, D_MARK))
    {
    }
};

// the kernel's grid on the CPU: the tile blocks of every job, then the record blocks; hits (may be null) counts the bins
template <int MODE>
static void walk(const std::vector<CarrierReadJob> &jobs, const CarrierOut &o, const std::vector<CarrierUnit> &units, size_t stride,
                 std::vector<int> *hits, std::vector<int> *record_hits)
{
    uint32_t max_bins = 0;
    for (const CarrierReadJob &j : jobs)
        max_bins = j.bins_end - j.bins_start > max_bins ? j.bins_end - j.bins_start : max_bins;
    const bool rows = o.any_row() && !jobs.empty() && max_bins;
    const uint32_t tiles = rows ? (max_bins + XREAD_THREADS - 1) / XREAD_THREADS : 0;
    const uint32_t tile_blocks = tiles * (uint32_t)jobs.size();
    const uint32_t n_units = (uint32_t)units.size();
    const uint32_t blocks = tile_blocks + (MODE == CREAD_AMPM && o.carrier ? (n_units + XREAD_THREADS - 1) / XREAD_THREADS : 0);
    for (uint32_t block = 0; block < blocks; ++block)
        for (uint32_t t = 0; t < XREAD_THREADS; ++t) {
            if (block >= tile_blocks) {
                const uint32_t unit = (block - tile_blocks) * XREAD_THREADS + t;
                if (MODE == CREAD_AMPM && unit < n_units) {
                    if (record_hits)
                        ++(*record_hits)[unit];
                    carrier_record(units.data(), unit, o.carrier);
                }
                continue;
            }
            const CarrierReadJob &j = jobs[block / tiles];
            const uint32_t i = (block % tiles) * XREAD_THREADS + t;
            if (i >= j.bins_end - j.bins_start)
                continue;
            if (hits) {
                const size_t e = (size_t)j.row * stride + j.start + i;
                CHECK(e < hits->size());
                ++(*hits)[e];
            }
            carrier_element<MODE>(j, i, o, units.data());
        }
}

static void walk_mode(uint32_t mode, const std::vector<CarrierReadJob> &jobs, const CarrierOut &o, const std::vector<CarrierUnit> &units,
                      size_t stride, std::vector<int> *hits, std::vector<int> *record_hits)
{
    if (mode == CREAD_SIDES)
        walk<CREAD_SIDES>(jobs, o, units, stride, hits, record_hits);
    else if (mode == CREAD_SK)
        walk<CREAD_SK>(jobs, o, units, stride, hits, record_hits);
    else
        walk<CREAD_AMPM>(jobs, o, units, stride, hits, record_hits);
}

static Result run(const Case &c, uint32_t unit, size_t stride, size_t units)
{
    const uint32_t bins = c.n / 2 + 1, rows = c.rows();
    // every stage's accumulator in memory of its own, so that the sanitizer sees a read past it
    std::vector<std::vector<double>> acc(c.count64.size());
    for (size_t s = 0; s < acc.size(); ++s)
        acc[s].assign(c.acc.begin() + s * rows * bins, c.acc.begin() + (s + 1) * rows * bins);
    std::vector<CarrierReadJob> jobs;
    const BankRow u = cross_row_jobs(
        c.breaks.data(), c.breaks.size(), unit, rows, bins, jobs, [&](uint32_t s) { return (const double *)acc[s].data(); },
        [&](uint32_t s) { return gain(c.n, c.count64[s], c.nenbw, c.power); });
    CHECK(u.job0 == 0 && u.njobs == jobs.size());
    for (size_t i = 0, k = 0; i < c.breaks.size(); ++i) // the jobs carry their Break's count
        if (c.breaks[i].include && c.breaks[i].bins_end > c.breaks[i].bins_start)
            CHECK(jobs[k++].count == c.breaks[i].count);
    // the unit table: every unit is this channel (the others select nothing: they have no job), so that a record block of more
    // than one unit is walked
    std::vector<CarrierUnit> cu;
    if (c.mode == CREAD_AMPM) {
        CarrierUnit one{};
        one.n2p = (double)c.n * (double)c.n * (double)c.power;
        one.bins = bins;
        one.src0 = acc.empty() ? nullptr : acc[0].data();
        one.count0 = c.count0;
        if (c.given)
            CHECK(carrier_given(c.are, c.aim, &one) == nullptr);
        cu.assign(units, one);
    }
    Result out;
    out.len = u.len;
    Buffers all(units, stride);
    CarrierOut o{all.upper.data(), all.lower.data(), all.freq.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stride};
    if (c.mode == CREAD_SK) {
        o.sk_upper = all.a.data();
        o.sk_lower = all.b.data();
    } else if (c.mode == CREAD_AMPM) {
        o.s_am = all.a.data();
        o.s_pm = all.b.data();
        o.s_ampm = all.c.data();
        o.carrier = all.carrier.data();
    }
    std::vector<int> hits(units * stride, 0), record_hits(units, 0);
    walk_mode(c.mode, jobs, o, cu, stride, &hits, &record_hits);
    for (size_t e = 0; e < hits.size(); ++e) // the unit's elements once each, nothing else
        CHECK(hits[e] == (e >= (size_t)unit * stride && e < (size_t)unit * stride + u.len ? 1 : 0));
    check_written(all.upper, unit, stride, u.len, 1, F_MARK);
    check_written(all.lower, unit, stride, u.len, 1, F_MARK);
    check_written(all.freq, unit, stride, u.len, 1, F_MARK);
    if (c.mode != CREAD_SIDES) {
        check_written(all.a, unit, stride, u.len, 1, D_MARK);
        check_written(all.b, unit, stride, u.len, 1, D_MARK);
    }
    if (c.mode == CREAD_AMPM) {
        check_written(all.c, unit, stride, u.len, 2, D_MARK);
        for (size_t e = 0; e < all.carrier.size(); ++e) // one write a record, every unit's four values, nothing behind them
            CHECK((e < 4 * units) == (memcmp(&all.carrier[e], &D_MARK, 8) != 0));
        for (size_t i = 0; i < units; ++i)
            CHECK(record_hits[i] == 1);
        memcpy(out.carrier, &all.carrier[4 * unit], sizeof out.carrier);
    }
    // each output alone writes the same bytes and nothing else
    for (int which = 0; which < 7; ++which) {
        Buffers b(units, stride);
        CarrierOut only{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stride};
        const bool sk = c.mode == CREAD_SK, am = c.mode == CREAD_AMPM;
        if (which == 0)
            only.upper = b.upper.data();
        else if (which == 1)
            only.lower = b.lower.data();
        else if (which == 2)
            only.freq = b.freq.data();
        else if (which == 3 && (sk || am))
            (sk ? only.sk_upper : only.s_am) = b.a.data();
        else if (which == 4 && (sk || am))
            (sk ? only.sk_lower : only.s_pm) = b.b.data();
        else if (which == 5 && am)
            only.s_ampm = b.c.data();
        else if (which == 6 && am)
            only.carrier = b.carrier.data();
        else
            continue;
        walk_mode(c.mode, jobs, only, cu, stride, nullptr, nullptr);
        auto same = [](const auto &x, const auto &y, bool asked, auto mark) {
            for (size_t e = 0; e < x.size(); ++e)
                if (asked ? memcmp(&x[e], &y[e], sizeof mark) != 0 : memcmp(&x[e], &mark, sizeof mark) != 0)
                    return false;
            return true;
        };
        CHECK(same(b.upper, all.upper, which == 0, F_MARK) && same(b.lower, all.lower, which == 1, F_MARK) && same(b.freq, all.freq, which == 2, F_MARK));
        CHECK(same(b.a, all.a, which == 3, D_MARK) && same(b.b, all.b, which == 4, D_MARK) && same(b.c, all.c, which == 5, D_MARK));
        CHECK(same(b.carrier, all.carrier, which == 6, D_MARK));
    }
    const size_t o0 = (size_t)unit * stride;
    out.upper.assign(all.upper.begin() + o0, all.upper.begin() + o0 + u.len);
    out.lower.assign(all.lower.begin() + o0, all.lower.begin() + o0 + u.len);
    out.freq.assign(all.freq.begin() + o0, all.freq.begin() + o0 + u.len);
    out.a.assign(all.a.begin() + o0, all.a.begin() + o0 + u.len);
    out.b.assign(all.b.begin() + o0, all.b.begin() + o0 + u.len);
    out.c.assign(all.c.begin() + 2 * o0, all.c.begin() + 2 * (o0 + u.len));
    for (uint32_t r = 0; r < CREAD_ROWS; ++r)
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
            out.band[r][b] = 0.0;
    if (c.mode == CREAD_SIDES)
        carrier_band_sides_host(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, out.band);
    else if (c.mode == CREAD_AMPM)
        carrier_band_ampm_host(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, cu[unit], out.band);
    return out;
}

static Case builtin_case(uint32_t mode)
{
    // three stages of n = 64 as the stitch lays them out with the default options: bins [0, 25) of the deepest, then [4, 25), then
    // [4, 33) of stage 0
    Case c;
    c.n = 64;
    c.mode = mode;
    c.nenbw = 1.5f;
    c.power = 0.25f;
    c.count64 = {100, 12, 1};
    c.count0 = 100;
    const uint64_t lo[3] = {0, 4, 4}, hi[3] = {25, 25, 33};
    uint64_t start = 0;
    for (int i = 0; i < 3; ++i) {
        psdc_break b{};
        b.start = start;
        b.include = 1;
        b.count = (uint32_t)c.count64[2 - i];
        b.bins_start = lo[i];
        b.bins_end = hi[i];
        b.fft_size = 64;
        b.decimation = 1ull << (3 * (2 - i));
        c.breaks.push_back(b);
        start += hi[i] - lo[i];
    }
    c.acc.resize((size_t)3 * c.rows() * 33);
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
    const size_t len = 25 + 21 + 29, bins = 33;
    { // sides: the trapezoids of each row in sequence
        const Case c = builtin_case(CREAD_SIDES);
        const Result r = run(c, 1, len + 5, 3);
        CHECK(r.len == len && r.freq[0] == 0.0f && r.freq[len - 1] == 0.5f);
        CHECK(r.upper[0] == (float)c.acc[(size_t)2 * 2 * bins] * (1.0f / (gain(64, 1, 1.5f, 0.25f) * 64.0f)));
        for (uint32_t row = 0; row < 2; ++row) {
            const std::vector<float> &p = row ? r.lower : r.upper;
            double whole = 0.0, p1 = 0.0, f1 = 0.0;
            for (size_t k = 0; k < len; ++k) {
                whole += 0.5 * ((double)p[k] + p1) * ((double)r.freq[k] - f1);
                p1 = p[k];
                f1 = r.freq[k];
            }
            CHECK(r.band[row][1] == 0.0 && r.band[row][0] > 0.0 && std::fabs(r.band[row][0] - whole) <= 1e-12 * whole);
        }
    }
    { // SK: s2 = 2 s1^2 / M gives (M + 1) / (M - 1); NaN for the stage of one average and where s1 == 0
        Case c = builtin_case(CREAD_SK);
        for (size_t s = 0; s < 3; ++s)
            for (size_t k = 0; k < bins; ++k) {
                double *a = &c.acc[s * 4 * bins];
                const double m = (double)c.count64[s];
                a[2 * bins + k] = 2.0 * a[k] * a[k] / m;
                a[3 * bins + k] = a[bins + k] * a[bins + k] / m;
            }
        c.acc[(1 * 4 + 0) * bins + 7] = 0.0; // S1 upper of the middle stage's bin 7: element 25 + 3
        const Result r = run(c, 2, len, 3);
        for (size_t e = 0; e < len; ++e) {
            const double m = e < 25 ? 1.0 : e < 46 ? 12.0 : 100.0;
            if (m < 2 || e == 28) {
                CHECK(std::isnan(r.a[e]));
            } else {
                CHECK(std::fabs(r.a[e] - (m + 1.0) / (m - 1.0)) <= 1e-12);
            }
            if (m < 2) {
                CHECK(std::isnan(r.b[e]));
            } else {
                CHECK(std::fabs(r.b[e]) <= 1e-12);
            }
        }
    }
    { // AM/PM: comp = u0 (U + L) / 2 is pure AM, comp = -u0 (U + L) / 2 pure PM; the carrier from bin 0 of stage 0
        for (int pm = 0; pm < 2; ++pm) {
            Case c = builtin_case(CREAD_AMPM);
            const double ur = 0.6, ui = 0.8;
            for (size_t s = 0; s < 3; ++s)
                for (size_t k = 0; k < bins; ++k) {
                    double *a = &c.acc[s * 4 * bins];
                    const double mean = 0.5 * (a[k] + a[bins + k]) * (pm ? -1.0 : 1.0);
                    a[2 * bins + k] = mean * ur;
                    a[3 * bins + k] = mean * ui;
                }
            double *a0 = &c.acc[0];
            a0[2 * bins] = 3.0 * ur * 100.0;
            a0[3 * bins] = 3.0 * ui * 100.0;
            a0[0] = a0[bins] = 300.0;
            const Result r = run(c, 0, len + 1, 2);
            CHECK(std::fabs(r.carrier[0] - 300.0 / (100.0 * 64.0 * 64.0 * 0.25)) <= 1e-15 && std::fabs(r.carrier[1] - ur) <= 1e-15);
            CHECK(std::fabs(r.carrier[2] - ui) <= 1e-15 && std::fabs(r.carrier[3] - 1.0) <= 1e-15);
            for (size_t e = 0; e + 29 < len; ++e) { // (the deeper stages: bin 0 of stage 0 is not among them)
                const double on = pm ? r.b[e] : r.a[e], off = pm ? r.a[e] : r.b[e];
                CHECK(on > 0.0 && std::fabs(off) <= 1e-14 * on && std::fabs(r.c[2 * e]) <= 1e-14 * on);
            }
            CHECK(r.band[2 + pm][0] > 0.0 && std::fabs(r.band[3 - pm][0]) <= 1e-12 * r.band[2 + pm][0] && r.band[2][1] == 0.0);
            // a given carrier: the same split from A = 2 (cos, sin) of half u's angle; lock NaN
            c.given = 1;
            const double half = 0.5 * std::atan2(ui, ur);
            c.are = 2.0 * std::cos(half);
            c.aim = 2.0 * std::sin(half);
            const Result g = run(c, 1, len, 2);
            CHECK(g.carrier[0] == c.are * c.are + c.aim * c.aim && std::fabs(g.carrier[1] - ur) <= 1e-15 && std::isnan(g.carrier[3]));
            // no carrier: comp[0] == 0, then no average in stage 0: the record (0, NaN, NaN, NaN), NaN rows, upper / lower as before
            c.given = 0;
            c.acc[2 * bins] = c.acc[3 * bins] = 0.0;
            for (int k = 0; k < 2; ++k) {
                const Result z = run(c, 1, len, 2);
                CHECK(z.carrier[0] == 0.0 && std::isnan(z.carrier[1]) && std::isnan(z.carrier[2]) && std::isnan(z.carrier[3]));
                for (size_t e = 0; e < len; ++e)
                    CHECK(std::isnan(z.a[e]) && std::isnan(z.b[e]) && std::isnan(z.c[2 * e]) && std::isnan(z.c[2 * e + 1]));
                CHECK(std::isnan(z.band[2][0]) && std::isnan(z.band[3][0]) && z.band[2][1] == 0.0 && z.band[0][0] == g.band[0][0]);
                CHECK(memcmp(z.upper.data(), g.upper.data(), 4 * len) == 0 && memcmp(z.lower.data(), g.lower.data(), 4 * len) == 0);
                c.acc[2 * bins] = 1.0;
                c.count0 = 0;
            }
        }
    }
    for (uint32_t mode = 0; mode < 3; ++mode) { // an excluded middle stage leaves two jobs; no stage at all leaves an empty unit
        Case c = builtin_case(mode);
        c.breaks[1].include = 0;
        c.breaks[2].start = c.breaks[1].start;
        CHECK(run(c, 0, 64, 1).len == 25 + 29);
        c.breaks.clear();
        c.count64.clear();
        c.acc.clear();
        c.count0 = 0;
        const Result r3 = run(c, 1, 4, 300); // (300 units: two record blocks)
        CHECK(r3.len == 0 && r3.band[0][0] == 0.0);
        if (mode == CREAD_AMPM)
            CHECK(r3.carrier[0] == 0.0 && std::isnan(r3.carrier[1]));
    }
    // the argument rules that need no object
    size_t lens[1];
    BankBands bb{};
    CarrierUnit u{};
    const float two[4] = {0.0f, 0.1f, 0.2f, 0.3f}, nan[2] = {NAN, 0.2f}, rev[2] = {0.2f, 0.1f}, many[18] = {};
    double sums[8];
    auto is = [](const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; };
    CHECK(is(cross_read_layout_refusal(lens, nullptr, nullptr), nullptr));
    CHECK(is(cross_read_layout_refusal(nullptr, lens, lens), "null lens"));
    CHECK(is(cross_read_layout_refusal(lens, nullptr, lens), "breaks without n_breaks"));
    CHECK(is(cross_read_band_refusal(two, 2, sums, false, &bb), nullptr) && bb.n == 2);
    CHECK(is(cross_read_band_refusal(many, 9, sums, true, &bb), "more than 8 bands"));
    CHECK(is(cross_read_band_refusal(nan, 1, sums, true, &bb), "a band with NaN or lo > hi"));
    CHECK(is(cross_read_band_refusal(rev, 1, sums, true, &bb), "a band with NaN or lo > hi"));
    CHECK(is(cross_read_band_refusal(two, 2, nullptr, true, &bb), "bands without a band output"));
    CHECK(is(cross_read_band_refusal(nullptr, 0, sums, true, &bb), "a band output without bands"));
    CHECK(is(cross_read_band_refusal(nullptr, 0, nullptr, false, &bb), "no output"));
    const char *bad = "a given carrier amplitude must be finite and not 0";
    CHECK(is(carrier_given(0.0, 0.0, &u), bad) && is(carrier_given(NAN, 1.0, &u), bad) && is(carrier_given(1.0, INFINITY, &u), bad));
    CHECK(is(carrier_given(1e200, 1e200, &u), bad) && u.given == 0);
    CHECK(is(carrier_given(0.0, 2.0, &u), nullptr) && u.given == 1 && u.P == 4.0 && u.ur == -1.0 && u.ui == 0.0);
}

template <class T>
static void take(FILE *f, T *dst, size_t count)
{
    if (count && fread(dst, sizeof(T), count, f) != count) {
        printf("FAIL short input\n");
        exit(1);
    }
}

template <class T>
static void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty())
        fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        builtin();
        printf("carrier_readout_check: %ld checks OK\n", checks);
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
        uint32_t head[7];
        take(in, head, 7);
        Case c;
        c.n = head[0];
        c.mode = head[4];
        c.given = head[5];
        c.count0 = head[6];
        CHECK(head[1] <= 64 && head[2] <= 64 && head[3] <= BANK_MAX_BANDS && c.n >= 2 && c.n <= (1u << 20) && c.mode <= 2);
        take(in, &c.nenbw, 1);
        take(in, &c.power, 1);
        take(in, &c.are, 1);
        take(in, &c.aim, 1);
        c.count64.resize(head[1]);
        take(in, c.count64.data(), head[1]);
        c.breaks.resize(head[2]);
        take(in, c.breaks.data(), head[2]);
        c.acc.resize((size_t)head[1] * c.rows() * (c.n / 2 + 1));
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
        put(out, r.upper);
        put(out, r.lower);
        put(out, r.freq);
        if (c.mode != CREAD_SIDES) {
            put(out, r.a);
            put(out, r.b);
        }
        if (c.mode == CREAD_AMPM) {
            put(out, r.c);
            fwrite(r.carrier, sizeof(double), 4, out);
        }
        const uint32_t band_rows = c.mode == CREAD_SIDES ? CREAD_SIDE_ROWS : c.mode == CREAD_AMPM ? CREAD_ROWS : 0;
        for (uint32_t b = 0; b < head[3]; ++b)
            for (uint32_t row = 0; row < band_rows; ++row)
                fwrite(&r.band[row][b], sizeof(double), 1, out);
    }
    fclose(in);
    if (fclose(out) != 0) {
        printf("FAIL cannot write the output\n");
        return 1;
    }
    printf("carrier_readout_check: %u cases, %ld checks OK\n", cases, checks);
    return 0;
}
