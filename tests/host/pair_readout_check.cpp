// pair_readout_check.cpp -- csrc/pair_readout.h on the CPU: the job and unit tables from Break lists, the per-element functions of
// pair_stitch_kernel<MODE> over every job (tile by tile, as the kernel's grid walks them, with the record blocks behind the
// tiles), the band sums as pair_band_kernel orders them, and the argument rules that need no object.
// Stand-alone (no library, no device):
//
//   pair_readout_check            built-in cases; asserts that the jobs write every element of a row exactly once and nothing else
//   pair_readout_check IN OUT     cases from IN (written by tests/test_pair_readout_host.py), every output to OUT
//
// IN:  u32 cases; a case: u32 n, stages, breaks, bands, mode (0 CSD, 1 AM/PM), rows (8 or 12), given, count0; f32 nenbw, power;
//      f64 given[5] = p_ab, re w, im w, re q, im q (used when given != 0); u64 count64[stages]; psdc_break[breaks];
//      f64 acc[stages][rows][n/2 + 1]; f32 bands[bands][2]
// OUT: a case: u64 L; CSD: f32 saa_up[L], saa_lo[L], sbb_up[L], sbb_lo[L], sab_up[L][2], sab_lo[L][2], freq[L]; f64 coh_up[L],
//      coh_lo[L], h1_up[L][2], h1_lo[L][2]; AM/PM: f32 freq[L]; f64 cab, cba, s_am, s_pm, s_am_pm, s_pm_am [L][2] each, carrier[7];
//      both: f64 band[bands][8]
#include "../../include/psdcascade.h"
#include "pair_readout.h"

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
    uint32_t n = 0, mode = 0, rows = 8, given = 0, count0 = 0;
    float nenbw = 0, power = 0;
    double car[5] = {};
    std::vector<uint64_t> count64;
    std::vector<psdc_break> breaks;
    std::vector<double> acc; // [stages][rows][n/2 + 1]
    BankBands bands{};
};

// the outputs of one unit, in the order of PairCsdOut (f[0 ... 6], d[0 ... 3]) or PairAmPmOut (f[0], d[0 ... 5])
struct Result {
    size_t len = 0;
    std::vector<float> f[7];
    std::vector<double> d[6];
    double carrier[PREAD_RECORD];
    double band[PREAD_BAND_ROWS][BANK_MAX_BANDS];
};

// PsdStage::gain in f32, as the library's stage_gain forms it
static float gain(uint32_t n, uint64_t count, float nenbw, float power) { return (float)((uint64_t)(n / 2u) * count) * nenbw * power; }

static const float F_MARK = -77.0f;
static const double D_MARK = -99.0;
static const size_t F_WIDTH[7] = {1, 1, 1, 1, 2, 2, 1}; // CSD: values an element of each f32 output
static const size_t D_WIDTH[4] = {1, 1, 2, 2};          // CSD: ... and of each f64 output (AM/PM: all 2)

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

template <class T>
static bool same(const std::vector<T> &x, const std::vector<T> &y, bool asked, T mark)
{
    for (size_t e = 0; e < x.size(); ++e)
        if (asked ? memcmp(&x[e], &y[e], sizeof mark) != 0 : memcmp(&x[e], &mark, sizeof mark) != 0)
            return false;
    return true;
}

struct Buffers {
    std::vector<float> f[7];
    std::vector<double> d[6], carrier;
    Buffers(size_t units, size_t stride, bool ampm)
    {
        for (int i = 0; i < 7; ++i)
            f[i] = marked(units, stride * F_WIDTH[i], F_MARK);
        for (int i = 0; i < 6; ++i)
            d[i] = marked(units, stride * (ampm ? 2 : D_WIDTH[i % 4]), D_MARK);
        carrier = marked(units, PREAD_RECORD, D_MARK);
    }
    // which: a bit an output (CSD: bits 0 ... 10; AM/PM: bit 0 freq, 1 ... 6 the f64 rows, 7 the carrier)
    PairCsdOut csd(unsigned which, size_t stride)
    {
        auto fp = [&](int i) { return which >> i & 1 ? f[i].data() : nullptr; };
        auto dp = [&](int i) { return which >> (7 + i) & 1 ? d[i].data() : nullptr; };
        return {fp(0), fp(1), fp(2), fp(3), fp(4), fp(5), fp(6), dp(0), dp(1), dp(2), dp(3), stride};
    }
    PairAmPmOut ampm(unsigned which, size_t stride)
    {
        auto dp = [&](int i) { return which >> (1 + i) & 1 ? d[i].data() : nullptr; };
        return {which & 1 ? f[0].data() : nullptr, dp(0), dp(1), dp(2), dp(3), dp(4), dp(5), which >> 7 & 1 ? carrier.data() : nullptr, stride};
    }
};

// the kernel's grid on the CPU: the tile blocks of every job, then the record blocks; hits (may be null) counts the bins
static void walk(uint32_t mode, const std::vector<CarrierReadJob> &jobs, const PairCsdOut &oc, const PairAmPmOut &oa,
                 const std::vector<PairUnit> &units, size_t stride, std::vector<int> *hits, std::vector<int> *record_hits)
{
    uint32_t max_bins = 0;
    for (const CarrierReadJob &j : jobs)
        max_bins = j.bins_end - j.bins_start > max_bins ? j.bins_end - j.bins_start : max_bins;
    const bool ampm = mode == PREAD_AMPM;
    const bool rows = (ampm ? oa.any_row() : oc.any_row()) && !jobs.empty() && max_bins;
    const uint32_t tiles = rows ? (max_bins + XREAD_THREADS - 1) / XREAD_THREADS : 0;
    const uint32_t tile_blocks = tiles * (uint32_t)jobs.size();
    const uint32_t n_units = (uint32_t)units.size();
    const uint32_t blocks = tile_blocks + (ampm && oa.carrier ? (n_units + XREAD_THREADS - 1) / XREAD_THREADS : 0);
    for (uint32_t block = 0; block < blocks; ++block)
        for (uint32_t t = 0; t < XREAD_THREADS; ++t) {
            if (block >= tile_blocks) {
                const uint32_t unit = (block - tile_blocks) * XREAD_THREADS + t;
                if (ampm && unit < n_units) {
                    if (record_hits)
                        ++(*record_hits)[unit];
                    pair_record(units.data(), unit, oa.carrier);
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
            if (ampm)
                pair_ampm_element(j, i, oa, units.data());
            else
                pair_csd_element(j, i, oc);
        }
}

static Result run(const Case &c, uint32_t unit, size_t stride, size_t units)
{
    const uint32_t bins = c.n / 2 + 1, rows = c.rows;
    const bool ampm = c.mode == PREAD_AMPM;
    CHECK(!ampm || rows == PREAD_ROWS);
    // every stage's accumulator in memory of its own, so that the sanitizer sees a read past it (an 8-row stage has no row 8)
    std::vector<std::vector<double>> acc(c.count64.size());
    for (size_t s = 0; s < acc.size(); ++s)
        acc[s].assign(c.acc.begin() + s * rows * bins, c.acc.begin() + (s + 1) * rows * bins);
    std::vector<CarrierReadJob> jobs;
    const BankRow u = cross_row_jobs(
        c.breaks.data(), c.breaks.size(), unit, rows, bins, jobs, [&](uint32_t s) { return (const double *)acc[s].data(); },
        [&](uint32_t s) { return gain(c.n, c.count64[s], c.nenbw, c.power); });
    CHECK(u.job0 == 0 && u.njobs == jobs.size());
    // the unit table: every unit is this pair (the others select nothing: they have no job), so that a record block of more than
    // one unit is walked
    std::vector<PairUnit> pu;
    if (ampm) {
        PairUnit one{};
        one.n2p = (double)c.n * (double)c.n * (double)c.power;
        one.bins = bins;
        one.src0 = acc.empty() ? nullptr : acc[0].data();
        one.count0 = c.count0;
        if (c.given)
            CHECK(pair_given(c.car, &one) == nullptr);
        pu.assign(units, one);
    }
    Result out;
    out.len = u.len;
    Buffers all(units, stride, ampm);
    const unsigned every = ampm ? 0xFFu : 0x7FFu;
    std::vector<int> hits(units * stride, 0), record_hits(units, 0);
    walk(c.mode, jobs, all.csd(every, stride), all.ampm(every, stride), pu, stride, &hits, &record_hits);
    for (size_t e = 0; e < hits.size(); ++e) // the unit's elements once each, nothing else: every job covers its row exactly once
        CHECK(hits[e] == (e >= (size_t)unit * stride && e < (size_t)unit * stride + u.len ? 1 : 0));
    const int nf = ampm ? 1 : 7, nd = ampm ? 6 : 4;
    for (int i = 0; i < 7; ++i)
        check_written(all.f[i], unit, stride, i < nf ? u.len : 0, ampm ? 1 : F_WIDTH[i], F_MARK);
    for (int i = 0; i < 6; ++i)
        check_written(all.d[i], unit, stride, i < nd ? u.len : 0, ampm ? 2 : D_WIDTH[i % 4], D_MARK);
    if (ampm) {
        for (size_t e = 0; e < all.carrier.size(); ++e) // one write a record, every unit's seven values, nothing behind them
            CHECK((e < PREAD_RECORD * units) == (memcmp(&all.carrier[e], &D_MARK, 8) != 0));
        for (size_t i = 0; i < units; ++i)
            CHECK(record_hits[i] == 1);
        memcpy(out.carrier, &all.carrier[PREAD_RECORD * unit], sizeof out.carrier);
    }
    // each output alone writes the same bytes and nothing else (the rows a thread loads depend on what is asked)
    for (int which = 0; which < (ampm ? 8 : 11); ++which) {
        Buffers b(units, stride, ampm);
        walk(c.mode, jobs, b.csd(1u << which, stride), b.ampm(1u << which, stride), pu, stride, nullptr, nullptr);
        for (int i = 0; i < 7; ++i)
            CHECK(same(b.f[i], all.f[i], ampm ? which == 0 && i == 0 : which == i, F_MARK));
        for (int i = 0; i < 6; ++i)
            CHECK(same(b.d[i], all.d[i], ampm ? which == 1 + i : which == 7 + i, D_MARK));
        CHECK(same(b.carrier, all.carrier, ampm && which == 7, D_MARK));
    }
    if (ampm) { // cab and cba without a split output take the short path: the same bytes
        Buffers b(units, stride, true);
        walk(c.mode, jobs, b.csd(0, stride), b.ampm(0x6u, stride), pu, stride, nullptr, nullptr);
        CHECK(same(b.d[0], all.d[0], true, D_MARK) && same(b.d[1], all.d[1], true, D_MARK) && same(b.d[2], all.d[2], false, D_MARK));
    }
    const size_t o0 = (size_t)unit * stride;
    for (int i = 0; i < nf; ++i) {
        const size_t w = ampm ? 1 : F_WIDTH[i];
        out.f[i].assign(all.f[i].begin() + w * o0, all.f[i].begin() + w * (o0 + u.len));
    }
    for (int i = 0; i < nd; ++i) {
        const size_t w = ampm ? 2 : D_WIDTH[i];
        out.d[i].assign(all.d[i].begin() + w * o0, all.d[i].begin() + w * (o0 + u.len));
    }
    for (uint32_t r = 0; r < PREAD_BAND_ROWS; ++r)
        for (uint32_t b = 0; b < BANK_MAX_BANDS; ++b)
            out.band[r][b] = 0.0;
    if (ampm)
        pair_band_ampm_host(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, pu[unit], out.band);
    else
        pair_band_csd_host(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, out.band);
    // two workgroups of four rows each give the sums of one workgroup of eight: a row's sum does not depend on the others
    for (uint32_t half = 0; half < 2; ++half) {
        double part[4][BANK_MAX_BANDS];
        if (ampm)
            bank_band_rows_host<4>(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, PairAmPmVal{pair_split_of(pu[unit]), 4 * half}, part);
        else
            bank_band_rows_host<4>(jobs.data(), (uint32_t)jobs.size(), u.len, c.bands, PairCsdVal{4 * half}, part);
        for (uint32_t r = 0; r < 4; ++r)
            CHECK(memcmp(part[r], out.band[4 * half + r], sizeof part[r]) == 0);
    }
    return out;
}

static Case builtin_case(uint32_t mode, uint32_t rows)
{
    // three stages of n = 64 as the stitch lays them out with the default options: bins [0, 25) of the deepest, then [4, 25), then
    // [4, 33) of stage 0
    Case c;
    c.n = 64;
    c.mode = mode;
    c.rows = rows;
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
    const size_t len = 25 + 21 + 29, bins = 33;
    for (uint32_t rows = 8; rows <= 12; rows += 4) { // CSD on both row counts: values, coherence, H1, the trapezoids in sequence
        Case c = builtin_case(PREAD_CSD, rows);
        c.acc[(1 * rows + 0) * bins + 7] = 0.0; // S_aa upper of the middle stage's bin 7: element 25 + 3
        c.acc[(1 * rows + 3) * bins + 9] = 0.0; // S_bb lower of its bin 9: element 25 + 5
        const Result r = run(c, 1, len + 5, 3);
        CHECK(r.len == len && r.f[6][0] == 0.0f && r.f[6][len - 1] == 0.5f);
        CHECK(r.f[0][0] == (float)c.acc[(size_t)2 * rows * bins] * (1.0f / (gain(64, 1, 1.5f, 0.25f) * 64.0f)));
        for (size_t e = 0; e < len; ++e) {
            const size_t s = e < 25 ? 2 : e < 46 ? 1 : 0, k = e < 25 ? e : e < 46 ? e - 25 + 4 : e - 46 + 4;
            const double *a = &c.acc[s * rows * bins];
            auto at = [&](uint32_t row) { return a[row * bins + k]; };
            if (e == 28) {
                CHECK(std::isnan(r.d[0][e]) && std::isnan(r.d[2][2 * e]) && std::isnan(r.d[2][2 * e + 1]) && !std::isnan(r.d[1][e]));
            } else {
                CHECK(r.d[0][e] == (at(4) * at(4) + at(6) * at(6)) / (at(0) * at(2)));
                CHECK(r.d[2][2 * e] == at(4) / at(0) && r.d[2][2 * e + 1] == at(6) / at(0));
            }
            if (e == 30) {
                CHECK(std::isnan(r.d[1][e]) && !std::isnan(r.d[3][2 * e]));
            } else {
                CHECK(r.d[1][e] == (at(5) * at(5) + at(7) * at(7)) / (at(1) * at(3)));
            }
            CHECK(r.d[3][2 * e] == at(5) / at(1) && r.d[3][2 * e + 1] == at(7) / at(1));
        }
        const float *row8[8] = {r.f[0].data(), r.f[1].data(), r.f[2].data(), r.f[3].data(), nullptr, nullptr, nullptr, nullptr};
        for (uint32_t row = 0; row < 8; ++row) {
            double whole = 0.0, p1 = 0.0, f1 = 0.0;
            for (size_t k = 0; k < len; ++k) {
                // (rows 4 ... 7: re up, re lo, im up, im lo from the interleaved sab rows)
                const double p = row < 4 ? row8[row][k] : r.f[4 + (row & 1)][2 * k + (row >= 6)];
                whole += 0.5 * (p + p1) * ((double)r.f[6][k] - f1);
                p1 = p;
                f1 = r.f[6][k];
            }
            CHECK(r.band[row][1] == 0.0 && r.band[row][0] > 0.0 && std::fabs(r.band[row][0] - whole) <= 1e-12 * whole);
        }
    }
    { // AM/PM: shared pure AM, then shared pure PM, with carriers of phases alpha (a) and beta (b): w = e^{i (beta - alpha)},
      // q = e^{i (alpha + beta)}.  Common modulation m of strength S: U = L* = S w, cab = cba* ... all four rows S-scaled phasors
        for (int pm = 0; pm < 2; ++pm) {
            Case c = builtin_case(PREAD_AMPM, 12);
            const double wr = 0.6, wi = 0.8, qr = -0.28, qi = 0.96;
            for (size_t s = 0; s < 3; ++s)
                for (size_t k = 0; k < bins; ++k) {
                    double *a = &c.acc[s * 12 * bins];
                    const double S = a[k], sg = pm ? -1.0 : 1.0;
                    // T1 = U conj(w) = S, T4 = conj(L) w = S, T2 = conj(cab) q = sg S, T3 = cba conj(q) = sg S
                    a[4 * bins + k] = S * wr;
                    a[6 * bins + k] = S * wi;
                    a[5 * bins + k] = S * wr;
                    a[7 * bins + k] = S * wi;
                    a[8 * bins + k] = sg * S * qr;
                    a[9 * bins + k] = sg * S * qi;
                    a[10 * bins + k] = sg * S * qr;
                    a[11 * bins + k] = sg * S * qi;
                }
            double *a0 = &c.acc[0];
            a0[0] = a0[2 * bins] = a0[3 * bins] = 300.0;
            a0[4 * bins] = 300.0 * wr;
            a0[6 * bins] = 300.0 * wi;
            a0[8 * bins] = 150.0 * qr;
            a0[9 * bins] = 150.0 * qi;
            const Result r = run(c, 0, len + 1, 2);
            CHECK(std::fabs(r.carrier[0] - 300.0 / (100.0 * 64.0 * 64.0 * 0.25)) <= 1e-15);
            CHECK(std::fabs(r.carrier[1] - wr) <= 1e-15 && std::fabs(r.carrier[2] - wi) <= 1e-15);
            CHECK(std::fabs(r.carrier[3] - qr) <= 1e-15 && std::fabs(r.carrier[4] - qi) <= 1e-15);
            CHECK(std::fabs(r.carrier[5] - 1.0) <= 1e-15 && std::fabs(r.carrier[6] - 0.5) <= 1e-15);
            for (size_t e = 0; e + 29 < len; ++e) { // (the deeper stages: bin 0 of stage 0 is not among them)
                const double on = r.d[2 + pm][2 * e], off = r.d[3 - pm][2 * e];
                CHECK(on > 0.0 && std::fabs(off) <= 1e-14 * on && std::fabs(r.d[2 + pm][2 * e + 1]) <= 1e-14 * on);
                CHECK(std::fabs(r.d[4][2 * e]) <= 1e-14 * on && std::fabs(r.d[4][2 * e + 1]) <= 1e-14 * on);
                CHECK(std::fabs(r.d[5][2 * e]) <= 1e-14 * on && std::fabs(r.d[5][2 * e + 1]) <= 1e-14 * on);
            }
            CHECK(r.band[2 * pm][0] > 0.0 && std::fabs(r.band[2 - 2 * pm][0]) <= 1e-12 * r.band[2 * pm][0] && r.band[0][1] == 0.0);
            // given carriers of any magnitude: the same split; locks NaN
            c.given = 1;
            c.car[0] = r.carrier[0];
            c.car[1] = 3.0 * wr;
            c.car[2] = 3.0 * wi;
            c.car[3] = 0.5 * qr;
            c.car[4] = 0.5 * qi;
            const Result g = run(c, 1, len, 2);
            CHECK(g.carrier[0] == c.car[0] && std::fabs(g.carrier[1] - wr) <= 1e-15 && std::fabs(g.carrier[4] - qi) <= 1e-15);
            CHECK(std::isnan(g.carrier[5]) && std::isnan(g.carrier[6]));
            for (size_t e = 0; e < len; ++e)
                CHECK(std::fabs(g.d[2 + pm][2 * e] - r.d[2 + pm][2 * e]) <= 1e-14 * std::fabs(r.d[2 + pm][2 * e]));
            // no carriers: cab[0] == 0, then sab_up[0] == 0, then no average in stage 0: the record (0, NaN x 6), NaN rows, cab / cba /
            // freq as before
            c.given = 0;
            for (int k = 0; k < 3; ++k) {
                Case z = c;
                if (k == 0)
                    z.acc[8 * bins] = z.acc[9 * bins] = 0.0;
                else if (k == 1)
                    z.acc[4 * bins] = z.acc[6 * bins] = 0.0;
                else
                    z.count0 = 0;
                const Result n = run(z, 1, len, 2);
                CHECK(n.carrier[0] == 0.0);
                for (int i = 1; i < 7; ++i)
                    CHECK(std::isnan(n.carrier[i]));
                for (size_t e = 0; e < 2 * len; ++e)
                    CHECK(std::isnan(n.d[2][e]) && std::isnan(n.d[3][e]) && std::isnan(n.d[4][e]) && std::isnan(n.d[5][e]));
                CHECK(std::isnan(n.band[0][0]) && std::isnan(n.band[7][0]) && n.band[2][1] == 0.0);
                CHECK(memcmp(n.f[0].data(), g.f[0].data(), 4 * len) == 0);
                if (k == 2)
                    CHECK(memcmp(n.d[0].data(), g.d[0].data(), 16 * len) == 0 && memcmp(n.d[1].data(), g.d[1].data(), 16 * len) == 0);
            }
        }
    }
    for (uint32_t mode = 0; mode < 2; ++mode) { // an excluded middle stage leaves two jobs; no stage at all leaves an empty unit
        Case c = builtin_case(mode, 12);
        c.breaks[1].include = 0;
        c.breaks[2].start = c.breaks[1].start;
        CHECK(run(c, 0, 64, 1).len == 25 + 29);
        c.breaks.clear();
        c.count64.clear();
        c.acc.clear();
        c.count0 = 0;
        const Result r3 = run(c, 1, 4, 300); // (300 units: two record blocks)
        CHECK(r3.len == 0 && r3.band[0][0] == 0.0);
        if (mode == PREAD_AMPM)
            CHECK(r3.carrier[0] == 0.0 && std::isnan(r3.carrier[1]) && std::isnan(r3.carrier[6]));
    }
    // the argument rules that need no object
    PairUnit u{};
    auto is = [](const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; };
    const char *bad = "given carriers must be finite, with p_ab > 0 and w, q not 0";
    const double zero_p[5] = {0.0, 1.0, 0.0, 1.0, 0.0}, neg_p[5] = {-1.0, 1.0, 0.0, 1.0, 0.0}, zero_w[5] = {1.0, 0.0, 0.0, 1.0, 0.0};
    const double zero_q[5] = {1.0, 1.0, 0.0, 0.0, 0.0}, nan_w[5] = {1.0, NAN, 0.0, 1.0, 0.0}, inf_q[5] = {1.0, 1.0, 0.0, 1.0, INFINITY};
    const double inf_p[5] = {INFINITY, 1.0, 0.0, 1.0, 0.0}, good[5] = {2.5, 0.0, -4.0, 3.0, 4.0};
    CHECK(is(pair_given(zero_p, &u), bad) && is(pair_given(neg_p, &u), bad) && is(pair_given(zero_w, &u), bad) && is(pair_given(zero_q, &u), bad));
    CHECK(is(pair_given(nan_w, &u), bad) && is(pair_given(inf_q, &u), bad) && is(pair_given(inf_p, &u), bad) && u.given == 0);
    CHECK(is(pair_given(good, &u), nullptr) && u.given == 1 && u.P == 2.5 && u.wr == 0.0 && u.wi == -1.0 && u.qr == 0.6 && u.qi == 0.8);
    BankBands bb{};
    double sums[8];
    const float two[4] = {0.0f, 0.1f, 0.2f, 0.3f}, many[18] = {};
    CHECK(is(cross_read_band_refusal(two, 2, sums, false, &bb), nullptr) && bb.n == 2);
    CHECK(is(cross_read_band_refusal(many, 9, sums, true, &bb), "more than 8 bands"));
    CHECK(is(cross_read_band_refusal(two, 2, nullptr, true, &bb), "bands without a band output"));
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
        printf("pair_readout_check: %ld checks OK\n", checks);
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
        uint32_t head[8];
        take(in, head, 8);
        Case c;
        c.n = head[0];
        c.mode = head[4];
        c.rows = head[5];
        c.given = head[6];
        c.count0 = head[7];
        CHECK(head[1] <= 64 && head[2] <= 64 && head[3] <= BANK_MAX_BANDS && c.n >= 2 && c.n <= (1u << 20) && c.mode <= 1);
        CHECK(c.rows == PREAD_CSD_ROWS || c.rows == PREAD_ROWS);
        take(in, &c.nenbw, 1);
        take(in, &c.power, 1);
        take(in, c.car, 5);
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
        const bool ampm = c.mode == PREAD_AMPM;
        for (int i = 0; i < (ampm ? 1 : 7); ++i)
            put(out, r.f[i]);
        for (int i = 0; i < (ampm ? 6 : 4); ++i)
            put(out, r.d[i]);
        if (ampm)
            fwrite(r.carrier, sizeof(double), PREAD_RECORD, out);
        for (uint32_t b = 0; b < head[3]; ++b)
            for (uint32_t row = 0; row < PREAD_BAND_ROWS; ++row)
                fwrite(&r.band[row][b], sizeof(double), 1, out);
    }
    fclose(in);
    if (fclose(out) != 0) {
        printf("FAIL cannot write the output\n");
        return 1;
    }
    printf("pair_readout_check: %u cases, %ld checks OK\n", cases, checks);
    return 0;
}
