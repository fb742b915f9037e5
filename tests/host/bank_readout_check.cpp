// bank_readout_check.cpp -- csrc/bank_readout.h on the CPU: the job table from Break lists, the per-element functions of
// bank_stitch_kernel over every job (tile by tile, as the kernel's grid walks them) and the band sums as bank_band_kernel orders
// them.  Stand-alone (no library, no device):
//
//   bank_readout_check            a built-in case; asserts that the jobs write every element of a row exactly once
//   bank_readout_check IN OUT     cases from IN (written by tests/test_bank_readout_host.py, which gets the Breaks from the
//                                 library's host-only stitch), rows, frequencies and band sums to OUT
//
// IN:  u32 cases; a case: u32 n, stages, breaks, bands; f32 nenbw, power; u64 count64[stages]; psdc_break[breaks];
//      f32 spectra[stages][n/2 + 1]; f32 bands[bands][2]
// OUT: a case: u64 L; f32 psd[L]; f32 freq[L]; f64 band[bands]
#include "../../include/psdcascade.h"
#include "bank_readout.h"

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
    uint32_t n = 0;
    float nenbw = 0, power = 0;
    std::vector<uint64_t> count64;
    std::vector<psdc_break> breaks;
    std::vector<float> spectra; // [stages][n/2 + 1]
    BankBands bands{};
};

struct Result {
    std::vector<float> psd, freq;
    double band[BANK_MAX_BANDS];
};

// PsdStage::gain in f32, as the library's stage_gain forms it
static float gain(uint32_t n, uint64_t count, float nenbw, float power) { return (float)((uint64_t)(n / 2u) * count) * nenbw * power; }

static Result run(const Case &c, uint32_t row, size_t stride, size_t rows)
{
    const size_t bins = c.n / 2 + 1;
    // every stage's accumulator row in memory of its own, so that the sanitizer sees a read past a row
    std::vector<std::vector<float>> acc(c.count64.size());
    for (size_t s = 0; s < acc.size(); ++s)
        acc[s].assign(c.spectra.begin() + s * bins, c.spectra.begin() + (s + 1) * bins);
    std::vector<BankJob> jobs;
    const BankRow r = bank_row_jobs(
        c.breaks.data(), c.breaks.size(), row, jobs, [&](uint32_t s) { return (const float *)acc[s].data(); },
        [&](uint32_t s) { return gain(c.n, c.count64[s], c.nenbw, c.power); });
    CHECK(r.job0 == 0 && r.njobs == jobs.size());
    uint32_t max_bins = 0;
    for (const BankJob &j : jobs)
        max_bins = j.bins_end - j.bins_start > max_bins ? j.bins_end - j.bins_start : max_bins;
    // the stitch kernel's grid: tiles x jobs workgroups of BANK_STITCH_THREADS threads
    std::vector<float> psd(rows * stride, -1.0f), freq(rows * stride, -1.0f);
    std::vector<int> hits(rows * stride, 0);
    const uint32_t tiles = (max_bins + BANK_STITCH_THREADS - 1) / BANK_STITCH_THREADS;
    for (uint32_t block = 0; block < tiles * jobs.size(); ++block)
        for (uint32_t t = 0; t < BANK_STITCH_THREADS; ++t) {
            const BankJob &j = jobs[block / tiles];
            const uint32_t i = (block % tiles) * BANK_STITCH_THREADS + t;
            if (i >= j.bins_end - j.bins_start)
                continue;
            const size_t o = (size_t)j.row * stride + j.start + i;
            CHECK(o < psd.size());
            psd[o] = bank_psd(j, j.bins_start + i);
            freq[o] = bank_freq(j, j.bins_start + i);
            ++hits[o];
        }
    for (size_t o = 0; o < hits.size(); ++o) // the row's elements once each, nothing else
        CHECK(hits[o] == (o >= (size_t)row * stride && o < (size_t)row * stride + r.len ? 1 : 0));
    Result out;
    out.psd.assign(psd.begin() + (size_t)row * stride, psd.begin() + (size_t)row * stride + r.len);
    out.freq.assign(freq.begin() + (size_t)row * stride, freq.begin() + (size_t)row * stride + r.len);
    bank_band_row_host(jobs.data(), (uint32_t)jobs.size(), r.len, c.bands, out.band);
    return out;
}

static void builtin()
{
    // three stages of n = 64 as the stitch lays them out with the default options: bins [0, 25) of the deepest, then [4, 25), then
    // [4, 33) of stage 0
    Case c;
    c.n = 64;
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
    c.spectra.resize(3 * 33);
    for (size_t k = 0; k < c.spectra.size(); ++k)
        c.spectra[k] = 1.0f + (float)(k % 7);
    c.bands.n = 2;
    c.bands.lo[0] = 0.0f;
    c.bands.hi[0] = 1.0f;
    c.bands.lo[1] = 0.3f;
    c.bands.hi[1] = 0.2999f; // (holds nothing)
    const Result r = run(c, 1, start + 5, 3);
    CHECK(r.psd.size() == start && r.freq.size() == start);
    CHECK(r.freq[0] == 0.0f && r.freq[start - 1] == 0.5f);
    double whole = 0.0, p1 = 0.0, f1 = 0.0; // the trapezoids in sequence
    for (size_t k = 0; k < r.psd.size(); ++k) {
        whole += 0.5 * ((double)r.psd[k] + p1) * ((double)r.freq[k] - f1);
        p1 = r.psd[k];
        f1 = r.freq[k];
    }
    CHECK(r.band[1] == 0.0);
    CHECK(r.band[0] > 0.0 && (r.band[0] - whole) <= 1e-12 * whole && (whole - r.band[0]) <= 1e-12 * whole);
    // an excluded middle stage leaves two jobs; no stage at all leaves an empty row
    c.breaks[1].include = 0;
    c.breaks[2].start = c.breaks[1].start;
    const Result r2 = run(c, 0, 64, 1);
    CHECK(r2.psd.size() == 25 + 29);
    c.breaks.clear();
    const Result r3 = run(c, 0, 4, 2);
    CHECK(r3.psd.empty() && r3.band[0] == 0.0);
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
        printf("bank_readout_check: %ld checks OK\n", checks);
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
        uint32_t head[4];
        take(in, head, 4);
        Case c;
        c.n = head[0];
        CHECK(head[1] <= 64 && head[2] <= 64 && head[3] <= BANK_MAX_BANDS && c.n >= 2 && c.n <= (1u << 20));
        take(in, &c.nenbw, 1);
        take(in, &c.power, 1);
        c.count64.resize(head[1]);
        take(in, c.count64.data(), head[1]);
        c.breaks.resize(head[2]);
        take(in, c.breaks.data(), head[2]);
        c.spectra.resize((size_t)head[1] * (c.n / 2 + 1));
        take(in, c.spectra.data(), c.spectra.size());
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
        CHECK(r.psd.size() == len);
        const uint64_t L = len;
        fwrite(&L, sizeof L, 1, out);
        if (len) {
            fwrite(r.psd.data(), sizeof(float), len, out);
            fwrite(r.freq.data(), sizeof(float), len, out);
        }
        fwrite(r.band, sizeof(double), head[3], out);
    }
    fclose(in);
    if (fclose(out) != 0) {
        printf("FAIL cannot write the output\n");
        return 1;
    }
    printf("bank_readout_check: %u cases, %ld checks OK\n", cases, checks);
    return 0;
}
