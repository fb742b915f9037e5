// tests/host/cross_read_check.cpp -- the host read-outs of the cross-spectral runtime (stabilizer-stream_amd/csrc/cross_runtime.cpp,
// UNCHANGED) on the CPU, under AddressSanitizer and UBSan, against the host model of the HIP runtime (tests/host/sim/) and the
// launcher models of sim/sim_cross_kernels.cpp, whose fold gives every accumulator a definite f64 value.  TEST INFRASTRUCTURE.
// What it pins down is what no GPU test reaches: the bytes, return codes and error texts of every stage read-out and every stitched
// read-out of the fifteen families, at exact, too small and absent output capacities.
//
// Every family gets two objects of 3 units at n = 64: one with set_avg / set_detrend at their defaults, one whose settings change
// mid-stream.  Unit 0 is fed 64 * 8 * 8 + 64 samples (three stages), unit 1 one segment (count 1), unit 2 nothing.  Every output
// buffer is exactly as long as the call's capacity says plus a guard, filled with the byte MARK, and written to the dump in full
// (struct Dump).  Two builds of the runtime that answer every call
// alike write the same dump; tests/golden/cross_read_dump.bin is that of the runtime before its read-outs were unified.
// usage: cross_read_check DUMP [--trace FILE]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/psdcascade.h"
#include "../../include/psdcascade_robust.h"
#include "plan.h"

#include <hip/hip_runtime.h> // (sim/hip/: the host model of the HIP runtime)
#include "sim_device.h"

using namespace psdk;
using sim::ident;
using sim::put_bits;
using sim::world;

namespace {

constexpr uint32_t N = 64, BINS = N / 2 + 1, UNITS = 3;
constexpr size_t FED0 = 64 * 8 * 8 + 64, FED1 = 64; // unit 0: three stages; unit 1: one segment
constexpr uint8_t MARK = 0xCD;
constexpr size_t GUARD = 4;      // elements behind every output buffer
constexpr size_t SPARE = 3;      // elements a call with room to spare has beyond the row's length
constexpr size_t BREAKS = 16;

int g_failures = 0;
void fail(const std::string &what)
{
    if (g_failures++ < 30)
        fprintf(stderr, "FAIL %s\n", what.c_str());
}

// The dump: a text line or two a call and its buffers as raw bytes.  A buffer whose bytes equal an earlier one's is written as
// "name=#k" (k: the number of the earlier one), an error text that is the record's before as "=".
struct Dump {
    FILE *f = nullptr;
    std::map<std::string, int> seen;
    int next = 0;
    std::string last_err;
    void text(const std::string &s) { fputs(s.c_str(), f); }
    void answer(int rc, const char *err, const std::string &more)
    {
        text("rc " + std::to_string(rc) + " err " + (last_err == err ? std::string("=") : "\"" + std::string(err) + "\"") + more + "\n");
        last_err = err;
    }
    void buf(const char *name, const std::vector<uint8_t> &b)
    {
        if (b.empty())
            return;
        const std::string key(b.begin(), b.end());
        const auto it = seen.find(key);
        if (it != seen.end()) {
            ++next;
            text(std::string(name) + "=#" + std::to_string(it->second) + "\n");
            return;
        }
        seen.emplace(key, next);
        text(std::string(name) + " #" + std::to_string(next++) + " bytes " + std::to_string(b.size()) + "\n");
        fwrite(b.data(), 1, b.size(), f);
        text("\n");
    }
};

// one output of a read-out: `per` elements of `elem` bytes a bin (stitched: a unit of capacity), or `bytes` in all (stage)
struct Out {
    const char *name;
    size_t elem, per;
    bool required = false; // the call refuses a NULL here
};
using Ptrs = void *const *;
struct Stitched {
    const char *name;
    std::vector<Out> outs;
    std::function<int(void *, uint32_t, int, uint32_t, int, Ptrs, size_t, size_t *, psdc_break *, size_t, size_t *)> call;
};
struct StageRead {
    const char *name;
    std::vector<Out> outs; // elem * per bytes each
    std::function<int(void *, uint32_t, uint32_t, Ptrs)> call;
};
struct Family {
    const char *name;
    std::function<void *()> create;
    std::function<int(void *, uint32_t, const float *, size_t)> feed; // host f32: every stream of the unit from the same samples
    std::function<int(void *, uint32_t, uint32_t)> set_avg;           // (none: the waterfalls)
    std::function<int(void *, int)> set_detrend;
    std::function<int(void *, uint32_t)> num_stages;
    std::function<void(void *)> destroy;
    std::function<const char *(void *)> last_error;
    std::vector<StageRead> stage_reads;
    std::vector<Stitched> stitched;
};

std::vector<uint8_t> marked(size_t bytes) { return std::vector<uint8_t>(bytes, MARK); }

struct Answer {
    int rc;
    size_t len, nb;
};

// one call of a stitched read-out: outputs `given` (bit i: output i), of capacity cap; breaks of capacity bcap (want_breaks)
Answer stitched_call(Dump &d, const Family &fam, void *h, const Stitched &s, const std::string &what, uint32_t unit, int ko, uint32_t mc, int kt,
                     unsigned given, size_t cap, bool want_breaks, size_t bcap, bool want_counts = true)
{
    std::vector<std::vector<uint8_t>> bufs(s.outs.size());
    std::vector<void *> p(s.outs.size(), nullptr);
    for (size_t i = 0; i < s.outs.size(); ++i)
        if (given >> i & 1) {
            bufs[i] = marked(s.outs[i].elem * (s.outs[i].per * cap + GUARD));
            p[i] = bufs[i].data();
        }
    std::vector<uint8_t> br = marked(want_breaks ? sizeof(psdc_break) * (bcap + 1) : 0);
    size_t len, nb;
    memset(&len, MARK, sizeof len);
    memset(&nb, MARK, sizeof nb);
    const int rc = s.call(h, unit, ko, mc, kt, p.data(), cap, want_counts ? &len : nullptr, want_breaks ? reinterpret_cast<psdc_break *>(br.data()) : nullptr,
                          bcap, want_counts ? &nb : nullptr);
    d.text(std::string("== ") + s.name + " u" + std::to_string(unit) + " opts " + std::to_string(ko) + std::to_string(mc) + std::to_string(kt) + " cap " +
           std::to_string(cap) + " bcap " + (want_breaks ? std::to_string(bcap) : "-") + " outs " + std::to_string(given) + ": " + what + "\n");
    d.answer(rc, fam.last_error(h), " len " + std::to_string(len) + " n_breaks " + std::to_string(nb));
    d.buf("breaks", br);
    for (size_t i = 0; i < s.outs.size(); ++i)
        if (p[i])
            d.buf(s.outs[i].name, bufs[i]);
    return {rc, len, nb};
}

// the calls of one stitched read-out on one unit.  A call with room to spare gives `SPARE` elements more than the size query
// asked for (no more: the dump holds every buffer in full)
void stitched_unit(Dump &d, const Family &fam, void *h, const Stitched &s, uint32_t unit, bool grid, bool edges)
{
    const unsigned all = (1u << s.outs.size()) - 1;
    auto roomy = [&](const char *what, int ko, uint32_t mc, int kt) {
        const Answer q = stitched_call(d, fam, h, s, std::string(what) + ", size query", unit, ko, mc, kt, 0, 0, false, 0);
        if (q.rc != PSDC_OK || q.len > 3 * BINS || q.nb > BREAKS) {
            fail(std::string(fam.name) + " " + s.name + ": the size query of unit " + std::to_string(unit) + " gave rc " + std::to_string(q.rc) + ", len " +
                 std::to_string(q.len) + ", n_breaks " + std::to_string(q.nb));
            return Answer{-1, 0, 0};
        }
        stitched_call(d, fam, h, s, what, unit, ko, mc, kt, all, q.len + SPARE, true, q.nb + 1);
        return q;
    };
    const Answer q = roomy("default options", 0, 1, 0);
    if (grid)
        for (int ko = 0; ko < 2; ++ko)
            for (uint32_t mc = 0; mc <= 2; mc += 2)
                for (int kt = 0; kt < 2; ++kt)
                    roomy("grid", ko, mc, kt);
    if (!edges || q.rc != PSDC_OK)
        return;
    if (q.len == 0 || q.nb == 0) {
        fail(std::string(fam.name) + " " + s.name + ": nothing to read out of unit " + std::to_string(unit));
        return;
    }
    stitched_call(d, fam, h, s, "only the last output", unit, 0, 1, 0, 1u << (s.outs.size() - 1), q.len + SPARE, false, 0);
    stitched_call(d, fam, h, s, "cap = len - 1", unit, 0, 1, 0, all, q.len - 1, true, q.nb + 1);
    stitched_call(d, fam, h, s, "cap = len", unit, 0, 1, 0, all, q.len, true, q.nb);
    stitched_call(d, fam, h, s, "breaks_cap = n_breaks - 1", unit, 0, 1, 0, all, q.len + SPARE, true, q.nb - 1);
    stitched_call(d, fam, h, s, "no len, no n_breaks", unit, 0, 1, 0, all, q.len, true, q.nb, false);
}

void stage_call(Dump &d, const Family &fam, void *h, const StageRead &s, const std::string &what, uint32_t unit, uint32_t stage, unsigned given)
{
    std::vector<std::vector<uint8_t>> bufs(s.outs.size());
    std::vector<void *> p(s.outs.size(), nullptr);
    for (size_t i = 0; i < s.outs.size(); ++i)
        if ((given >> i & 1) || s.outs[i].required) {
            bufs[i] = marked(s.outs[i].elem * (s.outs[i].per + GUARD));
            p[i] = bufs[i].data();
        }
    const int rc = s.call(h, unit, stage, p.data());
    d.text(std::string("== ") + s.name + " u" + std::to_string(unit) + " stage " + std::to_string(stage) + " outs " + std::to_string(given) + ": " + what +
           "\n");
    d.answer(rc, fam.last_error(h), "");
    for (size_t i = 0; i < s.outs.size(); ++i)
        if (p[i])
            d.buf(s.outs[i].name, bufs[i]);
}

// what the units are fed from: the identities the segment models require (sim_cross_kernels.cpp)
struct Sources {
    std::vector<float> f32[UNITS];
    Sources()
    {
        for (uint32_t u = 0; u < UNITS; ++u) {
            f32[u].resize(FED0);
            for (size_t j = 0; j < FED0; ++j)
                put_bits(&f32[u][j], ident(16 * (int)u, j));
        }
    }
};

void run_family(Dump &d, const Family &fam, const Sources &src, bool midstream)
{
    const std::string ctx = std::string(fam.name) + (midstream ? " (settings changed mid-stream)" : " (default settings)");
    d.text("#### " + ctx + "\n");
    void *h = fam.create();
    if (!h) {
        fail(ctx + ": create failed: " + fam.last_error(nullptr));
        return;
    }
    auto ok = [&](int rc, const char *what) {
        if (rc < 0)
            fail(ctx + ": " + what + " -> " + std::to_string(rc) + " (" + fam.last_error(h) + ")");
    };
    size_t fed = 0;
    for (size_t len : {(size_t)1000, (size_t)2000, FED0 - 3000}) {
        ok(fam.feed(h, 0, src.f32[0].data() + fed, len), "feed");
        fed += len;
        if (midstream && fed == 1000) {
            if (fam.set_avg)
                ok(fam.set_avg(h, 100, 40), "set_avg"); // stage k averages min(40 >> 3 k, 100): 40, 5, 0
            ok(fam.set_detrend(h, PSDC_DETREND_MEAN), "set_detrend");
        }
    }
    ok(fam.feed(h, 1, src.f32[1].data(), FED1), "feed");
    for (uint32_t unit = 0; unit < UNITS; ++unit) {
        const int ns = fam.num_stages(h, unit);
        d.text("unit " + std::to_string(unit) + " stages " + std::to_string(ns) + "\n");
        if (ns != (unit == 0 ? 3 : unit == 1 ? 1 : 0))
            fail(ctx + ": unit " + std::to_string(unit) + " has " + std::to_string(ns) + " stages");
        for (const StageRead &s : fam.stage_reads) {
            const unsigned all = (1u << s.outs.size()) - 1;
            for (int stage = 0; stage <= ns; ++stage) // (the last one is out of range)
                stage_call(d, fam, h, s, stage == ns ? "stage = number of stages" : "every output", unit, (uint32_t)stage, all);
            if (ns) {
                stage_call(d, fam, h, s, "only the last output", unit, 0, 1u << (s.outs.size() - 1));
                stage_call(d, fam, h, s, "no output", unit, 0, 0);
            }
        }
        for (const Stitched &s : fam.stitched)
            stitched_unit(d, fam, h, s, unit, unit == 0 && !midstream, unit == 0 && !midstream);
    }
    for (const std::string &e : world().errors)
        fail(ctx + ": " + e);
    world() = sim::World(); // (the next object's folds count from 0 again)
    fam.destroy(h);
}

template <class T>
T *at(Ptrs p, size_t i)
{
    return static_cast<T *>(p[i]);
}

// the parts every family has, by the names of its C functions
#define FAMILY_COMMON(F, T)                                                                                                                          \
    F.name = #T;                                                                                                                                     \
    F.set_detrend = [](void *h, int k) { return T##_set_detrend(static_cast<T *>(h), k); };                                                          \
    F.num_stages = [](void *h, uint32_t u) { return T##_num_stages(static_cast<T *>(h), u); };                                                       \
    F.destroy = [](void *h) { T##_destroy(static_cast<T *>(h)); };                                                                                   \
    F.last_error = [](void *h) { return T##_last_error(static_cast<const T *>(h)); }
#define FAMILY_AVG(F, T) F.set_avg = [](void *h, uint32_t l, uint32_t c) { return T##_set_avg(static_cast<T *>(h), l, c); }
// a carrier a unit (ftw = 100 (u + 1): the mixer models know the unit by it), or one a side of a pair
#define FAMILY_CREATE_CARRIER(F, T)                                                                                                                  \
    F.create = []() -> void * {                                                                                                                      \
        T *h = T##_create(N, PSDC_WINDOW_HANN, UNITS, 0);                                                                                            \
        for (uint32_t u = 0; h && u < UNITS; ++u)                                                                                                    \
            T##_set_carrier(h, u, 100 * (u + 1), 7);                                                                                                 \
        return h;                                                                                                                                    \
    }
#define FAMILY_CREATE_PAIR_CARRIERS(F, T)                                                                                                            \
    F.create = []() -> void * {                                                                                                                      \
        T *h = T##_create(N, PSDC_WINDOW_HANN, UNITS, 0);                                                                                            \
        for (uint32_t u = 0; h && u < UNITS; ++u) {                                                                                                  \
            T##_set_carrier(h, u, 0, 100 * (u + 1), 7);                                                                                              \
            T##_set_carrier(h, u, 1, 100 * (u + 1) + 1, 9);                                                                                          \
        }                                                                                                                                            \
        return h;                                                                                                                                    \
    }
#define FEED1(F, T) F.feed = [](void *h, uint32_t u, const float *x, size_t n) { return T##_process(static_cast<T *>(h), u, x, n); }
#define FEED2(F, T) F.feed = [](void *h, uint32_t u, const float *x, size_t n) { return T##_process(static_cast<T *>(h), u, x, x, n); }
#define FEED4(F, T) F.feed = [](void *h, uint32_t u, const float *x, size_t n) { return T##_process(static_cast<T *>(h), u, x, x, x, x, n); }
#define STAT Out{"stat", sizeof(psdc_stage_stat), 1}

// the zoom read-out of two f32 rows: T_psd of the zoom, IQ, zoom / IQ SK and AM/PM families
#define TWO_ROWS_PSD(T)                                                                                                                              \
    Stitched                                                                                                                                         \
    {                                                                                                                                                \
        "psd", {{"upper", 4, 1}, {"lower", 4, 1}},                                                                                                   \
            [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {           \
                return T##_psd(static_cast<T *>(h), u, ko, mc, kt, at<float>(p, 0), at<float>(p, 1), cap, len, br, bc, nb);                          \
            }                                                                                                                                        \
    }
#define FOUR_ROWS_STAGE(T, fn, a, b, c, e)                                                                                                           \
    StageRead                                                                                                                                        \
    {                                                                                                                                                \
        #fn, {STAT, {a, 8, BINS}, {b, 8, BINS}, {c, 8, BINS}, {e, 8, BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {                          \
            return T##_##fn(static_cast<T *>(h), u, st, at<psdc_stage_stat>(p, 0), at<double>(p, 1), at<double>(p, 2), at<double>(p, 3),             \
                            at<double>(p, 4));                                                                                                       \
        }                                                                                                                                            \
    }

std::vector<Family> families()
{
    std::vector<Family> v;
    {
        Family f;
        FAMILY_COMMON(f, psdc_cross);
        FAMILY_AVG(f, psdc_cross);
        f.create = []() -> void * { return psdc_cross_create(N, PSDC_WINDOW_HANN, UNITS, 0); };
        FEED2(f, psdc_cross);
        f.stage_reads.push_back({"stage_spectra", {STAT, {"sxx", 4, BINS}, {"syy", 4, BINS}, {"sxy", 4, 2 * BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {
                                     return psdc_cross_stage_spectra(static_cast<psdc_cross *>(h), u, st, at<psdc_stage_stat>(p, 0), at<float>(p, 1),
                                                                     at<float>(p, 2), at<float>(p, 3));
                                 }});
        f.stitched.push_back({"csd", {{"sxx", 4, 1}, {"syy", 4, 1}, {"sxy", 4, 2}},
                              [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {
                                  return psdc_cross_csd(static_cast<psdc_cross *>(h), u, ko, mc, kt, at<float>(p, 0), at<float>(p, 1), at<float>(p, 2), cap,
                                                        len, br, bc, nb);
                              }});
        v.push_back(f);
    }
    {
        Family f;
        FAMILY_COMMON(f, psdc_csm);
        FAMILY_AVG(f, psdc_csm);
        f.create = []() -> void * { return psdc_csm_create(N, PSDC_WINDOW_HANN, 3, UNITS, 0); };
        f.feed = [](void *h, uint32_t u, const float *x, size_t n) {
            const float *xs[3] = {x, x, x};
            return psdc_csm_process(static_cast<psdc_csm *>(h), u, xs, n);
        };
        f.stage_reads.push_back({"stage_spectra", {STAT, {"rows", 4, 9 * BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {
                                     return psdc_csm_stage_spectra(static_cast<psdc_csm *>(h), u, st, at<psdc_stage_stat>(p, 0), at<float>(p, 1));
                                 }});
        f.stitched.push_back({"csd", {{"rows", 4, 9}},
                              [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {
                                  return psdc_csm_csd(static_cast<psdc_csm *>(h), u, ko, mc, kt, at<float>(p, 0), cap, len, br, bc, nb);
                              }});
        v.push_back(f);
    }
#define ZOOM_FAMILY(T, FEED)                                                                                                                         \
    {                                                                                                                                                \
        Family f;                                                                                                                                    \
        FAMILY_COMMON(f, T);                                                                                                                         \
        FAMILY_AVG(f, T);                                                                                                                            \
        FAMILY_CREATE_CARRIER(f, T);                                                                                                                 \
        FEED(f, T);                                                                                                                                  \
        f.stage_reads.push_back({"stage_spectra", {STAT, {"upper", 4, BINS}, {"lower", 4, BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {     \
                                     return T##_stage_spectra(static_cast<T *>(h), u, st, at<psdc_stage_stat>(p, 0), at<float>(p, 1),                \
                                                              at<float>(p, 2));                                                                      \
                                 }});                                                                                                                \
        f.stitched.push_back(TWO_ROWS_PSD(T));                                                                                                       \
        v.push_back(f);                                                                                                                              \
    }
    ZOOM_FAMILY(psdc_zoom, FEED1)
    ZOOM_FAMILY(psdc_iq, FEED2)
#define ZCSD_FAMILY(T, FEED)                                                                                                                         \
    {                                                                                                                                                \
        Family f;                                                                                                                                    \
        FAMILY_COMMON(f, T);                                                                                                                         \
        FAMILY_AVG(f, T);                                                                                                                            \
        FAMILY_CREATE_PAIR_CARRIERS(f, T);                                                                                                           \
        FEED(f, T);                                                                                                                                  \
        f.stage_reads.push_back({"stage_spectra", {STAT, {"rows", 4, 8 * BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {                      \
                                     return T##_stage_spectra(static_cast<T *>(h), u, st, at<psdc_stage_stat>(p, 0), at<float>(p, 1));               \
                                 }});                                                                                                                \
        f.stitched.push_back(                                                                                                                        \
            {"csd", {{"saa_upper", 4, 1}, {"saa_lower", 4, 1}, {"sbb_upper", 4, 1}, {"sbb_lower", 4, 1}, {"sab_upper", 4, 2}, {"sab_lower", 4, 2}},  \
             [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {          \
                 return T##_csd(static_cast<T *>(h), u, ko, mc, kt, at<float>(p, 0), at<float>(p, 1), at<float>(p, 2), at<float>(p, 3),              \
                                at<float>(p, 4), at<float>(p, 5), cap, len, br, bc, nb);                                                             \
             }});                                                                                                                                    \
        v.push_back(f);                                                                                                                              \
    }
    ZCSD_FAMILY(psdc_zcsd, FEED2)
    ZCSD_FAMILY(psdc_iqcsd, FEED4)
    {
        Family f;
        FAMILY_COMMON(f, psdc_sk);
        FAMILY_AVG(f, psdc_sk);
        f.create = []() -> void * { return psdc_sk_create(N, PSDC_WINDOW_HANN, UNITS, 0); };
        FEED1(f, psdc_sk);
        f.stage_reads.push_back({"stage_moments", {STAT, {"s1", 8, BINS}, {"s2", 8, BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {
                                     return psdc_sk_stage_moments(static_cast<psdc_sk *>(h), u, st, at<psdc_stage_stat>(p, 0), at<double>(p, 1),
                                                                  at<double>(p, 2));
                                 }});
        f.stitched.push_back({"psd", {{"psd", 4, 1}},
                              [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {
                                  return psdc_sk_psd(static_cast<psdc_sk *>(h), u, ko, mc, kt, at<float>(p, 0), cap, len, br, bc, nb);
                              }});
        f.stitched.push_back({"sk", {{"sk", 8, 1}},
                              [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {
                                  return psdc_sk_sk(static_cast<psdc_sk *>(h), u, ko, mc, kt, at<double>(p, 0), cap, len, br, bc, nb);
                              }});
        v.push_back(f);
    }
#define ZSK_FAMILY(T, FEED)                                                                                                                          \
    {                                                                                                                                                \
        Family f;                                                                                                                                    \
        FAMILY_COMMON(f, T);                                                                                                                         \
        FAMILY_AVG(f, T);                                                                                                                            \
        FAMILY_CREATE_CARRIER(f, T);                                                                                                                 \
        FEED(f, T);                                                                                                                                  \
        f.stage_reads.push_back(FOUR_ROWS_STAGE(T, stage_moments, "s1_upper", "s1_lower", "s2_upper", "s2_lower"));                                  \
        f.stitched.push_back(TWO_ROWS_PSD(T));                                                                                                       \
        f.stitched.push_back(                                                                                                                        \
            {"sk", {{"sk_upper", 8, 1}, {"sk_lower", 8, 1}},                                                                                         \
             [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {          \
                 return T##_sk(static_cast<T *>(h), u, ko, mc, kt, at<double>(p, 0), at<double>(p, 1), cap, len, br, bc, nb);                        \
             }});                                                                                                                                    \
        v.push_back(f);                                                                                                                              \
    }
    ZSK_FAMILY(psdc_zsk, FEED1)
    ZSK_FAMILY(psdc_iqsk, FEED2)
#define AMPM_FAMILY(T, FEED)                                                                                                                         \
    {                                                                                                                                                \
        Family f;                                                                                                                                    \
        FAMILY_COMMON(f, T);                                                                                                                         \
        FAMILY_AVG(f, T);                                                                                                                            \
        FAMILY_CREATE_CARRIER(f, T);                                                                                                                 \
        FEED(f, T);                                                                                                                                  \
        f.stage_reads.push_back(FOUR_ROWS_STAGE(T, stage_rows, "upper", "lower", "comp_re", "comp_im"));                                             \
        f.stitched.push_back(TWO_ROWS_PSD(T));                                                                                                       \
        f.stitched.push_back(                                                                                                                        \
            {"sidebands", {{"upper", 8, 1}, {"lower", 8, 1}, {"comp_re", 8, 1}, {"comp_im", 8, 1}},                                                  \
             [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {          \
                 return T##_sidebands(static_cast<T *>(h), u, ko, mc, kt, at<double>(p, 0), at<double>(p, 1), at<double>(p, 2), at<double>(p, 3),    \
                                      cap, len, br, bc, nb);                                                                                         \
             }});                                                                                                                                    \
        v.push_back(f);                                                                                                                              \
    }
    AMPM_FAMILY(psdc_zampm, FEED1)
    AMPM_FAMILY(psdc_iqampm, FEED2)
#define XAMPM_FAMILY(T, FEED)                                                                                                                        \
    {                                                                                                                                                \
        Family f;                                                                                                                                    \
        FAMILY_COMMON(f, T);                                                                                                                         \
        FAMILY_AVG(f, T);                                                                                                                            \
        FAMILY_CREATE_PAIR_CARRIERS(f, T);                                                                                                           \
        FEED(f, T);                                                                                                                                  \
        f.stage_reads.push_back({"stage_rows", {STAT, {"rows", 8, 12 * BINS}}, [](void *h, uint32_t u, uint32_t st, Ptrs p) {                        \
                                     return T##_stage_rows(static_cast<T *>(h), u, st, at<psdc_stage_stat>(p, 0), at<double>(p, 1));                 \
                                 }});                                                                                                                \
        f.stitched.push_back(                                                                                                                        \
            {"sidebands", {{"rows", 8, 12}},                                                                                                         \
             [](void *h, uint32_t u, int ko, uint32_t mc, int kt, Ptrs p, size_t cap, size_t *len, psdc_break *br, size_t bc, size_t *nb) {          \
                 return T##_sidebands(static_cast<T *>(h), u, ko, mc, kt, at<double>(p, 0), cap, len, br, bc, nb);                                   \
             }});                                                                                                                                    \
        v.push_back(f);                                                                                                                              \
    }
    XAMPM_FAMILY(psdc_zxampm, FEED2)
    XAMPM_FAMILY(psdc_iqxampm, FEED4)
    // the waterfalls: blocks of 4 segments in a ring of 3; at most WF_ROWS rows a read-out; no stitched read-out and no set_avg.
    // Their image and robust read-outs run a kernel, which a host build has not: they answer with a device error behind the lookup
    // of the stage, which is what this program is after.
    constexpr uint32_t WF_ROWS = 4;
#define WF_READS(T, ROBUST, ROWS_OUTS, ROWS_ARGS)                                                                                                           \
    f.stage_reads.push_back({"stage_blocks", {{"blocks", sizeof(psdc_wf_blocks), 1, true}},                                                          \
                             [](void *h, uint32_t u, uint32_t st, Ptrs p) { return T##_stage_blocks(static_cast<T *>(h), u, st, at<psdc_wf_blocks>(p, 0)); }}); \
    f.stage_reads.push_back({"stage_rows", ROWS_OUTS, [](void *h, uint32_t u, uint32_t st, Ptrs p) {                                                 \
                                 return T##_stage_rows(static_cast<T *>(h), u, st, WF_ROWS, at<uint64_t>(p, 0), at<uint32_t>(p, 1), ROWS_ARGS,       \
                                                       at<uint32_t>(p, 2));                                                                          \
                             }});                                                                                                                    \
    f.stage_reads.push_back({"image",                                                                                                                \
                             {{"block_index", 8, WF_ROWS, true}, {"counts", 4, WF_ROWS, true}, {"n_rows", 4, 1, true}, {"psd", 4, WF_ROWS * 2 * BINS}, \
                              {"sk", 4, WF_ROWS * 2 * BINS, true}},                                                                                  \
                             [](void *h, uint32_t u, uint32_t st, Ptrs p) {                                                                          \
                                 return T##_image(static_cast<T *>(h), u, st, WF_ROWS, at<float>(p, 3), at<float>(p, 4), at<uint64_t>(p, 0),         \
                                                  at<uint32_t>(p, 1), at<uint32_t>(p, 2));                                                           \
                             }});                                                                                                                    \
    f.stage_reads.push_back({"robust",                                                                                                               \
                             {{"info", sizeof(psdcx_robust_info), 1, true}, {"median", 4, 2 * BINS, true}},                                          \
                             [](void *h, uint32_t u, uint32_t st, Ptrs p) {                                                                          \
                                 return ROBUST(static_cast<T *>(h), u, st, WF_ROWS, -1.0, 1.0, at<float>(p, 1), nullptr, nullptr, nullptr, \
                                                           nullptr, at<psdcx_robust_info>(p, 0));                                                    \
                             }})
    {
        Family f;
        FAMILY_COMMON(f, psdc_wf);
        f.create = []() -> void * { return psdc_wf_create(N, PSDC_WINDOW_HANN, UNITS, 4, 3, 0); };
        FEED1(f, psdc_wf);
#define WF_OUTS                                                                                                                                      \
    {                                                                                                                                                \
        {"block_index", 8, WF_ROWS, true}, {"counts", 4, WF_ROWS, true}, {"n_rows", 4, 1, true}, {"s1", 8, WF_ROWS * BINS}, {"s2", 8, WF_ROWS * BINS} \
    }
#define WF_ARGS at<double>(p, 3), at<double>(p, 4)
        WF_READS(psdc_wf, psdcx_wf_robust, WF_OUTS, WF_ARGS);
        v.push_back(f);
    }
    {
        Family f;
        FAMILY_COMMON(f, psdc_zwf);
        f.create = []() -> void * {
            psdc_zwf *h = psdc_zwf_create(N, PSDC_WINDOW_HANN, UNITS, 4, 3, 0);
            for (uint32_t u = 0; h && u < UNITS; ++u)
                psdc_zwf_set_carrier(h, u, 100 * (u + 1), 7);
            return h;
        };
        FEED1(f, psdc_zwf);
#define ZWF_OUTS                                                                                                                                     \
    {                                                                                                                                                \
        {"block_index", 8, WF_ROWS, true}, {"counts", 4, WF_ROWS, true}, {"n_rows", 4, 1, true}, {"s1_upper", 8, WF_ROWS * BINS},                    \
            {"s1_lower", 8, WF_ROWS * BINS}, {"s2_upper", 8, WF_ROWS * BINS}, {"s2_lower", 8, WF_ROWS * BINS}                                        \
    }
#define ZWF_ARGS at<double>(p, 3), at<double>(p, 4), at<double>(p, 5), at<double>(p, 6)
        WF_READS(psdc_zwf, psdcx_zwf_robust, ZWF_OUTS, ZWF_ARGS);
        v.push_back(f);
    }
    return v;
}

} // namespace

int main(int argc, char **argv)
{
    const char *dump_file = nullptr, *trace_file = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--trace") && i + 1 < argc)
            trace_file = argv[++i];
        else
            dump_file = argv[i];
    }
    if (!dump_file) {
        fprintf(stderr, "usage: cross_read_check DUMP [--trace FILE]\n");
        return 2;
    }
    std::vector<std::vector<std::string>> trace;
    sim::rt().trace = &trace;
    Dump d;
    if (!(d.f = fopen(dump_file, "wb"))) {
        fprintf(stderr, "cross_read_check: cannot write %s\n", dump_file);
        return 2;
    }
    const Sources src;
    const std::vector<Family> fams = families();
    for (const Family &fam : fams)
        for (int midstream = 0; midstream < 2; ++midstream)
            run_family(d, fam, src, midstream != 0);
    const long bytes = ftell(d.f);
    fclose(d.f);
    if (sim::rt().live_blocks != 0)
        fail(std::to_string(sim::rt().live_blocks) + " device / pinned allocations alive after every object was destroyed");
    size_t lines = 0;
    for (const auto &g : trace)
        lines += g.size();
    if (trace_file) {
        FILE *f = fopen(trace_file, "w");
        if (!f) {
            fail(std::string("cannot write ") + trace_file);
        } else {
            for (size_t g = 0; g < trace.size(); ++g) {
                fprintf(f, g ? "== stream %zu\n" : "== host\n", g - 1);
                for (const std::string &l : trace[g])
                    fprintf(f, "%s\n", l.c_str());
            }
            fclose(f);
        }
    }
    if (g_failures) {
        fprintf(stderr, "cross_read_check: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("cross_read_check: %zu families, %d buffers in a dump of %ld bytes, %zu trace lines: every read-out answered\n", fams.size(), d.next, bytes, lines);
    return 0;
}
