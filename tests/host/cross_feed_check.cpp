// tests/host/cross_feed_check.cpp -- the feeds of the cross-spectral host runtime (stabilizer-stream_amd/csrc/cross_runtime.cpp,
// UNCHANGED) on the CPU, under AddressSanitizer and UBSan, against the host model of the HIP runtime (tests/host/sim/).  TEST
// INFRASTRUCTURE.  What it covers is the part of that file no GPU test can pin down on every run: which stream a piece of a call
// goes on, which events it waits for, when a pinned staging slot is written again, and where in stage 0 the piece lands.
//
// The launchers of cross.h, csm.h, zoom.h, zoom_cross.h, iq.h, iq_cross.h, sk.h, zoom_sk.h, zoom_ampm.h and sample_int.h are the
// models of sim/sim_cross_kernels.cpp (which says what they check); the decimator is the model of sim_kernels.cpp.  Sample j of
// unit u is fed as the bit pattern ident(16 u, j) (an s16 sample as the low 16 bits of j; an sc16 pair holds the 32 bits), and a
// unit's carrier is set to ftw = 100 (u + 1) + side, as those models expect.
//
// Every model, and the runtime model's asynchronous copies, event records and event waits, write a line to a trace, stream by
// stream; `--trace FILE` stores it.  Two builds of the runtime that make the same HIP calls on every stream write the same file.
// usage: cross_feed_check [--trace FILE]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/psdcascade.h"
#include "iq.h"
#include "iq_cross.h"
#include "plan.h"
#include "sample_int.h"
#include "sk.h"
#include "zoom_ampm.h"
#include "zoom_sk.h"

#include "sim_device.h"

using namespace psdk;
using sim::ident;
using sim::put_bits;
using sim::world;

// ---- the scenarios -----------------------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t N = 64, HOP = 32; // the smallest supported size, Hann window (overlap n / 2)
constexpr size_t STAGING = (size_t)1 << 22; // cross_runtime.cpp's: a host call longer than this goes up in pieces
constexpr size_t STREAM = STAGING + 16384;  // samples a unit may take in one scenario (the identities hold 2^24)
constexpr int UNITS = 2;

int g_failures = 0;
std::string g_ctx;

void fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g_failures < 30)
        fprintf(stderr, "FAIL [%s] %s\n", g_ctx.c_str(), buf);
    ++g_failures;
}

// what a unit is fed from, in host memory and in "device" memory (exact sizes: ASan sees a read past the end of either)
struct Sources {
    std::vector<float> f32[UNITS], z32[UNITS];
    std::vector<int16_t> s16[UNITS];
    float *d_f32[UNITS] = {}, *d_z32[UNITS] = {};
    int16_t *d_s16[UNITS] = {};
    Sources()
    {
        for (int u = 0; u < UNITS; ++u) {
            f32[u].resize(STREAM);
            z32[u].resize(2 * STREAM);
            s16[u].resize(STREAM);
            for (size_t j = 0; j < STREAM; ++j) {
                put_bits(&f32[u][j], ident(16 * u, j));
                z32[u][2 * j] = z32[u][2 * j + 1] = f32[u][j];
                s16[u][j] = (int16_t)(uint16_t)j;
            }
        }
    }
    void upload() // device copies of the short head of every stream that the device routes feed
    {
        for (int u = 0; u < UNITS; ++u) {
            (void)hipMalloc(&d_f32[u], sizeof(float) * DEV);
            (void)hipMalloc(&d_z32[u], sizeof(float) * 2 * DEV);
            (void)hipMalloc(&d_s16[u], sizeof(int16_t) * DEV);
            memcpy(d_f32[u], f32[u].data(), sizeof(float) * DEV);
            memcpy(d_z32[u], z32[u].data(), sizeof(float) * 2 * DEV);
            memcpy(d_s16[u], s16[u].data(), sizeof(int16_t) * DEV);
        }
    }
    void release()
    {
        for (int u = 0; u < UNITS; ++u) {
            (void)hipFree(d_f32[u]);
            (void)hipFree(d_z32[u]);
            (void)hipFree(d_s16[u]);
            d_f32[u] = d_z32[u] = nullptr;
            d_s16[u] = nullptr;
        }
    }
    static constexpr size_t DEV = 16384; // every device call ends below this stream index
};

enum Route { F32, F32_Z, S16 }; // f32 planar, f32 interleaved, 16-bit integers (interleaved where the unit is complex)

// one family: how to make, feed and end an object.  feed(route, dev, unit, off, len, producer_event)
struct Family {
    const char *name;
    std::vector<Route> routes;
    std::function<void *()> create;
    std::function<int(void *, Route, bool, uint32_t, size_t, size_t, void *)> feed;
    std::function<int(void *)> sync;
    std::function<void(void *)> destroy;
    std::function<const char *(void *)> last_error;
};

template <class H>
Family family(const char *name, std::vector<Route> routes, std::function<H *()> create,
              std::function<int(H *, Route, bool, uint32_t, size_t, size_t, void *)> feed, int (*sync)(H *), void (*destroy)(H *),
              const char *(*last_error)(const H *))
{
    Family f;
    f.name = name;
    f.routes = std::move(routes);
    f.create = [create] { return static_cast<void *>(create()); };
    f.feed = [feed](void *h, Route r, bool dev, uint32_t u, size_t off, size_t len, void *ev) { return feed(static_cast<H *>(h), r, dev, u, off, len, ev); };
    f.sync = [sync](void *h) { return sync(static_cast<H *>(h)); };
    f.destroy = [destroy](void *h) { destroy(static_cast<H *>(h)); };
    f.last_error = [last_error](void *h) { return last_error(static_cast<const H *>(h)); };
    return f;
}

void check_world(const char *what, const uint64_t *fed)
{
    for (const std::string &e : world().errors)
        fail("%s: %s", what, e.c_str());
    Geometry g;
    g.n = N, g.overlap = N - HOP, g.hop = HOP;
    for (int u = 0; u < UNITS; ++u) {
        const uint64_t want = segments_for(g, fed[u]);
        const std::vector<uint8_t> &got = world().seg[16 * u];
        for (uint64_t j = 0; j < want; ++j)
            if (j >= got.size() || got[j] != 1) {
                fail("%s: segment %llu of unit %d was transformed %d times (%llu samples fed)", what, (unsigned long long)j, u,
                     j < got.size() ? (int)got[j] : 0, (unsigned long long)fed[u]);
                break;
            }
        for (uint64_t j = want; j < got.size(); ++j)
            if (got[j]) {
                fail("%s: segment %llu of unit %d transformed, of %llu complete ones", what, (unsigned long long)j, u, (unsigned long long)want);
                break;
            }
    }
    sim::world() = sim::World();
}

// every route at the call lengths 1, 63 and 8 * 64 + 1, from host and from device memory, units in turn; one device call behind
// a producer event; then, with `big`, for every route one host call of STAGING + 5 samples (two pieces: both staging slots
// and, for the mixer-fronted kinds, the landing buffer are used again) between short calls
void run_family(const Family &fam, Sources &src, bool big)
{
    g_ctx = fam.name;
    void *h = fam.create();
    if (!h) {
        fail("create failed: %s", fam.last_error(nullptr));
        return;
    }
    uint64_t fed[UNITS] = {};
    hipEvent_t producer = nullptr;
    (void)hipEventCreate(&producer);
    bool producer_used = false;
    auto call = [&](Route r, bool dev, uint32_t u, size_t len, void *ev) {
        if (fed[u] + len > (dev ? Sources::DEV : STREAM)) {
            fail("the scenario feeds unit %u past the end of its source", u);
            return;
        }
        const int rc = fam.feed(h, r, dev, u, (size_t)fed[u], len, ev);
        if (rc < 0)
            fail("route %d %s, unit %u, %zu samples at %llu -> %d (%s)", (int)r, dev ? "device" : "host", u, len, (unsigned long long)fed[u], rc,
                 fam.last_error(h));
        else
            fed[u] += len;
    };
    for (int rep = 0; rep < 2; ++rep) // (the second time round the buffers have grown and rounds R - 2 are recorded)
        for (Route r : fam.routes)
            for (int dev = 0; dev < 2; ++dev)
                for (size_t len : {(size_t)1, (size_t)63, (size_t)(8 * 64 + 1)}) {
                    const uint32_t u = (uint32_t)((len + rep) % UNITS);
                    void *ev = nullptr;
                    if (dev && rep == 1 && !producer_used) {
                        (void)hipEventRecord(producer, nullptr);
                        ev = producer;
                        producer_used = true;
                    }
                    call(r, dev != 0, u, len, ev);
                }
    // (the identities of a stream end at 2^24 and the sources at STREAM: every long call gets an object of its own)
    for (size_t i = 0; big && i < fam.routes.size(); ++i) {
        if (fam.sync(h) < 0)
            fail("sync -> %s", fam.last_error(h));
        check_world("before a long call", fed);
        fam.destroy(h);
        if (!(h = fam.create())) {
            fail("create failed: %s", fam.last_error(nullptr));
            return;
        }
        memset(fed, 0, sizeof fed);
        const uint32_t u = (uint32_t)(i % UNITS);
        call(fam.routes[i], false, u, 63, nullptr);
        call(fam.routes[i], true, u, 8 * 64 + 1, nullptr);
        call(fam.routes[i], false, u, STAGING + 5, nullptr);
        call(fam.routes[i], false, u ^ 1, 63, nullptr);
        call(fam.routes[i], true, u ^ 1, 63, nullptr);
        call(fam.routes[i], false, u, 1, nullptr);
    }
    if (fam.sync(h) < 0)
        fail("sync -> %s", fam.last_error(h));
    check_world("at the end", fed);
    fam.destroy(h);
    (void)hipEventDestroy(producer);
}

// frames whose header seq is the absolute batch index (as in round_plan_check.cpp)
std::vector<uint8_t> make_frames(size_t n_frames, int batches, uint32_t seq0)
{
    const size_t fs = 8 + 64 * (size_t)batches;
    std::vector<uint8_t> b(n_frames * fs, 0x5a);
    for (size_t f = 0; f < n_frames; ++f) {
        uint8_t *p = &b[f * fs];
        p[0] = 0x7b, p[1] = 0x05, p[2] = 1, p[3] = (uint8_t)batches;
        const uint32_t s = seq0 + (uint32_t)(f * (size_t)batches);
        p[4] = (uint8_t)s, p[5] = (uint8_t)(s >> 8), p[6] = (uint8_t)(s >> 16), p[7] = (uint8_t)(s >> 24);
    }
    return b;
}

// one host and one device frames call (and a host call again: its staging slot comes round) into both units of an object
template <class H>
void run_frames(const char *name, H *h, const uint32_t *map, int (*host)(H *, const uint32_t *, const uint8_t *, size_t, size_t, size_t *),
                int (*device)(H *, const uint32_t *, const uint8_t *, size_t, size_t, size_t *, void *), int (*sync)(H *), void (*destroy)(H *),
                const char *(*last_error)(const H *))
{
    g_ctx = name;
    if (!h) {
        fail("create failed: %s", last_error(nullptr));
        return;
    }
    const int batches = 5;
    const size_t fs = 8 + 64 * (size_t)batches, per_frame = 8 * (size_t)batches;
    uint64_t fed[UNITS] = {};
    size_t frames_in = 0;
    for (size_t nf : {(size_t)7, (size_t)3, (size_t)16}) {
        const bool dev = nf == 3;
        std::vector<uint8_t> fr = make_frames(nf, batches, (uint32_t)(frames_in * batches));
        uint8_t *d = nullptr;
        if (dev) {
            (void)hipMalloc(&d, fr.size());
            memcpy(d, fr.data(), fr.size());
        }
        size_t ok = 0;
        const int rc = dev ? device(h, map, d, fs, nf, &ok, nullptr) : host(h, map, fr.data(), fs, nf, &ok);
        if (rc < 0 || ok != nf)
            fail("%zu %s frames -> %d, %zu taken (%s)", nf, dev ? "device" : "host", rc, ok, last_error(h));
        if (sync(h) < 0) // (the frames are the caller's until the call's work is done)
            fail("sync -> %s", last_error(h));
        if (d)
            (void)hipFree(d);
        frames_in += nf;
        for (int u = 0; u < UNITS; ++u)
            fed[u] += nf * per_frame;
    }
    check_world("frames", fed);
    destroy(h);
}

} // namespace

int main(int argc, char **argv)
{
    const char *trace_file = nullptr;
    for (int i = 1; i < argc; ++i)
        if (!strcmp(argv[i], "--trace") && i + 1 < argc)
            trace_file = argv[++i];
    std::vector<std::vector<std::string>> trace;
    sim::rt().trace = &trace;
    const auto t0 = std::chrono::steady_clock::now();
    Sources src;
    src.upload();
    auto carriers = [](auto *h, auto set) { // ftw = 100 (u + 1) + side: the models know the unit by it
        for (uint32_t u = 0; h && u < (uint32_t)UNITS; ++u)
            set(h, u, 100 * (u + 1));
        return h;
    };
    auto zoom_carriers = [&](psdc_zoom *h) { return carriers(h, [](psdc_zoom *z, uint32_t u, uint64_t f) { psdc_zoom_set_carrier(z, u, f, 7); }); };
    auto iq_carriers = [&](psdc_iq *h) { return carriers(h, [](psdc_iq *z, uint32_t u, uint64_t f) { psdc_iq_set_carrier(z, u, f, 7); }); };
    auto zcsd_carriers = [&](psdc_zcsd *h) {
        return carriers(h, [](psdc_zcsd *z, uint32_t u, uint64_t f) {
            psdc_zcsd_set_carrier(z, u, 0, f, 7);
            psdc_zcsd_set_carrier(z, u, 1, f + 1, 9);
        });
    };
    auto iqcsd_carriers = [&](psdc_iqcsd *h) {
        return carriers(h, [](psdc_iqcsd *z, uint32_t u, uint64_t f) {
            psdc_iqcsd_set_carrier(z, u, 0, f, 7);
            psdc_iqcsd_set_carrier(z, u, 1, f + 1, 9);
        });
    };
    // the sources of a call: stream u from `off` on, in the memory and the number format of the route
    auto f32 = [&](bool dev, uint32_t u, size_t off) { return (dev ? src.d_f32[u] : src.f32[u].data()) + off; };
    auto z32 = [&](bool dev, uint32_t u, size_t off) { return (dev ? src.d_z32[u] : src.z32[u].data()) + 2 * off; };
    auto s16 = [&](bool dev, uint32_t u, size_t off) { return static_cast<const void *>((dev ? src.d_s16[u] : src.s16[u].data()) + off); };
    // (an sc16 pair is the 32 identity bits: the f32 stream itself)
    auto sc16 = [&](bool dev, uint32_t u, size_t off) { return static_cast<const void *>(f32(dev, u, off)); };

    std::vector<Family> fams;
    fams.push_back(family<psdc_cross>(
        "psdc_cross", {F32}, [] { return psdc_cross_create(N, PSDC_WINDOW_HANN, UNITS, 0); },
        [&](psdc_cross *h, Route, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            return dev ? psdc_cross_process_device(h, u, f32(true, u, off), f32(true, u, off), len, ev)
                       : psdc_cross_process(h, u, f32(false, u, off), f32(false, u, off), len);
        },
        psdc_cross_sync, psdc_cross_destroy, psdc_cross_last_error));
    fams.push_back(family<psdc_csm>(
        "psdc_csm", {F32}, [] { return psdc_csm_create(N, PSDC_WINDOW_HANN, 3, UNITS, 0); },
        [&](psdc_csm *h, Route, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            const float *x[3] = {f32(dev, u, off), f32(dev, u, off), f32(dev, u, off)};
            return dev ? psdc_csm_process_device(h, u, x, len, ev) : psdc_csm_process(h, u, x, len);
        },
        psdc_csm_sync, psdc_csm_destroy, psdc_csm_last_error));
    fams.push_back(family<psdc_sk>(
        "psdc_sk", {F32}, [] { return psdc_sk_create(N, PSDC_WINDOW_HANN, UNITS, 0); },
        [&](psdc_sk *h, Route, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            return dev ? psdc_sk_process_device(h, u, f32(true, u, off), len, ev) : psdc_sk_process(h, u, f32(false, u, off), len);
        },
        psdc_sk_sync, psdc_sk_destroy, psdc_sk_last_error));
    fams.push_back(family<psdc_zoom>(
        "psdc_zoom", {F32, S16}, [&] { return zoom_carriers(psdc_zoom_create(N, PSDC_WINDOW_HANN, UNITS, 0)); },
        [&](psdc_zoom *h, Route r, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            if (r == S16)
                return dev ? psdc_int_zoom_process_device(h, u, s16(true, u, off), PSDC_SAMPLE_S16, 1.0f, len, ev)
                           : psdc_int_zoom_process(h, u, s16(false, u, off), PSDC_SAMPLE_S16, 1.0f, len);
            return dev ? psdc_zoom_process_device(h, u, f32(true, u, off), len, ev) : psdc_zoom_process(h, u, f32(false, u, off), len);
        },
        psdc_zoom_sync, psdc_zoom_destroy, psdc_zoom_last_error));
    fams.push_back(family<psdc_zcsd>(
        "psdc_zcsd", {F32, S16}, [&] { return zcsd_carriers(psdc_zcsd_create(N, PSDC_WINDOW_HANN, UNITS, 0)); },
        [&](psdc_zcsd *h, Route r, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            if (r == S16)
                return dev ? psdc_int_zcsd_process_device(h, u, s16(true, u, off), s16(true, u, off), PSDC_SAMPLE_S16, 1.0f, len, ev)
                           : psdc_int_zcsd_process(h, u, s16(false, u, off), s16(false, u, off), PSDC_SAMPLE_S16, 1.0f, len);
            return dev ? psdc_zcsd_process_device(h, u, f32(true, u, off), f32(true, u, off), len, ev)
                       : psdc_zcsd_process(h, u, f32(false, u, off), f32(false, u, off), len);
        },
        psdc_zcsd_sync, psdc_zcsd_destroy, psdc_zcsd_last_error));
    fams.push_back(family<psdc_iq>(
        "psdc_iq", {F32, F32_Z, S16}, [&] { return iq_carriers(psdc_iq_create(N, PSDC_WINDOW_HANN, UNITS, 0)); },
        [&](psdc_iq *h, Route r, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            if (r == S16)
                return dev ? psdc_int_iq_process_device(h, u, sc16(true, u, off), PSDC_SAMPLE_S16, 1.0f, len, ev)
                           : psdc_int_iq_process(h, u, sc16(false, u, off), PSDC_SAMPLE_S16, 1.0f, len);
            if (r == F32_Z)
                return dev ? psdc_iq_process_interleaved_device(h, u, z32(true, u, off), len, ev)
                           : psdc_iq_process_interleaved(h, u, z32(false, u, off), len);
            return dev ? psdc_iq_process_device(h, u, f32(true, u, off), f32(true, u, off), len, ev)
                       : psdc_iq_process(h, u, f32(false, u, off), f32(false, u, off), len);
        },
        psdc_iq_sync, psdc_iq_destroy, psdc_iq_last_error));
    fams.push_back(family<psdc_iqcsd>(
        "psdc_iqcsd", {F32, F32_Z, S16}, [&] { return iqcsd_carriers(psdc_iqcsd_create(N, PSDC_WINDOW_HANN, UNITS, 0)); },
        [&](psdc_iqcsd *h, Route r, bool dev, uint32_t u, size_t off, size_t len, void *ev) {
            if (r == S16)
                return dev ? psdc_int_iqcsd_process_device(h, u, sc16(true, u, off), sc16(true, u, off), PSDC_SAMPLE_S16, 1.0f, len, ev)
                           : psdc_int_iqcsd_process(h, u, sc16(false, u, off), sc16(false, u, off), PSDC_SAMPLE_S16, 1.0f, len);
            if (r == F32_Z)
                return dev ? psdc_iqcsd_process_interleaved_device(h, u, z32(true, u, off), z32(true, u, off), len, ev)
                           : psdc_iqcsd_process_interleaved(h, u, z32(false, u, off), z32(false, u, off), len);
            const float *x = f32(dev, u, off);
            return dev ? psdc_iqcsd_process_device(h, u, x, x, x, x, len, ev) : psdc_iqcsd_process(h, u, x, x, x, x, len);
        },
        psdc_iqcsd_sync, psdc_iqcsd_destroy, psdc_iqcsd_last_error));
    for (const Family &fam : fams)
        run_family(fam, src, true);

    // frames: channel u of the zoom object takes trace u; pair 0 of the pair object traces (0, 1) and pair 1 traces (1, 0)
    const uint32_t zoom_map[UNITS] = {0, 1}, cross_map[2 * UNITS] = {0, 1, 1, 0};
    run_frames("psdc_zoom frames", zoom_carriers(psdc_zoom_create(N, PSDC_WINDOW_HANN, UNITS, 0)), zoom_map, psdc_zoomcascade_process_frames,
               psdc_zoomcascade_process_frames_device, psdc_zoom_sync, psdc_zoom_destroy, psdc_zoom_last_error);
    run_frames("psdc_cross frames", psdc_cross_create(N, PSDC_WINDOW_HANN, UNITS, 0), cross_map, psdc_csd_process_frames,
               psdc_csd_process_frames_device, psdc_cross_sync, psdc_cross_destroy, psdc_cross_last_error);

    g_ctx = "end";
    src.release();
    if (sim::rt().live_blocks != 0)
        fail("%zu device / pinned allocations alive after every object was destroyed", sim::rt().live_blocks);
    size_t lines = 0;
    for (const auto &g : trace)
        lines += g.size();
    if (trace_file) {
        FILE *f = fopen(trace_file, "w");
        if (!f) {
            fail("cannot write %s", trace_file);
        } else {
            for (size_t g = 0; g < trace.size(); ++g) {
                fprintf(f, g ? "== stream %zu\n" : "== host\n", g - 1);
                for (const std::string &l : trace[g])
                    fprintf(f, "%s\n", l.c_str());
            }
            fclose(f);
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (g_failures) {
        fprintf(stderr, "cross_feed_check: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("cross_feed_check: %zu families and 2 frames objects, %zu trace lines on %zu streams, %.1f s: every segment exactly once from "
           "the samples of its index, nothing left allocated\n",
           fams.size(), lines, trace.size() - 1, secs);
    return 0;
}
