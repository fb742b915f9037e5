// tests/host/fused_walk_check.cpp -- the walks of tests/fused_instances.py through the library's host runtime (csrc/runtime.cpp,
// planner.cpp, frames_ingest.cpp, readout.cpp, UNCHANGED) on the CPU model of tests/host/sim/, as round_plan_check.cpp runs the
// fuzz feeds: every kernel job must read exactly the samples it is meant to read from memory that exists, and at the end every
// segment and every decimator output of every stage was produced exactly once.  The planner prints its PSDC_DBG_PLAN lines to
// stderr; tests/test_fused_instances_host.py parses them as tests/test_gpu_fused_instances.py parses those of the GPU run.
// TEST INFRASTRUCTURE.
//
// usage: fused_walk_check --instances       the (family, size, teams) the launch switch and the geometry headers compile
//        fused_walk_check < script          lines: case <id> <n> <rect 0|1> <channels> <detrend> <limit> <count> [NAME=VALUE ...]
//                                                  f32 <samples> <misaligned 0|1> | frames <frames> <continues 0|1> <batches> | check | end
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/psdcascade.h"
#include "fft_block.h"
#include "fft_block3.h"
#include "fft_team.h"
#include "hbf_taps.h"
#include "kernels.h"
#include "plan.h"
#include <hip/hip_runtime.h> // tests/host/sim/hip/hip_runtime.h

#include "sim_device.h"

using namespace psdk;
using sim::ident;
using sim::world;

namespace {

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
        fprintf(stdout, "FAIL [%s] %s\n", g_ctx.c_str(), buf);
    ++g_failures;
}

template <int N>
void team_line()
{
    printf("%s %d teams %d\n", fused_family_name(fused_family(N, true)), N, FUSED_WAVES * TeamFft<N>::TPW);
}
template <int N>
void big3_line()
{
    static_assert(BlockFft3<N>::TEAM == N / 16, "one team of N / 16 threads a workgroup");
    printf("%s %d teams 1\n", fused_family_name(fused_family(N, true)), N);
}
template <int N>
void big_line()
{
    static_assert(BlockFft<N>::TEAM == N / 16, "one team of N / 16 lanes a workgroup");
    printf("%s %d teams 1\n", fused_family_name(fused_family(N, N == 2048 || N == 4096 ? false : true)), N);
}

// what launch_fused can reach: the sizes each family's transform is defined for (instantiating another size does not compile:
// TeamFft / BlockFft3 / BlockFft static_assert theirs), named by the launch switch's own family function; and every other size
// from 2 to 2^17, with and without the seeds, must have no family
int print_instances()
{
    team_line<256>();
    team_line<512>();
    team_line<1024>();
    big3_line<2048>();
    big3_line<4096>();
    big_line<2048>();
    big_line<4096>();
    big_line<8192>();
    big_line<16384>();
    for (int n = 2; n <= (1 << 17); ++n)
        for (int seeds = 0; seeds < 2; ++seeds) {
            const bool known = n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096 || n == 8192 || n == 16384;
            if ((fused_family(n, seeds != 0) != FUSED_FAMILY_NONE) != known) {
                printf("FAIL fused_family(%d, %d)\n", n, seeds);
                return 1;
            }
        }
    printf("forms pair frames single1 single2\n");
    return 0;
}

struct Case {
    psdc_handle *h = nullptr;
    uint32_t n = 0, overlap = 0;
    int nch = 1;
    bool plain = true;
    uint64_t taken = 0;
    std::vector<std::unique_ptr<std::vector<float>>> f32s;    // caller memory stays until the case ends
    std::vector<std::unique_ptr<std::vector<uint8_t>>> frames;
    const uint8_t *frames_end = nullptr;
};

// header seq = absolute batch index: the model identifies frame samples from it
void fill_frames(uint8_t *b, size_t n_frames, int batches, uint32_t seq0)
{
    const size_t fs = 8 + 64 * (size_t)batches;
    memset(b, 0x5a, n_frames * fs);
    for (size_t f = 0; f < n_frames; ++f) {
        uint8_t *p = b + f * fs;
        p[0] = 0x7b, p[1] = 0x05, p[2] = 1, p[3] = (uint8_t)batches;
        const uint32_t s = seq0 + (uint32_t)(f * (size_t)batches);
        p[4] = (uint8_t)s, p[5] = (uint8_t)(s >> 8), p[6] = (uint8_t)(s >> 16), p[7] = (uint8_t)(s >> 24);
    }
}

void verify(Case &c)
{
    Geometry g;
    g.n = c.n, g.overlap = c.overlap, g.hop = c.n - c.overlap, g.drain = (uint32_t)HBF_DRAIN;
    sim::drain();
    for (const std::string &e : world().errors)
        fail("model: %s", e.c_str());
    for (int ch = 0; ch < c.nch; ++ch) {
        uint64_t total = c.taken;
        const int ns = psdc_num_stages(c.h, (uint32_t)ch);
        int k = 0;
        for (; total > 0 && k < 16; ++k) {
            const int tag = ch * 16 + k;
            const uint64_t J = segments_for(g, total), P = decimated_prefix(g, J);
            if (k >= ns) {
                fail("channel %d: stage %d holds %llu samples but the handle has %d stages", ch, k, (unsigned long long)total, ns);
                break;
            }
            const std::vector<uint8_t> &sv = world().seg[tag], &dv = world().dec[tag];
            for (uint64_t s = 0; s < std::max<uint64_t>(J, sv.size()); ++s)
                if ((s < sv.size() ? sv[s] : 0) != (s < J ? 1 : 0)) {
                    fail("channel %d stage %d: segment %llu transformed %d times (of %llu)", ch, k, (unsigned long long)s,
                         s < sv.size() ? sv[s] : 0, (unsigned long long)J);
                    break;
                }
            for (uint64_t m = 0; m < std::max<uint64_t>(P / 8, dv.size()); ++m) {
                const int got = m < dv.size() ? dv[m] : 0, want = m < P / 8 ? 1 : 0;
                if (got != want && !(m < (uint64_t)HBF_DRAIN && got == 0)) { // (the drained outputs may never be computed)
                    fail("channel %d stage %d: decimator output %llu produced %d times (of %llu)", ch, k, (unsigned long long)m, got,
                         (unsigned long long)(P / 8));
                    break;
                }
            }
            psdc_stage_stat st{};
            if (psdc_stage_info(c.h, (uint32_t)ch, (uint32_t)k, &st) < 0)
                fail("psdc_stage_info: %s", psdc_last_error(c.h));
            if (st.pending != pending_for(g, total) || (c.plain && st.count != J))
                fail("channel %d stage %d: pending %llu count %u, closed form %llu / %llu", ch, k, (unsigned long long)st.pending, st.count,
                     (unsigned long long)pending_for(g, total), (unsigned long long)J);
            total = emitted_for(g, P);
        }
        if (k != ns && !(k < ns && total == 0))
            fail("channel %d: %d stages expected, the handle has %d", ch, k, ns);
    }
}

int run_script()
{
    Case c;
    char line[1024];
    auto end_case = [&] {
        if (!c.h)
            return;
        verify(c);
        psdc_destroy(c.h);
        c = Case{};
    };
    while (fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "case") {
            end_case();
            std::string id, kv;
            int rect = 0, detrend = 0;
            unsigned long long limit = 0, count = 0;
            in >> id >> c.n >> rect >> c.nch >> detrend >> limit >> count;
            g_ctx = id;
            sim::drain();
            world() = sim::World{};
            std::vector<std::string> names;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                names.push_back(kv.substr(0, eq));
                setenv(names.back().c_str(), kv.substr(eq + 1).c_str(), 1);
            }
            fprintf(stderr, "case %s\n", id.c_str());
            c.h = psdc_create(c.n, rect ? PSDC_WINDOW_RECTANGULAR : PSDC_WINDOW_HANN, (uint32_t)c.nch, 0);
            for (const std::string &nm : names)
                unsetenv(nm.c_str());
            if (!c.h) {
                fail("psdc_create: %s", psdc_last_error(nullptr));
                return 1;
            }
            c.overlap = rect ? 0 : c.n / 2;
            c.plain = limit == 0xFFFFFFFFull && count == 0xFFFFFFFFull;
            int rc = psdc_configure(c.h, PSDC_OPT_MIN_PAIRS, 1);
            rc = rc < 0 ? rc : psdc_configure(c.h, PSDC_OPT_COALESCE, 2);
            rc = rc < 0 ? rc : psdc_set_detrend(c.h, detrend);
            if (rc >= 0 && !c.plain)
                rc = psdc_set_avg(c.h, (uint32_t)limit, (uint32_t)count);
            if (rc < 0)
                fail("settings: %s", psdc_last_error(c.h));
        } else if (op == "f32") {
            size_t len = 0;
            int mis = 0;
            in >> len >> mis;
            // sample i of the stream at an address that is 16-byte aligned where i is a multiple of 4 (+ one element when misaligned)
            c.f32s.emplace_back(new std::vector<float>(len + 12));
            float *p = c.f32s.back()->data();
            p += ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4 + (c.taken & 3) + (size_t)mis;
            for (size_t i = 0; i < len; ++i)
                sim::put_bits(p + i, ident(0, c.taken + i));
            if (psdc_process_device(c.h, 0, p, len) < 0)
                fail("psdc_process_device: %s", psdc_last_error(c.h));
            c.taken += len;
        } else if (op == "frames") {
            size_t nf = 0;
            int cont = 0, batches = 0;
            in >> nf >> cont >> batches;
            const size_t fs = 8 + 64 * (size_t)batches;
            uint8_t *base = nullptr;
            if (cont) { // the caller reserved room behind the call before (below)
                base = const_cast<uint8_t *>(c.frames_end);
            } else {
                c.frames.emplace_back(new std::vector<uint8_t>((nf + 4096) * fs + 16));
                base = c.frames.back()->data();
                base += (8 - (reinterpret_cast<uintptr_t>(base) & 7)) & 7;
            }
            if (cont && nf > 4096)
                fail("a continuing call of %zu frames", nf);
            fill_frames(base, nf, batches, (uint32_t)(c.taken / 8));
            size_t ok = 0;
            if (psdc_process_adcdac_frames_device(c.h, base, fs, nf, &ok) < 0 || ok != nf)
                fail("psdc_process_adcdac_frames_device: %zu of %zu frames (%s)", ok, nf, psdc_last_error(c.h));
            c.frames_end = base + nf * fs;
            c.taken += nf * 8 * (size_t)batches;
        } else if (op == "check") {
            for (int ch = 0; ch < c.nch; ++ch)
                if (psdc_num_stages(c.h, (uint32_t)ch) < 0)
                    fail("psdc_num_stages: %s", psdc_last_error(c.h));
        } else if (op == "end") {
            end_case();
        }
    }
    end_case();
    sim::drain();
    world() = sim::World{};
    if (sim::rt().live_blocks != 0)
        fail("%zu device / pinned allocations were never freed", sim::rt().live_blocks);
    printf("fused_walk_check: %s\n", g_failures ? "FAILED" : "every segment and every decimator output exactly once, every read inside its source");
    return g_failures ? 1 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--instances"))
        return print_instances();
    return run_script();
}
