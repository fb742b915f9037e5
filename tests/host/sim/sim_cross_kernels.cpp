// tests/host/sim/sim_cross_kernels.cpp -- TEST INFRASTRUCTURE: models of the launchers of the cross-spectral host runtime
// (stabilizer-stream_amd/csrc/cross_runtime.cpp), for the check programs that link that file unchanged against the host model of
// the HIP runtime: tests/host/cross_feed_check.cpp (the feeds) and tests/host/cross_read_check.cpp (the read-outs).
//
// The launchers of cross.h, csm.h, zoom.h, zoom_cross.h, iq.h, iq_cross.h, sk.h, zoom_sk.h, zoom_ampm.h and sample_int.h are
// modelled here; the decimator is the model of sim_kernels.cpp.  As in sim_device.h the models track IDENTITY: sample j of
// unit u is fed as the bit pattern ident(16 u, j) (an s16 sample as the low 16 bits of j; an sc16 pair holds the 32 bits).  A
// mixer, copy or frames model reads every source byte of its job and writes every destination float, passing its first source
// through; the segment models then require every segment of every stream to hold the samples of its index, so a staging slot
// written too early or a wrong offset into stage 0 shows as a wrong identity, and every segment index must come exactly once.
// A unit's carrier is set to ftw = 100 (u + 1) + side, which the mixer models check (and read the unit from, for s16).
//
// The fold of launch_cross_post gives every accumulator a definite f64 value, so that a read-out returns definite bytes: a hash
// of the fold job's order of arrival (sim::World::fold_jobs), the row and the bin.
//
// Every model writes a line to the trace of its stream (sim::Runtime::trace).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
using sim::bits_of;
using sim::error;
using sim::ident;
using sim::pname;
using sim::put_bits;
using sim::world;

// ---- the launchers -----------------------------------------------------------------------------------------------------------
namespace psdk {

static bool pow2_in(int n, int lo, int hi) { return n >= lo && n <= hi && (n & (n - 1)) == 0; }
bool cross_supported(int n) { return pow2_in(n, 64, 4096); }
bool zoom_cross_supported(int n) { return pow2_in(n, 64, 4096); }
bool csm_supported(int n, int m) { return m >= 2 && m <= CSM_MAX_M && pow2_in(n, 64, m == 4 ? 2048 : 4096); }
int cross_segments_per_tile(int) { return 8; }
int csm_segments_per_tile(int, int) { return 8; }
int zoom_segments_per_tile(int) { return 8; }
int zoom_cross_segments_per_tile(int) { return 8; }
int sk_segments_per_tile(int) { return 8; }
int cross_block_threads(int) { return 256; }
int csm_block_threads(int, int) { return 256; }
int zoom_block_threads(int) { return 256; }
int zoom_cross_block_threads(int) { return 256; }
int cross_fold_blocks(int, int) { return 1; }

static void tr(hipStream_t s, const std::string &line) { sim::trace_line(sim::S(s)->id, line); }
static std::string num(unsigned long long v) { return std::to_string(v); }

// a segment kernel: every segment of every one of the job's nch streams holds the samples of its index, of ONE unit and stage
template <class Batch>
static hipError_t segments(const char *name, int n, int nch, const Batch &b, const float *win, const cf *tw, hipStream_t s)
{
    if (!win || !tw)
        error("%s: null table", name);
    std::string line = std::string(name) + " n " + num(n) + " jobs " + num(b.njobs) + " blocks " + num(b.nblocks) + " hop " + num(b.hop) +
                       " detrend " + num(b.detrend);
    for (int ji = 0; ji < b.njobs; ++ji)
        line += " [" + pname(b.jobs[ji].src[0]) + " base " + num(b.jobs[ji].src_base) + " seg " + num(b.jobs[ji].seg0) + " x " +
                num(b.jobs[ji].nseg) + " blocks " + num(b.jobs[ji].nblocks) + " " + pname(b.jobs[ji].partial) + "]";
    tr(s, line);
    sim::enqueue(s, [=] {
        for (int ji = 0; ji < b.njobs; ++ji) {
            const auto &job = b.jobs[ji];
            const int tag = (int)(bits_of(job.src[0] + (job.seg0 * b.hop - job.src_base)) >> 24);
            for (int la = 0; la < job.nseg; ++la) {
                const long long sidx = job.seg0 + la;
                bool ok = true;
                for (int c = 0; c < nch && ok; ++c) {
                    const float *p = job.src[c] + (sidx * b.hop - job.src_base);
                    for (int j = 0; j < n && ok; ++j)
                        ok = bits_of(p + j) == ident(tag, (uint64_t)sidx * b.hop + j);
                    if (!ok)
                        error("%s job %d: segment %lld of stream %d does not hold samples %lld.. of tag %d", name, ji, sidx, c,
                              sidx * b.hop, tag);
                }
                sim::mark(world().seg, tag, (uint64_t)sidx);
                world().seg_segments += 1;
            }
        }
    });
    return hipSuccess;
}
hipError_t launch_cross(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("cross", n, 2, b, win, tw, s); }
hipError_t launch_csm(int n, int m, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("csm", n, m, b, win, tw, s); }
hipError_t launch_zoom(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("zoom", n, 2, b, win, tw, s); }
hipError_t launch_zoom_cross(int n, const CsmBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("zoom_cross", n, 4, b, win, tw, s); }
hipError_t launch_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("sk", n, 1, b, win, tw, s); }
hipError_t launch_zoom_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("zoom_sk", n, 2, b, win, tw, s); }
hipError_t launch_zoom_ampm(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s) { return segments("zoom_ampm", n, 2, b, win, tw, s); }

// What the fold of job `order` adds to acc[r][k]: 53 mantissa bits of a hash of the three, in [0.5, 1.5), so the value does not
// fit an f32 and a read-out's cast is seen.  Rows 0 and 1 (a unit's "auto" rows in every kind, S1 in the SK kinds) are positive,
// the others take a sign from the hash; row 0 holds exactly 0.0 in every seventh bin from bin 3 on, whatever the job (a bin without
// power: the NaN of the SK read-outs).
static double fold_value(unsigned long long order, int r, int k)
{
    if (r == 0 && k % 7 == 3)
        return 0.0;
    unsigned long long z = (order << 32) + ((unsigned long long)r << 16) + (unsigned long long)k + 0x9E3779B97F4A7C15ull; // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double v = 0.5 + (double)(z >> 11) * (1.0 / 9007199254740992.0);
    return r >= 2 && (z & 1) ? -v : v;
}

// the epilogue: the tails are carried (the next round reads them); a fold adds fold_value to every accumulator of its job, or
// stores it when the job is `fresh`
hipError_t launch_cross_post(const CrossPostBatch &b, hipStream_t s)
{
    std::string line = "post folds " + num(b.nfold) + " rows " + num(b.nrows) + " tails " + num(b.ntail);
    for (int i = 0; i < b.ntail; ++i)
        line += " [" + pname(b.tail[i].dst) + " <- " + pname(b.tail[i].src) + " x " + num(b.tail[i].count) + "]";
    tr(s, line);
    const unsigned long long order0 = (unsigned long long)world().fold_jobs;
    world().fold_jobs += b.nfold;
    sim::enqueue(s, [=] {
        for (int i = 0; i < b.nfold; ++i)
            for (int r = 0; r < b.nrows; ++r)
                for (int k = 0; k < b.nbins; ++k) {
                    double &a = b.fold[i].acc[(size_t)r * b.nbins + k];
                    a = (b.fold[i].fresh ? 0.0 : a) + fold_value(order0 + i, r, k);
                }
        for (int i = 0; i < b.ntail; ++i)
            for (long long k = 0; k < b.tail[i].count; ++k)
                b.tail[i].dst[k] = b.tail[i].src[k];
    });
    return hipSuccess;
}

// the unit a carrier belongs to, and what the mixers check of it
static int unit_of(unsigned long long ftw) { return (int)(ftw / 100) - 1; }
static void check_carrier(const char *name, unsigned long long ftw, uint32_t first, unsigned long long j0)
{
    if (unit_of(ftw) < 0 || unit_of(ftw) > 15 || first != ident(16 * unit_of(ftw), j0))
        error("%s: carrier %llu at stream index %llu, but the source starts with sample %u of tag %u", name, ftw, j0, first & 0xFFFFFFu,
              first >> 24);
}
static void read_all(const void *p, size_t bytes) // (ASan: the bytes exist)
{
    const volatile uint8_t *q = static_cast<const volatile uint8_t *>(p);
    unsigned acc = 0;
    for (size_t i = 0; i < bytes; ++i)
        acc += q[i];
    (void)acc;
}

// zoom_mix_kernel: len floats in, len floats to each of dst_i, dst_q
hipError_t launch_zoom_mix(const ZoomMixJob &j, hipStream_t s)
{
    tr(s, "zoom_mix " + pname(j.x) + " -> " + pname(j.dst_i) + " " + pname(j.dst_q) + " len " + num(j.len) + " j0 " + num(j.j0) + " ftw " +
              num(j.ftw) + " phase " + num(j.phase0));
    sim::enqueue(s, [=] {
        check_carrier("zoom_mix", j.ftw, bits_of(j.x), j.j0);
        for (size_t i = 0; i < j.len; ++i)
            j.dst_i[i] = j.dst_q[i] = j.x[i];
    });
    return hipSuccess;
}
// the integer mixer of a real channel: s16 sample i holds the low 16 bits of its stream index
hipError_t launch_zoom_mix_int(const SintMixJob &j, int kind, hipStream_t s)
{
    tr(s, "zoom_mix_int kind " + num(kind) + " " + pname(j.src) + " -> " + pname(j.dst_i) + " " + pname(j.dst_q) + " len " + num(j.len) + " j0 " +
              num(j.j0) + " ftw " + num(j.ftw) + " phase " + num(j.phase0));
    if (kind != SAMPLE_S16)
        return hipErrorInvalidValue;
    sim::enqueue(s, [=] {
        const int16_t *x = static_cast<const int16_t *>(j.src);
        for (size_t i = 0; i < j.len; ++i) {
            if ((uint16_t)x[i] != (uint16_t)(j.j0 + i)) {
                error("zoom_mix_int: unit %zu of the launch is sample %u, not sample %llu", i, (unsigned)(uint16_t)x[i], j.j0 + i);
                break;
            }
            put_bits(j.dst_i + i, ident(16 * unit_of(j.ftw), j.j0 + i));
            j.dst_q[i] = j.dst_i[i];
        }
    });
    return hipSuccess;
}
// iq_mix_kernel: planar reads both streams, interleaved reads 2 len floats at src_i
hipError_t launch_iq_mix(const IqMixJob &j, bool interleaved, hipStream_t s)
{
    tr(s, std::string("iq_mix ") + (interleaved ? "interleaved " : "planar ") + pname(j.src_i) + " " + pname(j.src_q) + " -> " + pname(j.dst_i) +
              " " + pname(j.dst_q) + " len " + num(j.len) + " j0 " + num(j.j0) + " ftw " + num(j.ftw) + " phase " + num(j.phase0));
    sim::enqueue(s, [=] {
        check_carrier("iq_mix", j.ftw, bits_of(j.src_i), j.j0);
        if (!interleaved)
            read_all(j.src_q, sizeof(float) * j.len);
        for (size_t i = 0; i < j.len; ++i) {
            if (interleaved)
                read_all(j.src_i + 2 * i + 1, sizeof(float));
            j.dst_i[i] = j.dst_q[i] = j.src_i[interleaved ? 2 * i : i];
        }
    });
    return hipSuccess;
}
// the integer mixer of a complex channel: an sc16 unit holds the 32 identity bits
hipError_t launch_iq_mix_int(const SintMixJob &j, int kind, hipStream_t s)
{
    tr(s, "iq_mix_int kind " + num(kind) + " " + pname(j.src) + " -> " + pname(j.dst_i) + " " + pname(j.dst_q) + " len " + num(j.len) + " j0 " +
              num(j.j0) + " ftw " + num(j.ftw) + " phase " + num(j.phase0));
    if (kind != SAMPLE_S16)
        return hipErrorInvalidValue;
    sim::enqueue(s, [=] {
        const float *z = static_cast<const float *>(j.src);
        check_carrier("iq_mix_int", j.ftw, bits_of(z), j.j0);
        for (size_t i = 0; i < j.len; ++i)
            j.dst_i[i] = j.dst_q[i] = z[i];
    });
    return hipSuccess;
}
// iq_pair_mix_kernel: planar reads four streams, interleaved the pairs at src[0] and src[2]
hipError_t launch_iq_pair_mix(const IqPairMixJob &j, bool interleaved, hipStream_t s)
{
    std::string line = std::string("iq_pair_mix ") + (interleaved ? "interleaved" : "planar");
    for (int c = 0; c < 4; ++c)
        line += " " + pname(j.src[c]);
    line += " ->";
    for (int c = 0; c < 4; ++c)
        line += " " + pname(j.dst[c]);
    tr(s, line + " len " + num(j.len) + " j0 " + num(j.j0) + " ftw " + num(j.ftw[0]) + " " + num(j.ftw[1]) + " phase " + num(j.phase0[0]) + " " +
              num(j.phase0[1]));
    sim::enqueue(s, [=] {
        check_carrier("iq_pair_mix", j.ftw[0], bits_of(j.src[0]), j.j0);
        if (j.ftw[1] != j.ftw[0] + 1)
            error("iq_pair_mix: carriers %llu and %llu are not the two sides of one pair", j.ftw[0], j.ftw[1]);
        for (int c = 0; c < 4; c += interleaved ? 2 : 1)
            read_all(j.src[c], sizeof(float) * (interleaved ? 2 : 1) * j.len);
        for (size_t i = 0; i < j.len; ++i)
            j.dst[0][i] = j.dst[1][i] = j.dst[2][i] = j.dst[3][i] = j.src[0][interleaved ? 2 * i : i];
    });
    return hipSuccess;
}
hipError_t launch_iq_pair_mix_int(const SintPairMixJob &j, int kind, hipStream_t s)
{
    std::string line = "iq_pair_mix_int kind " + num(kind) + " " + pname(j.src[0]) + " " + pname(j.src[1]) + " ->";
    for (int c = 0; c < 4; ++c)
        line += " " + pname(j.dst[c]);
    tr(s, line + " len " + num(j.len) + " j0 " + num(j.j0) + " ftw " + num(j.ftw[0]) + " " + num(j.ftw[1]) + " phase " + num(j.phase0[0]) + " " +
              num(j.phase0[1]));
    if (kind != SAMPLE_S16)
        return hipErrorInvalidValue;
    sim::enqueue(s, [=] {
        const float *z = static_cast<const float *>(j.src[0]);
        check_carrier("iq_pair_mix_int", j.ftw[0], bits_of(z), j.j0);
        read_all(j.src[1], sizeof(float) * j.len);
        for (size_t i = 0; i < j.len; ++i)
            j.dst[0][i] = j.dst[1][i] = j.dst[2][i] = j.dst[3][i] = z[i];
    });
    return hipSuccess;
}

// AdcDac frames as make_frames() builds them: the header's seq is the absolute batch index of the frame's first batch, so sample
// (seq + batch) * 8 + i of trace t is known from the header.  Every trace of `traces` is read; the first gives the identity.
template <class Batch>
static void decode(const char *name, const Batch &b, const int *traces, int ntr, float *const *dst, int ndst, unsigned long long j0, bool j0_known)
{
    if (b.fmt != 1)
        error("%s: format %d (the check feeds AdcDac frames)", name, b.fmt);
    for (size_t f = 0; f < b.n_frames; ++f) {
        const uint8_t *h = b.frames + f * b.frame_size;
        const uint32_t seq = (uint32_t)h[4] | ((uint32_t)h[5] << 8) | ((uint32_t)h[6] << 16) | ((uint32_t)h[7] << 24);
        for (int bt = 0; bt < b.batches; ++bt) {
            for (int t = 0; t < ntr; ++t)
                read_all(h + 8 + 64 * (size_t)bt + 16 * (size_t)traces[t], 16);
            for (int i = 0; i < 8; ++i) {
                const size_t si = (f * (size_t)b.batches + (size_t)bt) * 8 + i;
                const uint64_t idx = ((uint64_t)seq + bt) * 8 + i;
                if (si == 0 && j0_known && j0 != idx)
                    error("%s: the launch starts at stream index %llu with sample %llu", name, j0, (unsigned long long)idx);
                for (int d = 0; d < ndst; ++d)
                    put_bits(dst[d] + si, ident(16 * traces[0], idx));
            }
        }
    }
}
template <class Batch>
static std::string frames_text(const char *name, const Batch &b, int units)
{
    return std::string(name) + " " + pname(b.frames) + " frames " + num(b.n_frames) + " of " + num(b.frame_size) + " batches " + num(b.batches) +
           " fmt " + num(b.fmt) + " units " + num(units);
}
hipError_t launch_cross_frames(const CrossFramesBatch &b, hipStream_t s)
{
    std::string line = frames_text("cross_frames", b, b.ndst);
    for (int k = 0; k < b.ndst; ++k)
        line += " [" + num(b.trace[k]) + " -> " + pname(b.dst[k]) + "]";
    tr(s, line);
    // (the check feeds pairs: destinations 2 k and 2 k + 1 are one unit, whose first trace names it)
    sim::enqueue(s, [=] {
        for (int k = 0; k + 1 < b.ndst; k += 2)
            decode("cross_frames", b, &b.trace[k], 2, &b.dst[k], 2, 0, false);
    });
    return hipSuccess;
}
hipError_t launch_zoom_frames(const ZoomFramesBatch &b, hipStream_t s)
{
    std::string line = frames_text("zoom_frames", b, b.nch);
    for (int k = 0; k < b.nch; ++k)
        line += " [" + num(b.trace[k]) + " -> " + pname(b.dst_i[k]) + " " + pname(b.dst_q[k]) + " j0 " + num(b.j0[k]) + " ftw " + num(b.ftw[k]) + "]";
    tr(s, line);
    sim::enqueue(s, [=] {
        for (int k = 0; k < b.nch; ++k) {
            float *dst[2] = {b.dst_i[k], b.dst_q[k]};
            if (unit_of(b.ftw[k]) != b.trace[k])
                error("zoom_frames: carrier %llu with trace %d", b.ftw[k], b.trace[k]);
            decode("zoom_frames", b, &b.trace[k], 1, dst, 2, b.j0[k], true);
        }
    });
    return hipSuccess;
}
hipError_t launch_iq_frames(const IqFramesBatch &b, hipStream_t s)
{
    std::string line = frames_text("iq_frames", b, b.nch);
    for (int k = 0; k < b.nch; ++k)
        line += " [" + num(b.trace_i[k]) + " " + num(b.trace_q[k]) + " -> " + pname(b.dst_i[k]) + " " + pname(b.dst_q[k]) + " j0 " + num(b.j0[k]) + "]";
    tr(s, line);
    sim::enqueue(s, [=] {
        for (int k = 0; k < b.nch; ++k) {
            float *dst[2] = {b.dst_i[k], b.dst_q[k]};
            const int traces[2] = {b.trace_i[k], b.trace_q[k]};
            decode("iq_frames", b, traces, 2, dst, 2, b.j0[k], true);
        }
    });
    return hipSuccess;
}
template <class Batch>
static hipError_t pair_frames(const char *name, int ntr, const Batch &b, hipStream_t s)
{
    std::string line = frames_text(name, b, b.npairs);
    for (int k = 0; k < b.npairs; ++k) {
        line += " [";
        for (int t = 0; t < ntr; ++t)
            line += num(b.trace[k][t]) + " ";
        line += "->";
        for (int c = 0; c < 4; ++c)
            line += " " + pname(b.dst[k][c]);
        line += " j0 " + num(b.j0[k]) + "]";
    }
    tr(s, line);
    sim::enqueue(s, [=] {
        for (int k = 0; k < b.npairs; ++k)
            decode(name, b, b.trace[k], ntr, b.dst[k], 4, b.j0[k], true);
    });
    return hipSuccess;
}
hipError_t launch_zoom_cross_frames(const ZoomCrossFramesBatch &b, hipStream_t s) { return pair_frames("zoom_cross_frames", 2, b, s); }
hipError_t launch_iq_cross_frames(const IqCrossFramesBatch &b, hipStream_t s) { return pair_frames("iq_cross_frames", 4, b, s); }

} // namespace psdk
