// cross_runtime.cpp -- the cross-spectral cascades behind psdc_cross_* / psdc_csd_* (pairs), psdc_csm_* (groups of m = 2 ... 4
// channels with their full spectral matrix), psdc_zoom_* (channels mixed down from a carrier) and psdc_zcsd_* (pairs of channels
// mixed down from a carrier each, with their cross spectrum) of include/psdcascade.h.  One
// runtime over the channel count: a pair object is m = 2 on cross_kernel with the rows xx, yy, re, im; a matrix object runs
// csm_kernel<N, M> with m * m rows (csm_fft.h); a zoom object's unit is one real channel whose m = 2 streams are the I and Q the
// mixer (zoom_mix_kernel, in place of the input copy) makes of it, on zoom_kernel with the rows upper, lower; a zoom cross
// object's unit is two such channels, m = 4 streams (I_a, Q_a, I_b, Q_b), on zoom_cross_kernel with the eight rows of
// zoom_cross_fft.h; an IQ object (psdc_iq_*) is the zoom kind with a different feed: its unit is one COMPLEX channel whose I and Q
// arrive from the caller and go through the complex mixer (iq_mix_kernel, iq_frames_kernel) into the same two streams; an IQ cross
// object (psdc_iqcsd_*) is the zoom cross kind with that feed for both sides at once: its unit is two complex channels, turned by
// one pair mixer (iq_pair_mix_kernel, iq_cross_frames_kernel) into the same four streams; a spectral kurtosis object (psdc_sk_*)
// has one real channel a unit, m = 1 stream fed as a pair's are, on sk_kernel with the rows S1 = sum w P and S2 = sum w P^2 of
// sk_fft.h; a zoom / IQ spectral kurtosis object (psdc_zsk_*, psdc_iqsk_*) is the zoom / IQ kind on zoom_sk_kernel, with the four
// rows of zoom_sk_fft.h; an AM/PM object (psdc_zampm_*, psdc_iqampm_*) is the zoom / IQ kind on zoom_ampm_kernel, with the four rows
// of zoom_ampm_fft.h.  Below, "pair" stands for any of these units.
//
// `n_pairs` independent pairs of streams (x, y) on one MI355X.  Per pair the stages follow PsdCascade<N>
// (src/psd.rs:399-544) fed x: same segmentation, window, detrend, /8 decimation of each channel and lazy stages.  Per stage
// three accumulators (xx, yy, and the complex xy = sum conj(X) Y as re / im rows) in f64 on the device.
//
// A round plans every (pair, stage) at once from the host-side stream positions (plan.h):
//   1. cross_kernel   the new complete segments of every (pair, stage): partial rows per workgroup
//   2. hbf_dec8       the /8 decimator of each channel into the next stage's stream (kernels.hip, unchanged)
//   3. cross_post     fold the partials into the accumulators, carry the stream tails into the other buffer
// Stage k + 1 consumes what stage k produced in earlier rounds, so a round is three launches whatever the depth and the pair
// count (more only when a round's job tables overflow a launch).  Read-outs drain: rounds until no stage has work.
// There is no CPU compute path.
//
// The host read-outs of a unit share one path ("the host read-outs of a unit", below): a stage read-out looks its stage up in one
// place (drained_stage) and copies its rows through one copier (stage_rows); a stitched read-out takes ONE snapshot of the drained
// unit (UnitSnap: counts, averages, pendings and, one copy a stage, the f64 accumulators), stitches the f32 cast of its leading
// rows and writes len, n_breaks and the Breaks in one place (unit_stitch); what a family computes in f64 from the bins that stitch
// took (SK, the sidebands) is an expression on one walk over them (Stitched::each_bin).
#include "csm.h"
#include "zoom_cross.h"
#include "iq.h"
#include "iq_cross.h"
#include "sample_int.h"
#include "sk.h"
#include "sk_fft.h"
#include "zoom_sk.h"
#include "zoom_sk_fft.h"
#include "zoom_ampm.h"
#include "zoom_ampm_fft.h"
#include "zoom_ampm_cross_fft.h"
#include "waterfall.h"
#include "waterfall_plan.h"
#include "waterfall_read.h"
#include "waterfall_robust.h"
#include "cross_readout.h"
#include "carrier_readout.h"
#include "pair_readout.h"
#include "host_runtime.h"
#include "../../include/psdcascade_robust.h"
#include "../../include/psdcascade_crossread.h"
#include "../../include/psdcascade_carrierread.h"
#include "../../include/ext/psdcascade_pairread.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

using namespace psdk;

#if !defined(__HIPCC__)
// A host build of this file (tests/host/cross_feed_check and cross_read_check: the HIP runtime modelled on the CPU, no device code) sees none of the
// launchers of sample_int.h, which declares them for hipcc alone.  The integer mixers are the check program's models; there is
// no converter, as in a host build of runtime.cpp: the integer feeds of the pair and matrix objects fail there with a device error.
namespace psdk {
hipError_t launch_zoom_mix_int(const SintMixJob &j, int kind, hipStream_t s);
hipError_t launch_iq_mix_int(const SintMixJob &j, int kind, hipStream_t s);
hipError_t launch_iq_pair_mix_int(const SintPairMixJob &j, int kind, hipStream_t s);
inline hipError_t launch_cvt_int(const SintCvtJob &, int, hipStream_t) { return hipErrorInvalidValue; }
// (nor a waterfall read-out kernel: psdc_wf_image[_device] fail there with a device error)
inline hipError_t launch_wf_image(const WfImageJob &, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_wf_robust(const WfRobustJob &, hipStream_t) { return hipErrorInvalidValue; } // (psdcx_*_robust[_device] too)
// (nor the bank read-out kernels of cross_readout.hip: the psdcxr_ read-outs fail there with a device error once a stage is included)
inline hipError_t launch_cross_stitch_pair(const CrossReadJob *, uint32_t, uint32_t, const CrossPairOut &, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_cross_stitch_rows(const CrossReadJob *, uint32_t, uint32_t, float *, float *, size_t, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_cross_band(const CrossReadJob *, const BankRow *, uint32_t, const BankBands &, double *, hipStream_t) { return hipErrorInvalidValue; }
// (nor those of carrier_readout.hip: the psdczr_ read-outs fail there in the same way)
inline hipError_t launch_carrier_stitch(int, const CarrierReadJob *, uint32_t, uint32_t, const CarrierOut &, const CarrierUnit *, uint32_t, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_carrier_band(uint32_t, const CarrierReadJob *, const BankRow *, const CarrierUnit *, uint32_t, const BankBands &, double *, hipStream_t) { return hipErrorInvalidValue; }
// (nor those of pair_readout.hip: the psdcpr_ read-outs fail there in the same way)
inline hipError_t launch_pair_stitch_csd(const CarrierReadJob *, uint32_t, uint32_t, const PairCsdOut &, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_pair_stitch_ampm(const CarrierReadJob *, uint32_t, uint32_t, const PairAmPmOut &, const PairUnit *, uint32_t, hipStream_t) { return hipErrorInvalidValue; }
inline hipError_t launch_pair_band(int, const CarrierReadJob *, const BankRow *, const PairUnit *, uint32_t, const BankBands &, double *, hipStream_t) { return hipErrorInvalidValue; }
} // namespace psdk
#endif

namespace {

constexpr uint32_t X_MAX_STAGES = 16;
constexpr uint32_t X_MAX_PAIRS = 65536;
constexpr size_t STAGING = (size_t)1 << 22; // host-fed samples a channel per pinned staging slot
constexpr size_t PIECE_SAMPLES = (size_t)1 << 22;            // a frames call is cut into pieces of <= this many samples a trace

thread_local std::string x_last_error;

struct XBuf {
    float *p[CSM_MAX_M][2] = {}; // [channel][ping-pong]
    int cur = 0;
    size_t cap = 0;    // floats per buffer
    uint64_t base = 0; // absolute stream index of p[c][cur][0] (both channels)
};

struct XStage {
    uint64_t total = 0; // samples received (each channel)
    uint64_t segs = 0;  // segments issued
    uint64_t dec = 0;   // samples handed to the decimator
    uint64_t count64 = 0;
    XBuf buf;
    double *acc = nullptr; // device [rows][n/2 + 1]: xx, yy, re xy, im xy of a pair; the m * m rows of csm_fft.h of a group
                           // (a waterfall kind: the stage's ring, [wf_depth] such row sets)
};

struct XObj;

// What tells the fifteen families apart, one row each in KINDS (below XObj): the names in error texts, the streams and rows of a
// unit, the feed in front of stage 0 and the segment kernel.  Everything else in this file is one runtime over these.
enum class Feed {
    PLAIN, // the m streams are the caller's, copied (or converted) into stage 0
    ZOOM,  // a real channel a two streams: the mixer makes I and Q of it
    IQ,    // a complex channel a two streams: the caller's I and Q through the complex mixer
};
struct KindDesc {
    const char *tag, *unit, *units;
    uint32_t m;    // streams of a unit (0: the caller's, psdc_csm)
    uint32_t rows; // accumulator rows of a stage (0: m * m)
    Feed feed;
    int (*segments_per_tile)(int n, int m);
    // the segment kernel: on CrossBatch jobs (two streams at most) or, for the kinds with up to four, on CsmBatch jobs
    hipError_t (*launch_pair)(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);
    hipError_t (*launch_group)(const XObj &h, CsmBatch &b); // (the kind may mark the batch for its launcher: CsmBatch::variant)
    std::string (*refusal)(uint32_t n, uint32_t m); // why the kind has no kernel for these sizes ("": it has), NULL: for every n
};

struct XObj {
    const KindDesc *kind = nullptr;
    uint32_t n = 0, n_pairs = 0;
    uint32_t m = 2; // streams of a pair / group
    bool mixed() const { return kind->feed != Feed::PLAIN; } // the streams are I and Q of mixed channels, two a channel
    uint32_t rows() const { return kind->rows ? kind->rows : m * m; }
    uint32_t reals() const { return mixed() ? m / 2 : m; } // channels a unit has (a mixed channel is two of the m streams)
    // f32 streams of STAGING samples a pinned staging slot and the landing buffer hold, which is also the entries a unit has in a
    // frames call's map: a zoom channel takes one, a zoom cross pair one for each side, an IQ unit its I and Q streams, else m
    uint32_t lanes() const { return kind->feed == Feed::ZOOM ? m / 2 : m; }
    uint32_t map_w() const { return lanes(); }
    // host-memory frame bytes a pinned staging slot takes at once, and the size of d_frames: a zoom object's slot holds one
    // channel's STAGING floats (16 MB), a zoom cross object's two (32 MB), an IQ cross object's four (64 MB), the others' at least two
    size_t frames_chunk() const { return sizeof(float) * STAGING * (mixed() ? lanes() : 2); }
    int device = 0;
    Geometry geo;
    float power = 0.25f, nenbw = 1.5f;
    int detrend = PSDC_DETREND_NONE;
    uint32_t avg_limit = 0xFFFFFFFFu, avg_count = 0xFFFFFFFFu;
    // waterfall kinds (include/psdcascade.h, "waterfall cascades"): segments a block and ring slots a stage; 0: not a waterfall
    uint32_t wf_block = 0, wf_depth = 0;
    size_t acc_sets() const { return wf_block ? wf_depth : 1; } // row sets a stage's `acc` holds
    hipStream_t stream = nullptr;
    // Device-fed samples are copied into stage 0 on a stream of their own, beside the kernels of the round before: the copy of
    // the samples of round R writes stage-0 buffer regions that only rounds <= R - 2 read (the round before has carried its
    // tail to the front of the buffer the copy appends to, or left the region behind its stream end alone), so it waits for
    // round R - 2 (ev_round[R & 1]) and the round waits for it (ev_copy).  A buffer that grows is copied on the compute stream
    // first (ev_grow).
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_round[2] = {nullptr, nullptr}, ev_copy = nullptr, ev_grow = nullptr;
    bool round_recorded[2] = {false, false};
    uint64_t rounds = 0; // rounds enqueued
    bool grew = false;   // ensure_room replaced a buffer since the flag was cleared
    float *d_win = nullptr;
    cf *d_tw = nullptr;
    std::vector<std::vector<XStage>> pairs;
    float *d_partial = nullptr;
    size_t partial_cap = 0;
    float *h_stage[2] = {nullptr, nullptr}; // pinned staging: [m channels][STAGING] each
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    bool ev_pending[2] = {false, false};
    int stage_cur = 0;
    std::vector<void *> retired; // replaced device buffers, freed at the next sync point
    bool idle = true;            // every stage drained
    uint64_t launches = 0, pairs_in = 0;
    // frames (psdc_csd_ / psdc_csm_ / psdc_zoomcascade_ / psdc_zoomcsdcascade_process_frames[_device]): Loss over every frame either call ingested; host-memory
    // frames go up through h_stage into d_frames (frames_chunk() bytes, made by the first host-frames call); device frames' headers
    // come to the host through `hdr`
    psdc_loss loss{};
    uint8_t *d_frames = nullptr;
    psdrt::HeaderGather hdr;
    // zoom: a channel's carrier (2^-64 turn a sample, start phase; channel `side` of unit u at reals() u + side) and the device
    // buffer host samples land in before the mixer (reals() x STAGING floats)
    std::vector<uint64_t> ftw, phase0;
    float *d_land = nullptr;
    int64_t resident = 1024; // cross_kernel workgroups a launch is dealt to (twice what the device holds at once)
    // the bank read-outs' job-table slots and host-form buffers (psdcxr_*, include/psdcascade_crossread.h), made by their first call;
    // destroy_impl frees them with the object
    psdrt::BankRead *bank_read = nullptr;
    std::string err;
};

} // namespace

struct psdc_cross : XObj {};
struct psdc_csm : XObj {};
struct psdc_zoom : XObj {};
struct psdc_zcsd : XObj {};
struct psdc_iq : XObj {};
struct psdc_iqcsd : XObj {};
struct psdc_sk : XObj {};
struct psdc_zsk : XObj {};
struct psdc_iqsk : XObj {};
struct psdc_zampm : XObj {};
struct psdc_iqampm : XObj {};
struct psdc_zxampm : XObj {};
struct psdc_iqxampm : XObj {};

namespace {

static_assert(CSM_MAX_JOBS == CROSS_MAX_JOBS, "one job table length for both segment kernels");

int xfail(XObj *h, int code, const std::string &msg)
{
    if (h)
        h->err = msg;
    x_last_error = msg;
    return code;
}

#define XCHK(h, expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            return xfail(h, PSDC_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

#define X_ON_DEVICE(h)                                                                                                 \
    psdrt::DevScope dev_scope_((h)->device);                                                                           \
    if (dev_scope_.err != hipSuccess)                                                                                  \
    return xfail(h, PSDC_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(dev_scope_.err))

size_t bins(const XObj *h) { return h->n / 2 + 1; }
uint32_t cur_avg(const XObj *h, size_t k) { return stage_avg(h->avg_limit, h->avg_count, (unsigned)k); }

// lowest absolute index a stage keeps: the decimator's history, which also covers the next segment
uint64_t keep_from(const Geometry &g, const XStage &s)
{
    if (s.segs == 0)
        return 0;
    const uint64_t back = std::max<uint64_t>(g.overlap, HBF_HALO);
    return s.dec > back ? s.dec - back : 0;
}

int free_retired(XObj *h)
{
    for (void *p : h->retired)
        XCHK(h, hipFree(p));
    h->retired.clear();
    return PSDC_OK;
}

// room for the stream up to absolute index new_end in the current buffers; growing allocates a new pair of buffers and
// copies what the stage holds on the stream (no host wait); the old ones are retired
int ensure_room(XObj *h, XStage &s, uint64_t new_end)
{
    const size_t need = (size_t)(new_end - s.buf.base);
    if (need <= s.buf.cap)
        return PSDC_OK;
    const size_t cap = std::max<size_t>(need + need / 4, 4 * (size_t)h->n + 2 * HBF_HALO);
    XBuf nb;
    nb.cap = cap;
    nb.base = s.buf.base;
    for (uint32_t c = 0; c < h->m; ++c)
        for (int i = 0; i < 2; ++i)
            XCHK(h, hipMalloc(&nb.p[c][i], sizeof(float) * cap));
    const size_t held = (size_t)(s.total - s.buf.base);
    h->grew = true;
    for (uint32_t c = 0; c < h->m; ++c) {
        if (held)
            XCHK(h, hipMemcpyAsync(nb.p[c][0], s.buf.p[c][s.buf.cur], sizeof(float) * held, hipMemcpyDeviceToDevice, h->stream));
        for (int i = 0; i < 2; ++i)
            if (s.buf.p[c][i])
                h->retired.push_back(s.buf.p[c][i]);
    }
    s.buf = nb;
    return PSDC_OK;
}

int add_stage(XObj *h, std::vector<XStage> &st)
{
    if (st.size() >= X_MAX_STAGES)
        return xfail(h, PSDC_ERR_ARG, std::string(h->kind->tag) + ": more than 16 stages");
    XStage s;
    XCHK(h, hipMalloc(&s.acc, sizeof(double) * h->acc_sets() * h->rows() * bins(h)));
    XCHK(h, hipMemsetAsync(s.acc, 0, sizeof(double) * h->acc_sets() * h->rows() * bins(h), h->stream));
    st.push_back(s);
    return PSDC_OK;
}

int ensure_partial(XObj *h, size_t floats)
{
    if (floats <= h->partial_cap)
        return PSDC_OK;
    if (h->d_partial)
        h->retired.push_back(h->d_partial);
    h->d_partial = nullptr;
    const size_t cap = floats + floats / 4;
    XCHK(h, hipMalloc(&h->d_partial, sizeof(float) * cap));
    h->partial_cap = cap;
    return PSDC_OK;
}

struct PlannedCross {
    CsmJob job; // (CrossJob's fields with room for four channels)
    CrossFoldJob fold;
};

CrossJob pair_job(const CsmJob &j)
{
    CrossJob c{};
    c.src[0] = j.src[0];
    c.src[1] = j.src[1];
    c.src_base = j.src_base;
    c.seg0 = j.seg0;
    c.partial = j.partial;
    c.log2_gamma = j.log2_gamma;
    c.nseg = j.nseg;
    c.block_begin = j.block_begin;
    c.nblocks = j.nblocks;
    c.ntiles = j.ntiles;
    c.step0 = j.step0;
    c.nb = j.nb;
    c.is_m1 = j.is_m1;
    c.ewma = j.ewma;
    return c;
}

// one pipeline round over every (pair, stage); *did: some stage had work
int run_round(XObj *h, bool *did)
{
    const Geometry &g = h->geo;
    const int spt = h->kind->segments_per_tile((int)h->n, (int)h->m);
    const int nch = (int)h->m;
    std::vector<PlannedCross> cross;
    std::vector<DecJob> decs;
    std::vector<CrossTailJob> tails;
    for (auto &st : h->pairs) {
        std::vector<uint64_t> tot0(st.size());
        for (size_t k = 0; k < st.size(); ++k)
            tot0[k] = st[k].total;
        for (size_t k = 0; k < st.size(); ++k) {
            const uint64_t j_new = segments_for(g, tot0[k]);
            if (j_new <= st[k].segs)
                continue;
            XStage &s = st[k];
            const uint64_t nb = j_new - s.segs;
            if (nb > (uint64_t)std::numeric_limits<int>::max() / 2)
                return xfail(h, PSDC_ERR_ARG, std::string(h->kind->tag) + ": too many segments in one round");
            const uint32_t avg = cur_avg(h, k);
            PlannedCross pc{};
            CsmJob &cj = pc.job;
            for (int c = 0; c < nch; ++c)
                cj.src[c] = s.buf.p[c][s.buf.cur];
            cj.src_base = (long long)s.buf.base;
            cj.step0 = 1;
            auto span = [&](uint64_t seg0, uint64_t nseg) {
                cj.seg0 = (long long)seg0;
                cj.nseg = (int)nseg;
                cj.ntiles = (int)((nseg + spt - 1) / spt);
            };
            if (h->wf_block) {
                // a waterfall stage: one job a piece of a block, every segment with weight 1, folded into the block's ring slot
                pc.fold.g_total = 1.0;
                wf_cut(s.segs, j_new, h->wf_block, h->wf_depth, [&](const WfPiece &p) {
                    span(p.seg0, p.nseg);
                    cj.nb = (int)p.nseg;
                    pc.fold.acc = s.acc + (size_t)p.slot * h->rows() * bins(h);
                    pc.fold.fresh = p.fresh ? 1 : 0;
                    cross.push_back(pc);
                });
            } else {
                const EwmaPlan ew = plan_ewma(count_report(s.count64), avg, nb);
                span(s.segs, nb);
                cj.log2_gamma = ew.gamma > 0.0f ? std::log2((double)ew.gamma) : -std::numeric_limits<double>::infinity();
                cj.nb = (int)ew.nb;
                cj.is_m1 = (int)std::min<int64_t>(ew.i_s - 1, std::numeric_limits<int>::max());
                cj.ewma = ew.ewma ? 1 : 0;
                pc.fold.acc = s.acc;
                pc.fold.g_total = ew.g_total;
                cross.push_back(pc);
            }
            // decimator: samples [dec, p_new) of each channel, outputs m >= drain land in stage k + 1
            const uint64_t p_new = decimated_prefix(g, j_new);
            const uint64_t e_old = emitted_for(g, s.dec), e_new = emitted_for(g, p_new);
            if (e_new > e_old) {
                if (k + 1 == st.size()) {
                    int rc = add_stage(h, st);
                    if (rc)
                        return rc;
                    tot0.push_back(0); // (a stage made in this round has no work in it)
                }
                XStage &s0 = st[k], &s1 = st[k + 1];
                int rc = ensure_room(h, s1, s1.total + (e_new - e_old));
                if (rc)
                    return rc;
                const uint64_t m0 = std::max<uint64_t>(s0.dec >> 3, g.drain), m1 = p_new >> 3;
                for (int c = 0; c < nch; ++c) {
                    DecJob dj{};
                    dj.src = s0.buf.p[c][s0.buf.cur];
                    dj.src_base = (long long)s0.buf.base;
                    dj.m0 = (long long)m0;
                    dj.nout = (int)(m1 - m0);
                    dj.dst = s1.buf.p[c][s1.buf.cur];
                    dj.dst_base = (long long)s1.buf.base;
                    decs.push_back(dj);
                }
                s1.total += e_new - e_old;
            }
            XStage &sk = st[k];
            sk.segs = j_new;
            sk.dec = p_new;
            sk.count64 = count_after64(sk.count64, avg, nb);
        }
        // stream tails: what each stage still needs moves to the front of its other buffers
        for (auto &s : st) {
            const uint64_t keep = keep_from(g, s);
            if (keep <= s.buf.base)
                continue;
            const uint64_t count = s.total - keep;
            if (count) {
                for (int c = 0; c < nch; ++c) {
                    CrossTailJob tj{};
                    tj.src = s.buf.p[c][s.buf.cur] + (keep - s.buf.base);
                    tj.dst = s.buf.p[c][s.buf.cur ^ 1];
                    tj.count = (long long)count;
                    tj.nblocks = (int)((count + CROSS_TAIL_CHUNK - 1) / CROSS_TAIL_CHUNK);
                    tails.push_back(tj);
                }
                s.buf.cur ^= 1;
            }
            s.buf.base = keep;
        }
    }
    *did = !cross.empty();
    if (cross.empty() && decs.empty() && tails.empty())
        return PSDC_OK;

    // partial slab and workgroups: every workgroup of a launch walks the same number of tiles, and the launch's workgroups are
    // about what the device holds at once (a job of few tiles next to one of many would otherwise make some workgroups walk
    // one tile more than the rest: a round with the decimated stages read 240 us where stage 0 alone read 160)
    const size_t rows = h->rows() * bins(h);
    std::vector<int> nblk(cross.size());
    size_t slab = 0;
    for (size_t b0 = 0; b0 < cross.size(); b0 += CROSS_MAX_JOBS) {
        const size_t b1 = std::min(cross.size(), b0 + CROSS_MAX_JOBS);
        int64_t tiles = 0;
        for (size_t i = b0; i < b1; ++i)
            tiles += cross[i].job.ntiles;
        const int64_t per = (tiles + h->resident - 1) / h->resident; // tiles a workgroup
        for (size_t i = b0; i < b1; ++i) {
            const int64_t t = cross[i].job.ntiles;
            nblk[i] = (int)((t + per - 1) / per);
            slab += (size_t)nblk[i] * rows;
        }
    }
    int rc = ensure_partial(h, slab);
    if (rc)
        return rc;
    size_t off = 0;
    for (size_t b0 = 0; b0 < cross.size(); b0 += CROSS_MAX_JOBS) {
        int nblocks = 0;
        for (size_t i = b0; i < std::min(cross.size(), b0 + CROSS_MAX_JOBS); ++i) {
            CsmJob &cj = cross[i].job;
            cj.partial = h->d_partial + off;
            cj.nblocks = nblk[i];
            cj.block_begin = nblocks;
            cross[i].fold.partial = cj.partial;
            cross[i].fold.nparts = nblk[i];
            off += (size_t)nblk[i] * rows;
            nblocks += nblk[i];
        }
        auto fill = [&](auto *cb, auto conv) {
            cb->hop = (int)g.hop;
            cb->detrend = h->detrend;
            cb->nblocks = nblocks;
            for (size_t i = b0; i < std::min(cross.size(), b0 + CROSS_MAX_JOBS); ++i)
                cb->jobs[cb->njobs++] = conv(cross[i].job);
        };
        hipError_t e;
        if (h->kind->launch_group) {
            CsmBatch *cb = new CsmBatch();
            fill(cb, [](const CsmJob &j) { return j; });
            e = h->kind->launch_group(*h, *cb);
            delete cb;
        } else {
            CrossBatch *cb = new CrossBatch();
            fill(cb, pair_job);
            e = h->kind->launch_pair((int)h->n, *cb, h->d_win, h->d_tw, h->stream);
            delete cb;
        }
        XCHK(h, e);
        ++h->launches;
    }
    for (size_t b0 = 0; b0 < decs.size(); b0 += MAX_JOBS) {
        DecBatch *db = new DecBatch();
        db->drain = (int)g.drain;
        for (size_t i = b0; i < std::min(decs.size(), b0 + MAX_JOBS); ++i) {
            DecJob dj = decs[i];
            dj.tile_begin = db->ntiles;
            db->jobs[db->njobs++] = dj;
            db->ntiles += (dj.nout + DEC_TILE - 1) / DEC_TILE;
        }
        hipError_t e = launch_dec(*db, h->stream);
        const bool any = db->ntiles > 0;
        delete db;
        XCHK(h, e);
        if (any)
            ++h->launches;
    }
    size_t fi = 0, ti = 0;
    while (fi < cross.size() || ti < tails.size()) {
        CrossPostBatch *pb = new CrossPostBatch();
        pb->nbins = (int)bins(h);
        pb->nrows = (int)h->rows();
        pb->fold_xb = cross_fold_blocks((int)h->rows(), (int)bins(h));
        for (; fi < cross.size() && pb->nfold < CROSS_MAX_FOLD; ++fi) {
            // a round longer than a waterfall ring folds into a slot more than once: a launch's folds run in no order, so a slot's
            // next fold waits for the next launch (the pieces are in segment order: the newest block is the one that stays)
            if (h->wf_block && std::any_of(pb->fold, pb->fold + pb->nfold, [&](const CrossFoldJob &f) { return f.acc == cross[fi].fold.acc; }))
                break;
            pb->fold[pb->nfold++] = cross[fi].fold;
        }
        for (; ti < tails.size() && pb->ntail < CROSS_MAX_TAIL; ++ti) {
            CrossTailJob tj = tails[ti];
            tj.block_begin = pb->tail_blocks;
            pb->tail_blocks += tj.nblocks;
            pb->tail[pb->ntail++] = tj;
        }
        hipError_t e = launch_cross_post(*pb, h->stream);
        delete pb;
        XCHK(h, e);
        ++h->launches;
    }
    const int slot = (int)(h->rounds & 1);
    XCHK(h, hipEventRecord(h->ev_round[slot], h->stream));
    h->round_recorded[slot] = true;
    ++h->rounds;
    return PSDC_OK;
}

int drain(XObj *h)
{
    if (h->idle)
        return PSDC_OK;
    for (;;) {
        bool did = false;
        int rc = run_round(h, &did);
        if (rc)
            return rc;
        if (!did)
            break;
    }
    h->idle = true;
    return PSDC_OK;
}

int sync_all(XObj *h)
{
    XCHK(h, hipStreamSynchronize(h->copy_stream));
    XCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 2; ++i)
        h->ev_pending[i] = false;
    return free_retired(h);
}

// who: the call to name in the text (the integer feeds do); NULL: the object's family
int check_pair(XObj *h, uint32_t pair, const char *who = nullptr)
{
    if (pair >= h->n_pairs)
        return xfail(h, PSDC_ERR_ARG, std::string(who ? who : h->kind->tag) + ": " + h->kind->unit + " " + std::to_string(pair) + " out of range (" +
                                          h->kind->units + " " + std::to_string(h->n_pairs) + ")");
    return PSDC_OK;
}

// stage 0 of a pair takes len more samples of each channel: room for them, and where they go
int stage0_room(XObj *h, uint32_t pair, size_t len, XStage **out)
{
    auto &st = h->pairs[pair];
    if (st.empty()) {
        int rc = add_stage(h, st);
        if (rc)
            return rc;
    }
    int rc = ensure_room(h, st[0], st[0].total + len);
    if (rc)
        return rc;
    *out = &st[0];
    return PSDC_OK;
}

void free_all(XObj *h)
{
    (void)hipStreamSynchronize(h->copy_stream);
    (void)hipStreamSynchronize(h->stream);
    for (auto &st : h->pairs)
        for (auto &s : st) {
            for (int c = 0; c < CSM_MAX_M; ++c)
                for (int i = 0; i < 2; ++i)
                    if (s.buf.p[c][i])
                        (void)hipFree(s.buf.p[c][i]);
            if (s.acc)
                (void)hipFree(s.acc);
        }
    h->pairs.assign(h->n_pairs, {});
    for (void *p : h->retired)
        (void)hipFree(p);
    h->retired.clear();
    if (h->d_partial)
        (void)hipFree(h->d_partial);
    h->d_partial = nullptr;
    h->partial_cap = 0;
    h->idle = true;
}

// why a matrix object cannot have these sizes ("": it can)
std::string csm_refusal(uint32_t n, uint32_t m)
{
    if (csm_supported(n <= 4096 ? (int)n : 0, m <= CSM_MAX_M ? (int)m : 0))
        return "";
    if (m < 2 || m > CSM_MAX_M)
        return "m = " + std::to_string(m) + " is not supported: a group has 2 to 4 channels";
    return "n = " + std::to_string(n) + " with m = " + std::to_string(m) +
           " is not supported: n must be a power of two in [64, 2048], or 4096 with m = 2 or 3";
}

// why a zoom cross object cannot have this size ("": it can)
std::string zcsd_refusal(uint32_t n, uint32_t)
{
    if (zoom_cross_supported(n <= 4096 ? (int)n : 0))
        return "";
    return "n = " + std::to_string(n) + " is not supported: n must be a power of two in [64, " +
           (zoom_cross_supported(4096) ? "4096]" : "2048]");
}

// One row a family.  A pair object is m = 2 on cross_kernel; a matrix object 2 <= m <= 4 on csm_kernel; a zoom object m = 2 (I and
// Q) on zoom_kernel; a zoom cross object m = 4 (I and Q of two channels) on zoom_cross_kernel; psdc_iq is psdc_zoom and psdc_iqcsd
// is psdc_zcsd with the IQ feed; psdc_sk is m = 1 on sk_kernel; psdc_zsk / psdc_iqsk are psdc_zoom / psdc_iq on zoom_sk_kernel;
// psdc_zampm / psdc_iqampm are psdc_zoom / psdc_iq on zoom_ampm_kernel; psdc_zxampm / psdc_iqxampm are psdc_zcsd / psdc_iqcsd on
// zoom_ampm_cross_kernel, which launch_zoom_cross runs for a batch marked ZCROSS_VARIANT_AMPM.
// psdc_wf / psdc_zwf are psdc_sk / psdc_zsk with a ring of row sets a stage (XObj::wf_block, run_round).
enum Kind { K_CROSS, K_CSM, K_ZOOM, K_ZCSD, K_IQ, K_IQCSD, K_SK, K_ZSK, K_IQSK, K_ZAMPM, K_IQAMPM, K_ZXAMPM, K_IQXAMPM, K_WF, K_ZWF };
constexpr auto SPT_CROSS = [](int n, int) { return cross_segments_per_tile(n); };
constexpr auto SPT_ZOOM = [](int n, int) { return zoom_segments_per_tile(n); };
constexpr auto SPT_ZCSD = [](int n, int) { return zoom_cross_segments_per_tile(n); };
constexpr auto SPT_SK = [](int n, int) { return sk_segments_per_tile(n); };
constexpr auto GROUP_CSM = [](const XObj &h, CsmBatch &b) { return launch_csm((int)h.n, (int)h.m, b, h.d_win, h.d_tw, h.stream); };
constexpr auto GROUP_ZCSD = [](const XObj &h, CsmBatch &b) { return launch_zoom_cross((int)h.n, b, h.d_win, h.d_tw, h.stream); };
constexpr auto GROUP_ZXAMPM = [](const XObj &h, CsmBatch &b) {
    b.variant = ZCROSS_VARIANT_AMPM;
    return launch_zoom_cross((int)h.n, b, h.d_win, h.d_tw, h.stream);
};
constexpr KindDesc KINDS[] = {
    // tag, unit, units, m, rows, feed, segments a tile, segment kernel (pair | group), refusal
    {"psdc_cross", "pair", "n_pairs", 2, 4, Feed::PLAIN, SPT_CROSS, launch_cross, nullptr, nullptr},
    {"psdc_csm", "group", "n_groups", 0, 0, Feed::PLAIN, csm_segments_per_tile, nullptr, GROUP_CSM, csm_refusal},
    {"psdc_zoom", "channel", "n_channels", 2, 2, Feed::ZOOM, SPT_ZOOM, launch_zoom, nullptr, nullptr},
    {"psdc_zcsd", "pair", "n_pairs", 4, 8, Feed::ZOOM, SPT_ZCSD, nullptr, GROUP_ZCSD, zcsd_refusal},
    {"psdc_iq", "channel", "n_channels", 2, 2, Feed::IQ, SPT_ZOOM, launch_zoom, nullptr, nullptr},
    {"psdc_iqcsd", "pair", "n_pairs", 4, 8, Feed::IQ, SPT_ZCSD, nullptr, GROUP_ZCSD, zcsd_refusal},
    {"psdc_sk", "channel", "n_channels", 1, 2, Feed::PLAIN, SPT_SK, launch_sk, nullptr, nullptr},
    {"psdc_zsk", "channel", "n_channels", 2, ZSK_ROWS, Feed::ZOOM, SPT_ZOOM, launch_zoom_sk, nullptr, nullptr},
    {"psdc_iqsk", "channel", "n_channels", 2, ZSK_ROWS, Feed::IQ, SPT_ZOOM, launch_zoom_sk, nullptr, nullptr},
    {"psdc_zampm", "channel", "n_channels", 2, ZAMPM_ROWS, Feed::ZOOM, SPT_ZOOM, launch_zoom_ampm, nullptr, nullptr},
    {"psdc_iqampm", "channel", "n_channels", 2, ZAMPM_ROWS, Feed::IQ, SPT_ZOOM, launch_zoom_ampm, nullptr, nullptr},
    {"psdc_zxampm", "pair", "n_pairs", 4, ZXAMPM_ROWS, Feed::ZOOM, SPT_ZCSD, nullptr, GROUP_ZXAMPM, zcsd_refusal},
    {"psdc_iqxampm", "pair", "n_pairs", 4, ZXAMPM_ROWS, Feed::IQ, SPT_ZCSD, nullptr, GROUP_ZXAMPM, zcsd_refusal},
    {"psdc_wf", "channel", "n_channels", 1, SK_ROWS, Feed::PLAIN, SPT_SK, launch_sk, nullptr, nullptr},
    {"psdc_zwf", "channel", "n_channels", 2, ZSK_ROWS, Feed::ZOOM, SPT_ZOOM, launch_zoom_sk, nullptr, nullptr},
};
static_assert(sizeof(KINDS) / sizeof(KINDS[0]) == K_ZWF + 1, "one row a kind");

// "": the arguments are fine
std::string check_args(const KindDesc &kind, uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs)
{
    if (kind.m && (n < 64 || n > 4096 || (n & (n - 1)) != 0)) // (the caller's m: the kind's refusal has looked at n with it)
        return "n must be a power of two in [64, 4096]";
    if (!win)
        return "null window table";
    if (overlap >= n || (n - overlap) % 8 != 0)
        return "the window's overlap must be < n with (n - overlap) % 8 == 0";
    if (!(power > 0.0f) || !(nenbw > 0.0f))
        return "window power and nenbw must be > 0";
    if (n_pairs < 1 || n_pairs > X_MAX_PAIRS)
        return std::string(kind.units) + " must be in [1, 65536]";
    return "";
}

void destroy_impl(XObj *h);

// m: the caller's, for the kind that has none of its own
XObj *create_impl(const KindDesc &kind, uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                  int device, const char *who, uint32_t m = 0)
{
    if (kind.m)
        m = kind.m;
    std::string why = kind.refusal ? kind.refusal(n, m) : "";
    if (why.empty())
        why = check_args(kind, n, win, power, nenbw, overlap, n_pairs);
    if (!why.empty()) {
        xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": " + why);
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        xfail(nullptr, PSDC_ERR_DEVICE, std::string(who) + ": no HIP device (there is no CPU fallback): " +
                                            (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": device " + std::to_string(device) + " out of range");
        return nullptr;
    }
    psdrt::DevScope scope(device);
    if (scope.err != hipSuccess) {
        xfail(nullptr, PSDC_ERR_DEVICE, std::string(who) + ": hipSetDevice: " + hipGetErrorString(scope.err));
        return nullptr;
    }
    XObj *h = new XObj();
    h->kind = &kind;
    h->n = n;
    h->m = m;
    if (h->mixed()) {
        h->ftw.assign((size_t)n_pairs * h->reals(), 0);
        h->phase0.assign((size_t)n_pairs * h->reals(), 0);
    }
    h->n_pairs = n_pairs;
    h->device = device;
    h->geo.n = n;
    h->geo.overlap = (uint32_t)overlap;
    h->geo.hop = n - (uint32_t)overlap;
    h->geo.drain = 35;
    h->power = power;
    h->nenbw = nenbw;
    h->pairs.assign(n_pairs, {});
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        // twice what is resident at one wavefront a SIMD (the kernel's registers allow no more); once and twice read the same
        // end to end within the noise of tools/cross_probe.py (N = 1024, one pair: 43.9 against 45.4 G pairs/s)
        h->resident = std::max<int64_t>(1, 2 * (int64_t)cus * 4 * 64 /
                                               (kind.m ? cross_block_threads((int)n) : csm_block_threads((int)n, (int)m)));
    std::vector<cf> tw(n);
    for (uint32_t j = 0; j < n; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)n;
        tw[j] = {(float)cos(a), (float)sin(a)};
    }
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_round[0], hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_round[1], hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_copy, hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&h->ev_grow, hipEventDisableTiming) == hipSuccess &&
              hipMalloc(&h->d_win, sizeof(float) * n) == hipSuccess && hipMalloc(&h->d_tw, sizeof(cf) * n) == hipSuccess &&
              hipMemcpy(h->d_win, win, sizeof(float) * n, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(h->d_tw, tw.data(), sizeof(cf) * n, hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; ok && i < 2; ++i)
        ok = hipHostMalloc(&h->h_stage[i], sizeof(float) * h->lanes() * STAGING) == hipSuccess &&
             hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        xfail(nullptr, PSDC_ERR_DEVICE, std::string(who) + ": device allocation failed");
        destroy_impl(h);
        delete h;
        return nullptr;
    }
    return h;
}


// ---- the feed skeleton: how samples reach stage 0 ----
//
// Every feed ends in run_round on the compute stream (h->stream); what differs is the way into stage 0.
//   * Host samples of the objects without a mixer (process_impl) go up on the compute stream itself, through a pinned staging slot:
//     nothing to order.
//   * Everything else is written into stage 0 on the copy stream, beside the kernels of the round before: device samples (copied, or
//     converted by one launch), mixer launches (whose host samples go up through a staging slot into the landing buffer d_land
//     first, in pieces of STAGING samples) and frames decodes.  The event rules are those at XObj::copy_stream, and they are
//     written out once, in feed_open and feed_close: the copy stream waits for the producer's event, for a grown buffer's move
//     (ev_grow) and for round R - 2 (ev_round[R & 1]); round R waits for the copy stream (ev_copy).  Pieces of one call need
//     no events between them: the uploads into the landing buffer and the mixers that read it are all on the copy stream.
//   * A pinned staging slot is written by the host again only once the upload that read it last is done (stage_upload).
// Host and device sources make the same launches on the same data -- a host piece is the device piece with the landing buffer as
// its source -- and an integer call makes the launches of the f32 call of the same length (the raw integers take the front of each
// staging and landing lane; the mixers convert them in registers, sample_int.h), so the same calls give the same bits on every route.

// one stream of a staged upload: `bytes` from host memory at src, through the slot at float offset `off`, to device memory at dst
struct Lane {
    const void *src;
    size_t bytes, off;
    void *dst;
};

// Take the next pinned staging slot (waiting for the upload that read it last), fill its lanes and send them up on `stream`.
// threaded: copy with psdrt::pinned_copy, which splits a large copy over a few threads (the frames path).
int stage_upload(XObj *h, hipStream_t stream, const Lane *lanes, uint32_t n, bool threaded = false)
{
    const int slot = h->stage_cur;
    if (h->ev_pending[slot])
        XCHK(h, hipEventSynchronize(h->stage_ev[slot]));
    for (uint32_t i = 0; i < n; ++i) {
        float *stg = h->h_stage[slot] + lanes[i].off;
        if (threaded)
            psdrt::pinned_copy(stg, lanes[i].src, lanes[i].bytes);
        else
            memcpy(stg, lanes[i].src, lanes[i].bytes);
        XCHK(h, hipMemcpyAsync(lanes[i].dst, stg, lanes[i].bytes, hipMemcpyHostToDevice, stream));
    }
    XCHK(h, hipEventRecord(h->stage_ev[slot], stream));
    h->ev_pending[slot] = true;
    h->stage_cur ^= 1;
    return PSDC_OK;
}

// Open the copy stream for what round R = h->rounds will read.  The caller has cleared h->grew and made room in stage 0
// (stage0_room) for every unit it feeds.
int feed_open(XObj *h, void *producer_event)
{
    if (producer_event)
        XCHK(h, hipStreamWaitEvent(h->copy_stream, (hipEvent_t)producer_event, 0));
    if (h->grew) { // the held samples move to the new buffers on the compute stream: the copy stream goes behind them
        XCHK(h, hipEventRecord(h->ev_grow, h->stream));
        XCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_grow, 0));
    }
    const int slot = (int)(h->rounds & 1); // round R - 2
    if (h->round_recorded[slot])
        XCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_round[slot], 0));
    return PSDC_OK;
}

// The copy stream's work is enqueued and the caller has counted the samples in: round R goes behind it.
int feed_close(XObj *h)
{
    XCHK(h, hipEventRecord(h->ev_copy, h->copy_stream));
    XCHK(h, hipStreamWaitEvent(h->stream, h->ev_copy, 0));
    h->idle = false;
    bool did = false;
    return run_round(h, &did);
}

// ---- frames (psdc_csd_process_frames[_device]) ----

struct FedPair {
    uint32_t pair;
    uint32_t tr[CSM_MAX_M]; // the trace of each channel
};

// the pairs a call feeds, from its map (map_w() entries a unit); PSDC_ERR_ARG for a NULL map, an entry with exactly one
// PSDC_TRACE_NONE or a trace no format carries
int read_map(XObj *h, const uint32_t *map, const char *who, std::vector<FedPair> *fed)
{
    if (!map)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null " + h->kind->unit + " map");
    fed->clear();
    const uint32_t w = h->map_w();
    for (uint32_t p = 0; p < h->n_pairs; ++p) {
        FedPair fp{};
        fp.pair = p;
        uint32_t none = 0, top = 0;
        for (uint32_t c = 0; c < w; ++c) {
            fp.tr[c] = map[w * p + c];
            if (fp.tr[c] == PSDC_TRACE_NONE)
                ++none;
            else
                top = std::max(top, fp.tr[c]);
        }
        if (none == w)
            continue;
        if (none)
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": " + h->kind->unit + " " + std::to_string(p) +
                                              (w == 2 ? " names one trace and PSDC_TRACE_NONE"
                                                         : " names PSDC_TRACE_NONE for some of its traces only"));
        if (top >= 4)
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": " + h->kind->unit + " " + std::to_string(p) + " names trace " +
                                              std::to_string(top) + " (frames carry at most 4)");
        fed->push_back(fp);
    }
    if (h->mixed() && fed->empty()) // (a pair object takes such a call for its Loss)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": the map feeds no " + h->kind->unit);
    return PSDC_OK;
}

// Where a call's frames are: the payloads in host memory (host) or on the device (dev), the headers in host memory either way
struct FrameSrc {
    const uint8_t *host = nullptr;
    const uint8_t *dev = nullptr;
    psdrt::HdrView hdr{nullptr, 0};
};

// decode frames [f, f + cnt) of src (format wf, `batches` a frame) into the stage-0 buffers at dst[m i + c] (pair fed[i], channel
// c), one launch per 32 / m pairs, on the copy stream.  A zoom channel's two buffers are its I and Q streams: zoom_frames_kernel
// decodes the channel's trace and mixes it with the channel's carrier, the first sample at stream index total + dst_off.  A zoom
// cross pair's four are I_a, Q_a, I_b, Q_b: zoom_cross_frames_kernel does the same for both sides of 8 pairs a launch, where
// psdc_zcsd_process_device has its two mixers.  An IQ channel's two are its I and Q as well, made of two traces by iq_frames_kernel;
// an IQ cross pair's four are made of four traces by iq_cross_frames_kernel, 8 pairs a launch.
int decode_frames(XObj *h, const FrameSrc &src, size_t frame_size, const WireFmt *wf, int batches, size_t f, size_t cnt,
                  const std::vector<FedPair> &fed, const std::vector<float *> &dst, size_t dst_off)
{
    const uint8_t *frames = src.dev ? src.dev + f * frame_size : nullptr;
    if (!src.dev) { // host memory: up through a pinned staging slot into d_frames (the decode of the chunk before has read it:
                    // both are on the copy stream)
        if (!h->d_frames)
            XCHK(h, hipMalloc(&h->d_frames, h->frames_chunk()));
        const Lane up{src.host + f * frame_size, cnt * frame_size, 0, h->d_frames};
        int rc = stage_upload(h, h->copy_stream, &up, 1, true);
        if (rc)
            return rc;
        frames = h->d_frames;
    }
    // what both kinds of launch say about the frames
    auto describe = [&](auto *b) {
        b->frames = frames;
        b->frame_size = frame_size;
        b->n_frames = (unsigned)cnt;
        b->batches = batches;
        b->fmt = wf->id;
    };
    const Feed feed = h->kind->feed;
    const bool two_sided = h->mixed() && h->m == 4; // two channels a unit
    if (two_sided && feed == Feed::IQ) {
        for (size_t i0 = 0; i0 < fed.size(); i0 += IQ_CROSS_FRAMES_MAX_PAIRS) {
            IqCrossFramesBatch b{};
            describe(&b);
            for (size_t i = i0; i < std::min<size_t>(fed.size(), i0 + IQ_CROSS_FRAMES_MAX_PAIRS); ++i, ++b.npairs) {
                const uint32_t p = fed[i].pair;
                for (int side = 0; side < 2; ++side) {
                    b.ftw[b.npairs][side] = h->ftw[2 * (size_t)p + side];
                    b.phase0[b.npairs][side] = h->phase0[2 * (size_t)p + side];
                }
                for (int c = 0; c < 4; ++c) { // I_a, Q_a, I_b, Q_b: the map's order and the order iq_pair_feed's mixer writes them in
                    b.trace[b.npairs][c] = (int)fed[i].tr[c];
                    b.dst[b.npairs][c] = dst[4 * i + c] + dst_off;
                }
                b.j0[b.npairs] = h->pairs[p][0].total + dst_off; // the stream index of both sides, as iq_pair_feed counts it
            }
            XCHK(h, launch_iq_cross_frames(b, h->copy_stream));
            ++h->launches;
        }
    } else if (two_sided) {
        for (size_t i0 = 0; i0 < fed.size(); i0 += ZOOM_CROSS_FRAMES_MAX_PAIRS) {
            ZoomCrossFramesBatch b{};
            describe(&b);
            for (size_t i = i0; i < std::min<size_t>(fed.size(), i0 + ZOOM_CROSS_FRAMES_MAX_PAIRS); ++i, ++b.npairs) {
                const uint32_t p = fed[i].pair;
                for (int side = 0; side < 2; ++side) {
                    b.trace[b.npairs][side] = (int)fed[i].tr[side];
                    b.ftw[b.npairs][side] = h->ftw[2 * (size_t)p + side];
                    b.phase0[b.npairs][side] = h->phase0[2 * (size_t)p + side];
                }
                for (int c = 0; c < 4; ++c) // I_a, Q_a, I_b, Q_b: the order zoom_feed's mixers write them in
                    b.dst[b.npairs][c] = dst[4 * i + c] + dst_off;
                b.j0[b.npairs] = h->pairs[p][0].total + dst_off; // the stream index of both sides, as zoom_feed counts it
            }
            XCHK(h, launch_zoom_cross_frames(b, h->copy_stream));
            ++h->launches;
        }
    } else if (feed == Feed::IQ) {
        for (size_t i0 = 0; i0 < fed.size(); i0 += ZOOM_FRAMES_MAX_CH) {
            IqFramesBatch b{};
            describe(&b);
            for (size_t i = i0; i < std::min<size_t>(fed.size(), i0 + ZOOM_FRAMES_MAX_CH); ++i, ++b.nch) {
                const uint32_t ch = fed[i].pair;
                b.trace_i[b.nch] = (int)fed[i].tr[0];
                b.trace_q[b.nch] = (int)fed[i].tr[1];
                b.dst_i[b.nch] = dst[2 * i] + dst_off;
                b.dst_q[b.nch] = dst[2 * i + 1] + dst_off;
                b.ftw[b.nch] = h->ftw[ch];
                b.phase0[b.nch] = h->phase0[ch];
                b.j0[b.nch] = h->pairs[ch][0].total + dst_off; // the stream index, as iq_feed counts it
            }
            XCHK(h, launch_iq_frames(b, h->copy_stream));
            ++h->launches;
        }
    } else if (feed == Feed::ZOOM) {
        for (size_t i0 = 0; i0 < fed.size(); i0 += ZOOM_FRAMES_MAX_CH) {
            ZoomFramesBatch b{};
            describe(&b);
            for (size_t i = i0; i < std::min<size_t>(fed.size(), i0 + ZOOM_FRAMES_MAX_CH); ++i, ++b.nch) {
                const uint32_t ch = fed[i].pair;
                b.trace[b.nch] = (int)fed[i].tr[0];
                b.dst_i[b.nch] = dst[2 * i] + dst_off;
                b.dst_q[b.nch] = dst[2 * i + 1] + dst_off;
                b.ftw[b.nch] = h->ftw[ch];
                b.phase0[b.nch] = h->phase0[ch];
                b.j0[b.nch] = h->pairs[ch][0].total + dst_off; // the stream index, as zoom_feed counts it
            }
            XCHK(h, launch_zoom_frames(b, h->copy_stream));
            ++h->launches;
        }
    } else {
        const size_t per_launch = CROSS_FRAMES_MAX_DST / h->m;
        for (size_t i0 = 0; i0 < fed.size(); i0 += per_launch) {
            CrossFramesBatch b{};
            describe(&b);
            for (size_t i = i0; i < std::min(fed.size(), i0 + per_launch); ++i)
                for (uint32_t c = 0; c < h->m; ++c) {
                    b.trace[b.ndst] = (int)fed[i].tr[c];
                    b.dst[b.ndst] = dst[h->m * i + c] + dst_off;
                    ++b.ndst;
                }
            XCHK(h, launch_cross_frames(b, h->copy_stream));
            ++h->launches;
        }
    }
    return PSDC_OK;
}

// One call's frames, taken by the rule of psdc_process_frames -- run_start and scan_piece of frame_scan.h: runs of one format, every
// header validated on the host -- with Loss committed piece by piece once the piece's samples are in the streams.  A run is cut into
// pieces of whole frames of <= PIECE_SAMPLES samples a trace; each piece is decoded and followed by one round.  The cut depends on
// the headers alone, so host and device frames give the same rounds.
int ingest_frames(XObj *h, const std::vector<FedPair> &fed, const FrameSrc &src, size_t frame_size, size_t n_frames,
                  size_t *good_out, const char *who)
{
    size_t &good = *good_out;
    const size_t payload = frame_size - 8;
    int bad = PSDC_OK;
    size_t f0 = 0;
    while (f0 < n_frames && bad == PSDC_OK) {
        const WireFmt *wf = nullptr;
        bad = psdrt::run_start(src.hdr, f0, false, &wf);
        if (bad != PSDC_OK)
            break;
        for (const FedPair &fp : fed) {
            const uint32_t top = *std::max_element(fp.tr, fp.tr + h->map_w());
            if ((int)top >= wf->ntraces)
                return xfail(h, PSDC_ERR_ARG, std::string(who) + ": " + h->kind->unit + " " + std::to_string(fp.pair) + " names trace " +
                                                  std::to_string(top) + " but " + wf->name + " frames carry " +
                                                  std::to_string(wf->ntraces) + " (frame " + std::to_string(f0) + ")");
        }
        const int batches = (int)(payload / (size_t)wf->batch_bytes);
        const size_t per_frame = (size_t)batches * (size_t)wf->spb; // samples a trace and frame
        const size_t piece_frames = per_frame ? std::max<size_t>(1, PIECE_SAMPLES / per_frame) : n_frames;
        int stop = psdrt::SCAN_LIMIT;
        while (f0 < n_frames && stop == psdrt::SCAN_LIMIT) {
            psdc_loss trial = h->loss; // the piece's headers and Loss::update
            const size_t cnt = psdrt::scan_piece(src.hdr, *wf, payload, f0, std::min(piece_frames, n_frames - f0), false, &trial, &stop);
            if (cnt == 0)
                break;
            if (batches > 0 && !fed.empty()) {
                const size_t per_ch = cnt * per_frame;
                // stage 0 of every fed pair takes per_ch more samples of each channel
                std::vector<float *> dst(h->m * fed.size());
                h->grew = false;
                for (size_t i = 0; i < fed.size(); ++i) {
                    XStage *s = nullptr;
                    int rc = stage0_room(h, fed[i].pair, per_ch, &s);
                    if (rc)
                        return rc;
                    for (uint32_t c = 0; c < h->m; ++c)
                        dst[h->m * i + c] = s->buf.p[c][s->buf.cur] + (s->total - s->buf.base);
                }
                int rc = feed_open(h, nullptr); // (a device call's producer has been waited for: frames_device_impl)
                if (rc)
                    return rc;
                const size_t chunk = src.dev ? cnt : std::max<size_t>(1, h->frames_chunk() / frame_size);
                for (size_t c0 = 0; c0 < cnt; c0 += chunk) {
                    rc = decode_frames(h, src, frame_size, wf, batches, f0 + c0, std::min(chunk, cnt - c0), fed, dst,
                                           c0 * per_frame);
                    if (rc)
                        return rc;
                }
                for (const FedPair &fp : fed) {
                    h->pairs[fp.pair][0].total += per_ch;
                    h->pairs_in += per_ch;
                }
                h->loss = trial; // the piece is in the streams: its frames count from here on
                good += cnt;
                if ((rc = feed_close(h)))
                    return rc;
            } else { // header-only frames, or no pair fed: Loss only
                h->loss = trial;
                good += cnt;
            }
            f0 += cnt;
        }
        if (stop < 0)
            bad = stop;
    }
    if (bad != PSDC_OK)
        return xfail(h, bad, std::string(who) + ": " + psdrt::frame_error_text(bad) + " (frame " + std::to_string(good) + ")");
    return PSDC_OK;
}

// the checks both frames calls begin with; *go: there are frames to take
int frames_args(XObj *h, const uint32_t *map, const void *frames, size_t frame_size, size_t n_frames, const char *who,
                std::vector<FedPair> *fed, bool *go)
{
    *go = false;
    int rc = read_map(h, map, who, fed);
    if (rc)
        return rc;
    rc = psdrt::check_frames_call(frames, frame_size, n_frames, go);
    if (rc)
        return xfail(h, rc, std::string(who) + ": " + (rc == PSDC_ERR_ARG ? "null frames" : psdrt::FRAME_SHORT_TEXT));
    if (n_frames > (size_t)std::numeric_limits<uint32_t>::max())
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": more than 2^32 - 1 frames in one call");
    return PSDC_OK;
}


#define X_HANDLE(h, who)                                                                                               \
    if (!(h))                                                                                                          \
    return xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": null handle")

void destroy_impl(XObj *h)
{
    psdrt::DevScope scope(h->device);
    if (h->stream && h->copy_stream)
        free_all(h);
    delete h->bank_read;
    h->bank_read = nullptr;
    for (int i = 0; i < 2; ++i) {
        if (h->h_stage[i])
            (void)hipHostFree(h->h_stage[i]);
        if (h->stage_ev[i])
            (void)hipEventDestroy(h->stage_ev[i]);
    }
    if (h->d_frames)
        (void)hipFree(h->d_frames);
    if (h->d_land)
        (void)hipFree(h->d_land);
    h->hdr.release();
    if (h->d_win)
        (void)hipFree(h->d_win);
    if (h->d_tw)
        (void)hipFree(h->d_tw);
    for (hipEvent_t e : {h->ev_round[0], h->ev_round[1], h->ev_copy, h->ev_grow})
        if (e)
            (void)hipEventDestroy(e);
    if (h->copy_stream)
        (void)hipStreamDestroy(h->copy_stream);
    if (h->stream)
        (void)hipStreamDestroy(h->stream);
}

XObj *create_kind(const KindDesc &kind, uint32_t n, int window_kind, uint32_t n_pairs, int device, const char *who, uint32_t m = 0)
{
    psdrt::WindowConsts wc{};
    std::string why = kind.refusal ? kind.refusal(n, m) : ""; // (before the window: a refused size names itself)
    if (why.empty() && (window_kind == PSDC_WINDOW_CUSTOM || !psdrt::window_consts(n, window_kind, &wc)))
        why = "window_kind must be PSDC_WINDOW_HANN or PSDC_WINDOW_RECTANGULAR";
    if (why.empty() && (n < 64 || n > 4096 || (n & (n - 1)) != 0))
        why = "n must be a power of two in [64, 4096]";
    if (!why.empty()) {
        xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": " + why);
        return nullptr;
    }
    std::vector<float> win(n);
    psdrt::window_weights(n, window_kind, win.data());
    return create_impl(kind, n, win.data(), wc.power, wc.nenbw, wc.overlap, n_pairs, device, who, m);
}

void destroy_obj(XObj *h)
{
    if (!h)
        return;
    destroy_impl(h);
    delete h;
}

int reset_impl(XObj *h, const char *who)
{
    X_HANDLE(h, who);
    X_ON_DEVICE(h);
    // everything the object made since it was created goes: stages, buffers, partial slab, counters
    free_all(h);
    h->detrend = PSDC_DETREND_NONE;
    h->avg_limit = h->avg_count = 0xFFFFFFFFu;
    h->stage_cur = 0;
    h->ev_pending[0] = h->ev_pending[1] = false;
    h->launches = h->pairs_in = 0;
    h->loss = psdc_loss{};
    std::fill(h->ftw.begin(), h->ftw.end(), 0);
    std::fill(h->phase0.begin(), h->phase0.end(), 0);
    h->rounds = 0;
    h->round_recorded[0] = h->round_recorded[1] = false;
    return PSDC_OK;
}

int set_detrend_impl(XObj *h, int detrend_kind, const char *who)
{
    X_HANDLE(h, who);
    if (detrend_kind == PSDC_DETREND_LINEAR)
        return xfail(h, PSDC_ERR_UNIMPLEMENTED, std::string(who) + ": Detrend::Linear is unimplemented (src/psd.rs:110)");
    if (detrend_kind < PSDC_DETREND_NONE || detrend_kind > PSDC_DETREND_MEAN)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": unknown detrend kind");
    X_ON_DEVICE(h);
    int rc = drain(h); // segments already fed are analysed with the setting they were fed under
    if (rc)
        return rc;
    h->detrend = detrend_kind;
    return PSDC_OK;
}

int set_avg_impl(XObj *h, uint32_t limit, uint32_t count, const char *who)
{
    X_HANDLE(h, who);
    X_ON_DEVICE(h);
    int rc = drain(h);
    if (rc)
        return rc;
    h->avg_limit = limit;
    h->avg_count = count;
    return PSDC_OK;
}

// The number format of a sample call: f32 (every psdc_*_process call) or the integers of the psdc_int_* calls, which the mixer
// converts as (float)v * scale (sample_int.h).
struct SampleFmt {
    int kind = SAMPLE_F32;
    float scale = 1.0f;
    size_t bytes() const { return kind == SAMPLE_F32 ? sizeof(float) : (size_t)sint_bytes(kind); } // of one number
};

// the psdc_int_* calls' format; the kind and the scale are checked by check_fmt
SampleFmt int_fmt(int kind, float scale)
{
    SampleFmt f;
    f.kind = kind == PSDC_SAMPLE_S16 ? SAMPLE_S16 : kind == PSDC_SAMPLE_S8 ? SAMPLE_S8 : -1;
    f.scale = scale;
    return f;
}

int check_fmt(XObj *h, const SampleFmt &fmt, const char *who)
{
    if (fmt.kind != SAMPLE_F32 && !sint_bytes(fmt.kind))
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": unknown sample kind (PSDC_SAMPLE_S16 or PSDC_SAMPLE_S8)");
    if (!std::isfinite(fmt.scale))
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": the scale is not finite");
    return PSDC_OK;
}

// the sample pointers of a psdc_sint_* call: none null, each aligned to the integer
int check_int_ptrs(XObj *h, const void *const *x, const SampleFmt &fmt, const char *who)
{
    for (uint32_t c = 0; c < h->m; ++c) {
        if (!x || !x[c])
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null sample pointer");
        if ((uintptr_t)x[c] % fmt.bytes())
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": the samples are not aligned to " + std::to_string(fmt.bytes()) + " bytes");
    }
    return PSDC_OK;
}

// the converter of one piece of an integer call: cnt integers of each of the m channels at src[c], written where the f32 call's
// copies write (sample_int.h, sample_cvt_int_kernel) -- ONE launch for the m channels, whose stream buffers share their phase
int convert_piece(XObj *h, XStage *s, const void *const *src, const SampleFmt &fmt, size_t at, size_t cnt, hipStream_t stream)
{
    SintCvtJob job{};
    for (uint32_t c = 0; c < h->m; ++c) {
        job.src[c] = src[c];
        job.dst[c] = s->buf.p[c][s->buf.cur] + at;
    }
    job.nch = h->m;
    job.len = cnt;
    job.scale = fmt.scale;
    XCHK(h, launch_cvt_int(job, fmt.kind, stream));
    ++h->launches;
    return PSDC_OK;
}

// the checks the two feeds of the objects without a mixer begin with; *go: there are samples to take
int plain_args(XObj *h, uint32_t pair, const void *const *x, const SampleFmt &fmt, size_t len, const char *who, bool *go)
{
    *go = false;
    X_HANDLE(h, who);
    const bool ints = fmt.kind != SAMPLE_F32;
    int rc = check_pair(h, pair, ints ? who : nullptr);
    if (rc)
        return rc;
    if (ints && (rc = check_fmt(h, fmt, who)))
        return rc;
    if (len == 0)
        return PSDC_OK;
    if (ints) {
        if ((rc = check_int_ptrs(h, x, fmt, who)))
            return rc;
    } else {
        for (uint32_t c = 0; c < h->m; ++c)
            if (!x || !x[c])
                return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null sample pointer");
    }
    *go = true;
    return PSDC_OK;
}

// x: h->m pointers (host memory).  fmt: f32 (psdc_cross_process, psdc_csm_process), or integers (psdc_sint_*): the raw integers
// go up into the landing lanes and one converter a piece writes the bytes the f32 call's uploads write.
int process_impl(XObj *h, uint32_t pair, const void *const *x, SampleFmt fmt, size_t len, const char *who)
{
    bool go = false;
    int rc = plain_args(h, pair, x, fmt, len, who, &go);
    if (rc || !go)
        return rc;
    const bool ints = fmt.kind != SAMPLE_F32;
    X_ON_DEVICE(h);
    if (ints && !h->d_land)
        XCHK(h, hipMalloc(&h->d_land, sizeof(float) * h->lanes() * STAGING));
    XStage *s = nullptr;
    if ((rc = stage0_room(h, pair, len, &s)))
        return rc;
    const size_t unit = fmt.bytes();
    for (size_t done = 0; done < len;) {
        const size_t cnt = std::min(STAGING, len - done);
        const size_t at = (size_t)(s->total + done - s->buf.base);
        Lane up[CSM_MAX_M];
        const void *from[CSM_MAX_M] = {};
        for (uint32_t c = 0; c < h->m; ++c) {
            float *land = ints ? h->d_land + c * STAGING : nullptr;
            from[c] = land;
            up[c] = {static_cast<const uint8_t *>(x[c]) + unit * done, unit * cnt, c * STAGING, ints ? land : s->buf.p[c][s->buf.cur] + at};
        }
        if ((rc = stage_upload(h, h->stream, up, h->m)))
            return rc;
        // (the next piece's uploads into the landing lanes run behind the converter: one stream)
        if (ints && (rc = convert_piece(h, s, from, fmt, at, cnt, h->stream)))
            return rc;
        done += cnt;
    }
    s->total += len;
    h->pairs_in += len;
    h->idle = false;
    bool did = false;
    return run_round(h, &did);
}

// d_x: h->m device pointers (the array itself is host memory).  fmt as in process_impl: an integer call has ONE converter launch
// where the f32 call has its m copies.
int process_device_impl(XObj *h, uint32_t pair, const void *const *d_x, SampleFmt fmt, size_t len, void *producer_event, const char *who)
{
    bool go = false;
    int rc = plain_args(h, pair, d_x, fmt, len, who, &go);
    if (rc || !go)
        return rc;
    X_ON_DEVICE(h);
    XStage *s = nullptr;
    h->grew = false;
    if ((rc = stage0_room(h, pair, len, &s)) || (rc = feed_open(h, producer_event)))
        return rc;
    const size_t at = (size_t)(s->total - s->buf.base);
    if (fmt.kind != SAMPLE_F32) {
        if ((rc = convert_piece(h, s, d_x, fmt, at, len, h->copy_stream)))
            return rc;
    } else {
        for (uint32_t c = 0; c < h->m; ++c)
            XCHK(h, hipMemcpyAsync(s->buf.p[c][s->buf.cur] + at, d_x[c], sizeof(float) * len, hipMemcpyDeviceToDevice, h->copy_stream));
    }
    s->total += len;
    h->pairs_in += len;
    return feed_close(h);
}

// The sources of a mixer feed: src[c] (NULL: none) starts in staging / landing lane c, and `unit` bytes of it are one stream sample.
//   zoom (reals() real channels): src[0 .. reals() - 1], unit = one number
//   IQ planar: src[0] = I, src[1] = Q, unit = 4;  IQ interleaved: src[0] = the (re, im) pairs, unit = two numbers
//   IQ pair planar: src[0 .. 3] = I_a, Q_a, I_b, Q_b;  interleaved: src[0], src[2] = the pairs of side a, b (over lanes 0-1, 2-3)
struct MixSrc {
    const void *src[CSM_MAX_M];
    size_t unit;
};

// A mixer-fronted unit takes len samples of each source, from host memory (up through the pinned staging into the landing buffer,
// pieces of STAGING samples) or from device memory (one piece).  mix(from, dst, j0, cnt) launches the family's mixer(s) for one
// piece on the copy stream: cnt samples of source c at from[c], to the unit's stream c at dst[c]; the first is stream sample j0
// (the samples the unit has taken since create or reset).
template <class Mix>
int mixer_feed(XObj *h, uint32_t unit, size_t len, bool dev, void *producer_event, const MixSrc &in, Mix mix)
{
    X_ON_DEVICE(h);
    if (!dev && !h->d_land)
        XCHK(h, hipMalloc(&h->d_land, sizeof(float) * h->lanes() * STAGING));
    XStage *s = nullptr;
    h->grew = false;
    int rc = stage0_room(h, unit, len, &s);
    if (rc || (rc = feed_open(h, producer_event)))
        return rc;
    const size_t piece = dev ? len : STAGING;
    for (size_t done = 0; done < len;) {
        const size_t cnt = std::min(piece, len - done);
        const void *from[CSM_MAX_M] = {};
        Lane up[CSM_MAX_M];
        uint32_t n_up = 0;
        for (uint32_t c = 0; c < CSM_MAX_M; ++c) {
            if (!in.src[c])
                continue;
            from[c] = static_cast<const uint8_t *>(in.src[c]) + in.unit * done;
            if (!dev) { // through lane c of the slot into lane c of the landing buffer, which the mixer then reads
                up[n_up++] = {from[c], in.unit * cnt, c * STAGING, h->d_land + c * STAGING};
                from[c] = h->d_land + c * STAGING;
            }
        }
        if (!dev && (rc = stage_upload(h, h->copy_stream, up, n_up)))
            return rc;
        float *dst[CSM_MAX_M] = {};
        for (uint32_t c = 0; c < h->m; ++c)
            dst[c] = s->buf.p[c][s->buf.cur] + (size_t)(s->total + done - s->buf.base);
        if ((rc = mix(from, dst, s->total + done, cnt)))
            return rc;
        done += cnt;
    }
    s->total += len;
    h->pairs_in += len;
    return feed_close(h);
}

// the checks every mixer feed begins with; *go: there are samples to take
int mixer_args(XObj *h, uint32_t unit, const SampleFmt &fmt, size_t len, const char *who, bool *go)
{
    *go = false;
    X_HANDLE(h, who);
    int rc = check_pair(h, unit, fmt.kind == SAMPLE_F32 ? nullptr : who);
    if (rc)
        return rc;
    if ((rc = check_fmt(h, fmt, who)))
        return rc;
    *go = len != 0;
    return PSDC_OK;
}

// A zoom unit: len real samples of each of its reals() channels (xs: that many pointers), f32 or integers; one mixer a channel.
int zoom_feed(XObj *h, uint32_t ch, const void *const *xs, SampleFmt fmt, size_t len, bool dev, void *producer_event, const char *who)
{
    bool go = false;
    int rc = mixer_args(h, ch, fmt, len, who, &go);
    if (rc || !go)
        return rc;
    const uint32_t nx = h->reals();
    MixSrc in{{}, fmt.bytes()};
    for (uint32_t c = 0; c < nx; ++c) {
        if (!xs[c])
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null sample pointer");
        if ((uintptr_t)xs[c] % in.unit)
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": the samples are not aligned to " + std::to_string(in.unit) + " bytes");
        in.src[c] = xs[c];
    }
    return mixer_feed(h, ch, len, dev, producer_event, in, [&](const void *const *from, float *const *dst, uint64_t j0, size_t cnt) -> int {
        for (uint32_t c = 0; c < nx; ++c) {
            const uint64_t ftw = h->ftw[(size_t)nx * ch + c], phase0 = h->phase0[(size_t)nx * ch + c];
            if (fmt.kind == SAMPLE_F32) {
                const ZoomMixJob mj{static_cast<const float *>(from[c]), dst[2 * c], dst[2 * c + 1], cnt, j0, ftw, phase0};
                XCHK(h, launch_zoom_mix(mj, h->copy_stream));
            } else {
                const SintMixJob mj{from[c], dst[2 * c], dst[2 * c + 1], cnt, j0, ftw, phase0, fmt.scale};
                XCHK(h, launch_zoom_mix_int(mj, fmt.kind, h->copy_stream));
            }
            ++h->launches;
        }
        return PSDC_OK;
    });
}

// the pointers of a complex feed: planar (every one of the n f32 streams 4-byte aligned) or interleaved ((re, im) pairs at the
// even ones, aligned to a pair; integers are always interleaved)
int check_iq_ptrs(XObj *h, const void *const *src, uint32_t n, bool interleaved, size_t unit, const char *who)
{
    for (uint32_t c = 0; c < n; c += interleaved ? 2 : 1) {
        if (!src[c])
            return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null sample pointer");
        if ((uintptr_t)src[c] % unit != 0)
            return xfail(h, PSDC_ERR_ARG, std::string(who) + (interleaved ? ": the (re, im) pairs are not aligned to " + std::to_string(unit) + " bytes"
                                                                          : std::string(": the samples are not aligned to 4 bytes")));
    }
    return PSDC_OK;
}

// An IQ channel: len complex samples, planar (src_q != NULL) or interleaved (src_q == NULL: src_i points to the pairs); one mixer.
int iq_feed(XObj *h, uint32_t ch, const void *src_i, const float *src_q, bool interleaved, SampleFmt fmt, size_t len, bool dev,
            void *producer_event, const char *who)
{
    bool go = false;
    int rc = mixer_args(h, ch, fmt, len, who, &go);
    if (rc || !go)
        return rc;
    const MixSrc in{{src_i, interleaved ? nullptr : src_q}, (interleaved ? 2 : 1) * fmt.bytes()};
    if (!src_i || (!interleaved && !src_q))
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null sample pointer");
    if ((rc = check_iq_ptrs(h, in.src, 2, interleaved, in.unit, who)))
        return rc;
    return mixer_feed(h, ch, len, dev, producer_event, in, [&](const void *const *from, float *const *dst, uint64_t j0, size_t cnt) -> int {
        if (fmt.kind == SAMPLE_F32) {
            const IqMixJob mj{static_cast<const float *>(from[0]), static_cast<const float *>(from[1]), dst[0], dst[1], cnt, j0, h->ftw[ch],
                              h->phase0[ch]};
            XCHK(h, launch_iq_mix(mj, interleaved, h->copy_stream));
        } else {
            const SintMixJob mj{from[0], dst[0], dst[1], cnt, j0, h->ftw[ch], h->phase0[ch], fmt.scale};
            XCHK(h, launch_iq_mix_int(mj, fmt.kind, h->copy_stream));
        }
        ++h->launches;
        return PSDC_OK;
    });
}

// An IQ cross pair: len complex samples of each side, planar (src: I_a, Q_a, I_b, Q_b) or interleaved (src[0], src[2]: the pairs
// of side a and side b; src[1], src[3] unused); ONE mixer launch a piece for both sides.
int iq_pair_feed(XObj *h, uint32_t pair, const void *const (&src)[4], bool interleaved, SampleFmt fmt, size_t len, bool dev,
                 void *producer_event, const char *who)
{
    bool go = false;
    int rc = mixer_args(h, pair, fmt, len, who, &go);
    if (rc || !go)
        return rc;
    MixSrc in{{}, (interleaved ? 2 : 1) * fmt.bytes()};
    if ((rc = check_iq_ptrs(h, src, 4, interleaved, in.unit, who)))
        return rc;
    for (int c = 0; c < 4; c += interleaved ? 2 : 1)
        in.src[c] = src[c];
    return mixer_feed(h, pair, len, dev, producer_event, in, [&](const void *const *from, float *const *dst, uint64_t j0, size_t cnt) -> int {
        IqPairMixJob mj{};
        SintPairMixJob ij{};
        for (int c = 0; c < 4; ++c) {
            mj.src[c] = static_cast<const float *>(from[c]);
            mj.dst[c] = ij.dst[c] = dst[c];
        }
        mj.len = ij.len = cnt;
        mj.j0 = ij.j0 = j0;
        ij.scale = fmt.scale;
        for (int side = 0; side < 2; ++side) {
            ij.src[side] = from[2 * side];
            mj.ftw[side] = ij.ftw[side] = h->ftw[2 * (size_t)pair + side];
            mj.phase0[side] = ij.phase0[side] = h->phase0[2 * (size_t)pair + side];
        }
        XCHK(h, fmt.kind == SAMPLE_F32 ? launch_iq_pair_mix(mj, interleaved, h->copy_stream) : launch_iq_pair_mix_int(ij, fmt.kind, h->copy_stream));
        ++h->launches;
        return PSDC_OK;
    });
}

int sync_impl(XObj *h, const char *who)
{
    X_HANDLE(h, who);
    X_ON_DEVICE(h);
    int rc = drain(h);
    if (rc)
        return rc;
    return sync_all(h);
}

int num_stages_impl(XObj *h, uint32_t pair, const char *who)
{
    X_HANDLE(h, who);
    int rc = check_pair(h, pair);
    if (rc)
        return rc;
    X_ON_DEVICE(h);
    if ((rc = drain(h)))
        return rc;
    return (int)h->pairs[pair].size();
}

// ---- the host read-outs of a unit --------------------------------------------------------------------------------------------
// Every one is built from the five pieces below.  A stage read-out is drained_stage and stage_rows: the stage's f64 accumulators,
// row by row, to where the call wants them.  A stitched read-out is unit_stitch: it drains, waits and takes ONE snapshot of the unit
// (UnitSnap: counts, averages, pendings and, with one copy a stage, the f64 accumulators), casts the leading rows to f32 and hands
// them to the row stitch of PsdCascade::psd (stitch_rows_impl), which also writes the f32 outputs; the capacity checks, len,
// n_breaks and the Breaks are written in one place.  What a family computes in f64 from the bins that stitch took (SK, the
// sidebands) is an expression on Stitched::each_bin.  The bank read-outs (psdcxr_*) take the snapshot's bookkeeping alone.

// a drained stage of a unit (the caller has checked the handle and the unit and is on the device)
int drained_stage(XObj *h, uint32_t unit, uint32_t stage, const XStage **out, const char *who)
{
    int rc = drain(h);
    if (rc)
        return rc;
    const auto &st = h->pairs[unit];
    if (stage >= st.size())
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": stage " + std::to_string(stage) + " out of range (" +
                                          std::to_string(st.size()) + " stages)");
    *out = &st[stage];
    return PSDC_OK;
}

// one stage's statistics and, with acc != NULL, its rows() x bins accumulators as they lie on the device
int stage_impl(XObj *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, std::vector<double> *acc, const char *who)
{
    X_HANDLE(h, who);
    int rc = check_pair(h, pair);
    if (rc)
        return rc;
    X_ON_DEVICE(h);
    const XStage *sp = nullptr;
    if ((rc = drained_stage(h, pair, stage, &sp, who)))
        return rc;
    const XStage &s = *sp;
    if (stat) {
        const uint32_t c = count_report(s.count64);
        stat->count = c;
        stat->avg = cur_avg(h, stage);
        stat->pending = pending_for(h->geo, s.total);
        stat->processed = (uint64_t)h->n * c - (uint64_t)h->geo.overlap * (c ? c - 1 : 0);
    }
    if (acc) {
        if ((rc = sync_all(h)))
            return rc;
        acc->resize(h->rows() * bins(h));
        XCHK(h, hipMemcpy(acc->data(), s.acc, sizeof(double) * acc->size(), hipMemcpyDeviceToHost));
    }
    return PSDC_OK;
}

// where a row of a read-out goes: element k to p[k * step]; p == NULL: the row is not wanted.  The re and im rows of a complex
// output are the two halves of one interleaved array (re_of, im_of)
template <class T>
struct RowOut {
    T *p = nullptr;
    size_t step = 1;
};
template <class T>
RowOut<T> re_of(T *z) { return {z, 2}; }
template <class T>
RowOut<T> im_of(T *z) { return {z ? z + 1 : nullptr, 2}; }
template <class T>
void put_row(const RowOut<T> &o, const T *src, size_t len)
{
    for (size_t k = 0; o.p && k < len; ++k)
        o.p[k * o.step] = src[k];
}
constexpr uint32_t X_MAX_ROWS = 16; // rows a stage has at most: CSM_MAX_M^2 (the AM/PM cross kinds: ZXAMPM_ROWS = 12)
static_assert(CSM_MAX_M * CSM_MAX_M <= X_MAX_ROWS && ZXAMPM_ROWS <= X_MAX_ROWS, "RowOut tables hold every row of a stage");
// nrows rows one behind the other, `stride` elements apart (rows == NULL: none is wanted)
template <class T>
void block_rows(T *rows, uint32_t nrows, size_t stride, RowOut<T> *outs)
{
    for (uint32_t r = 0; r < nrows; ++r)
        outs[r] = {rows ? rows + (size_t)r * stride : nullptr, 1};
}

// the rows of one stage, each to where outs[r] says (T: float, cast from the f64 accumulators, or double); beside its statistics
template <class T>
int stage_rows(XObj *h, uint32_t unit, uint32_t stage, psdc_stage_stat *stat, const RowOut<T> *outs, uint32_t nrows, const char *who)
{
    std::vector<double> acc;
    const bool any = std::any_of(outs, outs + nrows, [](const RowOut<T> &o) { return o.p != nullptr; });
    int rc = stage_impl(h, unit, stage, stat, any ? &acc : nullptr, who);
    if (rc || acc.empty())
        return rc;
    const size_t b = bins(h);
    for (uint32_t r = 0; r < nrows; ++r)
        for (size_t k = 0; outs[r].p && k < b; ++k)
            outs[r].p[k * outs[r].step] = (T)acc[r * b + k];
    return PSDC_OK;
}
// ... with every row of the stage one behind the other in `rows`
template <class T>
int stage_block(XObj *h, uint32_t unit, uint32_t stage, psdc_stage_stat *stat, T *rows, const char *who)
{
    RowOut<T> outs[X_MAX_ROWS];
    const uint32_t nrows = h ? h->rows() : 0;
    block_rows(rows, nrows, h ? bins(h) : 0, outs);
    return stage_rows(h, unit, stage, stat, outs, nrows, who);
}

// which stages and bins a stitch takes (PsdCascade::psd's arguments), and where a stitched read-out puts what every one has
struct StitchSel {
    int keep_overlap;
    uint32_t min_count;
    int keep_transition_band;
};
struct StitchOut {
    size_t cap; // elements every output row has room for
    size_t *len;
    psdc_break *breaks;
    size_t breaks_cap;
    size_t *n_breaks;
};

// A drained unit as a stitch sees it: of every stage the count, the average and the pending samples and, where they were asked
// for, the f64 accumulators as they lie on the device (ns x rows() x bins)
struct UnitSnap {
    uint32_t ns = 0;
    size_t bins = 0, stage_elems = 0; // (rows() x bins)
    std::vector<uint64_t> c64, pend;
    std::vector<uint32_t> avgs;
    std::unique_ptr<double[]> acc; // (not a vector: every element is copied over, none needs a zero first)
    const double *stage(size_t i) const { return acc.get() + i * stage_elems; }
    // the first nlead rows of every stage in f32, as the row stitch takes them (ns x nlead x bins)
    std::unique_ptr<float[]> lead(uint32_t nlead) const
    {
        std::unique_ptr<float[]> rows(new float[std::max<size_t>(1, (size_t)ns * nlead * bins)]);
        for (uint32_t i = 0; i < ns; ++i)
            for (size_t k = 0; k < nlead * bins; ++k)
                rows[(size_t)i * nlead * bins + k] = (float)stage(i)[k];
        return rows;
    }
};

// the bookkeeping of a unit (the caller has drained; no device call)
void unit_layout(const XObj *h, uint32_t unit, UnitSnap *in)
{
    const auto &st = h->pairs[unit];
    const uint32_t ns = (uint32_t)st.size();
    in->ns = ns;
    in->bins = bins(h);
    in->stage_elems = h->rows() * in->bins;
    in->c64.resize(std::max<uint32_t>(ns, 1));
    in->pend.resize(std::max<uint32_t>(ns, 1));
    in->avgs.resize(std::max<uint32_t>(ns, 1));
    for (uint32_t i = 0; i < ns; ++i) {
        in->c64[i] = st[i].count64;
        in->pend[i] = pending_for(h->geo, st[i].total);
        in->avgs[i] = cur_avg(h, i);
    }
}

// drain, wait, and the unit with its accumulators: one copy a stage
int unit_snap(XObj *h, uint32_t unit, UnitSnap *in)
{
    int rc;
    if ((rc = drain(h)) || (rc = sync_all(h)))
        return rc;
    unit_layout(h, unit, in);
    in->acc.reset(new double[std::max<size_t>(1, in->ns * in->stage_elems)]);
    for (uint32_t i = 0; i < in->ns; ++i)
        XCHK(h, hipMemcpy(in->acc.get() + i * in->stage_elems, h->pairs[unit][i].acc, sizeof(double) * in->stage_elems, hipMemcpyDeviceToHost));
    return PSDC_OK;
}

// psdc_stitch_window on each of `nrows` rows of caller stages (n_stages x nrows x (n/2+1)) into outs[r] (a row that is not wanted
// still has its length computed; a row with a step is stitched aside and spread out once every row has come); Breaks from row 0
int stitch_rows_impl(const char *who, uint32_t n, float power, float nenbw, size_t overlap, uint32_t n_stages, const uint64_t *counts64,
                     const uint32_t *avgs, const uint64_t *pendings, const float *rows, uint32_t nrows, const StitchSel &sel,
                     const RowOut<float> *outs, const StitchOut &o)
{
    if (n < 2 || overlap >= n || n_stages > 20 || nrows > X_MAX_ROWS)
        return xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": bad arguments");
    if (n_stages && (!counts64 || !avgs || !pendings || !rows))
        return xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": null input");
    const size_t b = n / 2 + 1;
    std::vector<float> sp(std::max<size_t>(1, (size_t)n_stages * b));
    float *dst[X_MAX_ROWS];
    size_t aside = 0;
    for (uint32_t r = 0; r < nrows; ++r)
        aside += outs[r].p && outs[r].step != 1;
    std::vector<float> tmp(std::max<size_t>(1, aside * o.cap));
    for (uint32_t r = 0, t = 0; r < nrows; ++r)
        dst[r] = !outs[r].p ? nullptr : outs[r].step == 1 ? outs[r].p : &tmp[t++ * o.cap];
    size_t plen = 0;
    bool any = false;
    for (uint32_t r = 0; r < nrows; ++r) {
        for (uint32_t i = 0; i < n_stages; ++i)
            memcpy(&sp[(size_t)i * b], rows + ((size_t)i * nrows + r) * b, sizeof(float) * b);
        any = any || dst[r];
        size_t l = 0, nb = 0;
        int rc = psdc_stitch_window(n, power, nenbw, overlap, n_stages, counts64, avgs, pendings, sp.data(), sel.keep_overlap,
                                    sel.min_count, sel.keep_transition_band, dst[r], dst[r] ? o.cap : 0, &l, r == 0 ? o.breaks : nullptr,
                                    r == 0 ? o.breaks_cap : 0, &nb);
        if (rc == PSDC_ERR_CAPACITY)
            return xfail(nullptr, rc, std::string(who) + ": output too small");
        if (rc)
            return xfail(nullptr, rc, std::string(who) + ": " + psdc_last_error(nullptr));
        if (r == 0) {
            plen = l;
            if (o.n_breaks)
                *o.n_breaks = nb;
            if (o.breaks && nb > o.breaks_cap)
                return xfail(nullptr, PSDC_ERR_CAPACITY, std::string(who) + ": breaks output too small");
        }
    }
    if (any && plen > o.cap)
        return xfail(nullptr, PSDC_ERR_CAPACITY, std::string(who) + ": output too small");
    for (uint32_t r = 0; r < nrows; ++r)
        if (dst[r] && dst[r] != outs[r].p)
            put_row(outs[r], dst[r], plen);
    if (o.len)
        *o.len = plen;
    return PSDC_OK;
}

// what unit_stitch leaves for a caller that goes on: the unit, and the length and the Breaks of its stitch
struct Stitched {
    UnitSnap snap;
    psdc_break br[X_MAX_STAGES];
    size_t len = 0, nb = 0;
    // f(stage, bin, out, Break) for every bin the stitch took: bin `bin` of stage `stage` is element `out` of an output row
    template <class F>
    void each_bin(F f) const
    {
        for (size_t i = 0; i < nb; ++i) { // Break i is stage ns - 1 - i (lowest rate first)
            if (!br[i].include)
                continue;
            for (uint64_t k = br[i].bins_start; k < br[i].bins_end; ++k)
                f(snap.ns - 1 - i, (size_t)k, (size_t)(br[i].start + (k - br[i].bins_start)), br[i]);
        }
    }
};

// Who keeps the Breaks while the rows are stitched.  The two answer a too small breaks_cap differently, and each family's answer
// is kept as it was (tests/golden/cross_read_dump.bin holds both):
//   CALLER  the families whose every row is an f32 output (pair, matrix, zoom, IQ and their cross forms) hand the caller's array to
//           the stitch: it is filled up to breaks_cap, row 0 alone is written, len and n_breaks are not, and the text is
//           "<stitch_who>: output too small";
//   OWN     the families that go on in f64 (SK, zoom / IQ SK, AM/PM and AM/PM cross) stitch into Stitched::br: every row, len and
//           n_breaks are written, no Break is, and the text is "<who>: breaks output too small".
enum class BreaksOf { CALLER, OWN };

// The stitched read-out of a unit: the checks of the handle, the unit and the device, the snapshot, the f32 stitch of the unit's
// first nlead rows into outs, then the capacity checks, len, n_breaks and the Breaks.  more: the caller has further outputs of `cap`
// elements to fill (from st).  stitch_who: the name the row stitch gives its errors.
int unit_stitch(XObj *h, uint32_t unit, const StitchSel &sel, uint32_t nlead, const RowOut<float> *outs, bool more, const StitchOut &o,
                BreaksOf breaks_of, const char *stitch_who, const char *who, Stitched *st)
{
    X_HANDLE(h, who);
    int rc = check_pair(h, unit);
    if (rc)
        return rc;
    X_ON_DEVICE(h);
    if ((rc = unit_snap(h, unit, &st->snap)))
        return rc;
    const UnitSnap &in = st->snap;
    const bool own = breaks_of == BreaksOf::OWN;
    const StitchOut so = own ? StitchOut{o.cap, &st->len, st->br, X_MAX_STAGES, &st->nb} : StitchOut{o.cap, &st->len, o.breaks, o.breaks_cap, o.n_breaks};
    rc = stitch_rows_impl(stitch_who, h->n, h->power, h->nenbw, h->geo.overlap, in.ns, in.c64.data(), in.avgs.data(), in.pend.data(),
                          in.lead(nlead).get(), nlead, sel, outs, so);
    if (rc)
        return xfail(h, rc, x_last_error);
    if (own && more && st->len > o.cap)
        return xfail(h, PSDC_ERR_CAPACITY, std::string(who) + ": output too small");
    if (o.len)
        *o.len = st->len;
    if (!own)
        return PSDC_OK;
    if (o.n_breaks)
        *o.n_breaks = st->nb;
    if (o.breaks) {
        if (st->nb > o.breaks_cap)
            return xfail(h, PSDC_ERR_CAPACITY, std::string(who) + ": breaks output too small");
        std::copy(st->br, st->br + st->nb, o.breaks);
    }
    return PSDC_OK;
}

// ... of a family whose every row is an f32 output: all nrows = rows() of them
int unit_stitch_rows(XObj *h, uint32_t unit, const StitchSel &sel, const RowOut<float> *outs, uint32_t nrows, const StitchOut &o,
                     const char *stitch_who, const char *who)
{
    Stitched st;
    return unit_stitch(h, unit, sel, nrows, outs, false, o, BreaksOf::CALLER, stitch_who, who, &st);
}

int stats_impl(XObj *h, uint64_t *launches, uint64_t *in, int reset, const char *who)
{
    X_HANDLE(h, who);
    if (launches)
        *launches = h->launches;
    if (in)
        *in = h->pairs_in;
    if (reset)
        h->launches = h->pairs_in = 0;
    return PSDC_OK;
}

int frames_host_impl(XObj *h, const uint32_t *map, const uint8_t *frames, size_t frame_size, size_t n_frames, size_t *n_ok,
                     const char *who)
{
    size_t good = 0;
    psdrt::StoreOk store_ok{n_ok, good};
    X_HANDLE(h, who);
    std::vector<FedPair> fed;
    bool go = false;
    int rc = frames_args(h, map, frames, frame_size, n_frames, who, &fed, &go);
    if (rc || !go)
        return rc;
    X_ON_DEVICE(h);
    FrameSrc src;
    src.host = frames;
    src.hdr = {frames, frame_size};
    return ingest_frames(h, fed, src, frame_size, n_frames, &good, who);
}

int frames_device_impl(XObj *h, const uint32_t *map, const uint8_t *d_frames, size_t frame_size, size_t n_frames, size_t *n_ok,
                       void *producer_event, const char *who)
{
    size_t good = 0;
    psdrt::StoreOk store_ok{n_ok, good};
    X_HANDLE(h, who);
    std::vector<FedPair> fed;
    bool go = false;
    int rc = frames_args(h, map, d_frames, frame_size, n_frames, who, &fed, &go);
    if (rc || !go)
        return rc;
    X_ON_DEVICE(h);
    // the headers come to the host through one gather launch on a stream of the object's own (behind the producer's event, as the
    // copy stream's decodes are); the host waits for that launch alone while the compute stream goes on with the rounds of
    // earlier calls
    if (producer_event) {
        XCHK(h, h->hdr.open());
        XCHK(h, hipStreamWaitEvent(h->hdr.stream, (hipEvent_t)producer_event, 0));
        XCHK(h, hipStreamWaitEvent(h->copy_stream, (hipEvent_t)producer_event, 0));
    }
    XCHK(h, h->hdr.launch(d_frames, frame_size, n_frames));
    ++h->launches;
    XCHK(h, hipStreamSynchronize(h->hdr.stream));
    FrameSrc src;
    src.dev = d_frames;
    src.hdr = {h->hdr.h_hdr, 8};
    return ingest_frames(h, fed, src, frame_size, n_frames, &good, who);
}

// the carrier of a channel of a one-channel-a-unit object (psdc_zoom, psdc_iq)
int set_carrier_impl(XObj *h, uint32_t channel, uint64_t ftw, uint64_t phase0, const char *who)
{
    X_HANDLE(h, who);
    int rc = check_pair(h, channel);
    if (rc)
        return rc;
    const auto &st = h->pairs[channel];
    if (!st.empty() && st[0].total)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": channel " + std::to_string(channel) + " has taken " +
                                          std::to_string(st[0].total) + " samples: a carrier is set before the first one (or after a reset)");
    h->ftw[channel] = ftw;
    h->phase0[channel] = phase0;
    return PSDC_OK;
}

// the two rows of one stage / the stitched two rows of a channel (psdc_zoom, psdc_iq)
int two_rows_stage_impl(XObj *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, float *upper, float *lower, const char *who)
{
    const RowOut<float> outs[2] = {{upper}, {lower}};
    return stage_rows(h, channel, stage, stat, outs, 2, who);
}

int two_rows_psd_impl(XObj *h, uint32_t channel, const StitchSel &sel, float *upper, float *lower, const StitchOut &o, const char *who)
{
    const RowOut<float> outs[2] = {{upper}, {lower}};
    return unit_stitch_rows(h, channel, sel, outs, 2, o, who, who);
}

// the carrier of one side of a pair of a two-channels-a-unit object (psdc_zcsd, psdc_iqcsd)
int pair_carrier_impl(XObj *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0, const char *who)
{
    X_HANDLE(h, who);
    int rc = check_pair(h, pair);
    if (rc)
        return rc;
    if (side > 1)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": side " + std::to_string(side) + " out of range (0: channel a, 1: channel b)");
    const auto &st = h->pairs[pair];
    if (!st.empty() && st[0].total)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": pair " + std::to_string(pair) + " has taken " +
                                          std::to_string(st[0].total) + " samples: a carrier is set before the first one (or after a reset)");
    h->ftw[2 * (size_t)pair + side] = ftw;
    h->phase0[2 * (size_t)pair + side] = phase0;
    return PSDC_OK;
}

// the stitched rows of a pair (psdc_zcsd, psdc_iqcsd): the complex rows are stitched as their real and imaginary rows, as
// psdc_cross_stitch does
int eight_rows_csd_impl(XObj *h, uint32_t pair, const StitchSel &sel, float *saa_upper, float *saa_lower, float *sbb_upper, float *sbb_lower,
                        float *sab_upper, float *sab_lower, const StitchOut &o, const char *who)
{
    const RowOut<float> outs[8] = {{saa_upper}, {saa_lower}, {sbb_upper}, {sbb_lower}, re_of(sab_upper), re_of(sab_lower), im_of(sab_upper), im_of(sab_lower)};
    return unit_stitch_rows(h, pair, sel, outs, 8, o, who, who);
}

int loss_impl(XObj *h, psdc_loss *out, int reset, const char *who)
{
    X_HANDLE(h, who);
    if (!out)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output");
    *out = h->loss;
    if (reset)
        h->loss = psdc_loss{};
    return PSDC_OK;
}

} // namespace

extern "C" {

// ---- pairs: m = 2 on cross_kernel, rows xx, yy, re, im ----

psdc_cross *psdc_cross_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                     int device)
{
    return static_cast<psdc_cross *>(create_impl(KINDS[K_CROSS], n, win, power, nenbw, overlap, n_pairs, device, "psdc_cross_create_window"));
}

psdc_cross *psdc_cross_create(uint32_t n, int window_kind, uint32_t n_pairs, int device)
{
    return static_cast<psdc_cross *>(create_kind(KINDS[K_CROSS], n, window_kind, n_pairs, device, "psdc_cross_create"));
}

void psdc_cross_destroy(psdc_cross *h) { destroy_obj(h); }

int psdc_cross_reset(psdc_cross *h) { return reset_impl(h, "psdc_cross_reset"); }
int psdc_cross_set_detrend(psdc_cross *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_cross_set_detrend"); }
int psdc_cross_set_avg(psdc_cross *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_cross_set_avg"); }

int psdc_cross_process(psdc_cross *h, uint32_t pair, const float *x, const float *y, size_t len)
{
    const void *xs[2] = {x, y};
    return process_impl(h, pair, xs, SampleFmt{}, len, "psdc_cross_process");
}

int psdc_cross_process_device(psdc_cross *h, uint32_t pair, const float *d_x, const float *d_y, size_t len,
                              void *producer_event)
{
    const void *xs[2] = {d_x, d_y};
    return process_device_impl(h, pair, xs, SampleFmt{}, len, producer_event, "psdc_cross_process_device");
}

int psdc_cross_sync(psdc_cross *h) { return sync_impl(h, "psdc_cross_sync"); }
int psdc_cross_num_stages(psdc_cross *h, uint32_t pair) { return num_stages_impl(h, pair, "psdc_cross_num_stages"); }

int psdc_cross_stage_spectra(psdc_cross *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, float *sxx, float *syy,
                             float *sxy)
{
    const RowOut<float> outs[4] = {{sxx}, {syy}, re_of(sxy), im_of(sxy)};
    return stage_rows(h, pair, stage, stat, outs, 4, "psdc_cross_stage_spectra");
}

int psdc_cross_stitch(uint32_t n, float power, float nenbw, size_t overlap, uint32_t n_stages, const uint64_t *counts64,
                      const uint32_t *avgs, const uint64_t *pendings, const float *rows, int keep_overlap, uint32_t min_count,
                      int keep_transition_band, float *sxx, float *syy, float *sxy, size_t cap, size_t *len,
                      psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    // the four rows of every stage as four spectra slabs, each stitched exactly as PsdCascade::psd
    const RowOut<float> outs[4] = {{sxx}, {syy}, re_of(sxy), im_of(sxy)};
    return stitch_rows_impl("psdc_cross_stitch", n, power, nenbw, overlap, n_stages, counts64, avgs, pendings, rows, 4,
                            {keep_overlap, min_count, keep_transition_band}, outs, {cap, len, breaks, breaks_cap, n_breaks});
}

int psdc_cross_csd(psdc_cross *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, float *sxx,
                   float *syy, float *sxy, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    const RowOut<float> outs[4] = {{sxx}, {syy}, re_of(sxy), im_of(sxy)};
    return unit_stitch_rows(h, pair, {keep_overlap, min_count, keep_transition_band}, outs, 4, {cap, len, breaks, breaks_cap, n_breaks},
                            "psdc_cross_stitch", "psdc_cross_csd");
}

int psdc_cross_stats_read(psdc_cross *h, uint64_t *launches, uint64_t *pairs_in, int reset)
{
    return stats_impl(h, launches, pairs_in, reset, "psdc_cross_stats_read");
}

int psdc_csd_process_frames(psdc_cross *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                            size_t *n_ok)
{
    return frames_host_impl(h, pair_traces, frames, frame_size, n_frames, n_ok, "psdc_csd_process_frames");
}

int psdc_csd_process_frames_device(psdc_cross *h, const uint32_t *pair_traces, const uint8_t *d_frames, size_t frame_size,
                                   size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, pair_traces, d_frames, frame_size, n_frames, n_ok, producer_event, "psdc_csd_process_frames_device");
}

int psdc_csd_loss_read(psdc_cross *h, psdc_loss *out, int reset) { return loss_impl(h, out, reset, "psdc_csd_loss_read"); }

const char *psdc_cross_last_error(const psdc_cross *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- groups of m channels: csm_kernel, the m * m rows of csm_fft.h ----

int psdc_csm_supported(uint32_t n, uint32_t m) { return n <= 4096 && m <= CSM_MAX_M && csm_supported((int)n, (int)m) ? 1 : 0; }

psdc_csm *psdc_csm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t m,
                                 uint32_t n_groups, int device)
{
    return static_cast<psdc_csm *>(create_impl(KINDS[K_CSM], n, win, power, nenbw, overlap, n_groups, device, "psdc_csm_create_window", m));
}

psdc_csm *psdc_csm_create(uint32_t n, int window_kind, uint32_t m, uint32_t n_groups, int device)
{
    return static_cast<psdc_csm *>(create_kind(KINDS[K_CSM], n, window_kind, n_groups, device, "psdc_csm_create", m));
}

void psdc_csm_destroy(psdc_csm *h) { destroy_obj(h); }

int psdc_csm_reset(psdc_csm *h) { return reset_impl(h, "psdc_csm_reset"); }
int psdc_csm_set_detrend(psdc_csm *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_csm_set_detrend"); }
int psdc_csm_set_avg(psdc_csm *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_csm_set_avg"); }

int psdc_csm_process(psdc_csm *h, uint32_t group, const float *const *x, size_t len)
{
    return process_impl(h, group, reinterpret_cast<const void *const *>(x), SampleFmt{}, len, "psdc_csm_process");
}

int psdc_csm_process_device(psdc_csm *h, uint32_t group, const float *const *d_x, size_t len, void *producer_event)
{
    return process_device_impl(h, group, reinterpret_cast<const void *const *>(d_x), SampleFmt{}, len, producer_event, "psdc_csm_process_device");
}

int psdc_csm_process_frames(psdc_csm *h, const uint32_t *group_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                            size_t *n_ok)
{
    return frames_host_impl(h, group_traces, frames, frame_size, n_frames, n_ok, "psdc_csm_process_frames");
}

int psdc_csm_process_frames_device(psdc_csm *h, const uint32_t *group_traces, const uint8_t *d_frames, size_t frame_size,
                                   size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, group_traces, d_frames, frame_size, n_frames, n_ok, producer_event, "psdc_csm_process_frames_device");
}

int psdc_csm_loss_read(psdc_csm *h, psdc_loss *out, int reset) { return loss_impl(h, out, reset, "psdc_csm_loss_read"); }
int psdc_csm_sync(psdc_csm *h) { return sync_impl(h, "psdc_csm_sync"); }
int psdc_csm_num_stages(psdc_csm *h, uint32_t group) { return num_stages_impl(h, group, "psdc_csm_num_stages"); }

int psdc_csm_stage_spectra(psdc_csm *h, uint32_t group, uint32_t stage, psdc_stage_stat *stat, float *rows)
{
    return stage_block(h, group, stage, stat, rows, "psdc_csm_stage_spectra");
}

int psdc_csm_stitch(uint32_t n, uint32_t m, float power, float nenbw, size_t overlap, uint32_t n_stages, const uint64_t *counts64,
                    const uint32_t *avgs, const uint64_t *pendings, const float *rows_in, int keep_overlap, uint32_t min_count,
                    int keep_transition_band, float *rows, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap,
                    size_t *n_breaks)
{
    if (m < 2 || m > CSM_MAX_M)
        return xfail(nullptr, PSDC_ERR_ARG, "psdc_csm_stitch: m must be 2, 3 or 4");
    RowOut<float> outs[X_MAX_ROWS];
    block_rows(rows, m * m, cap, outs);
    return stitch_rows_impl("psdc_csm_stitch", n, power, nenbw, overlap, n_stages, counts64, avgs, pendings, rows_in, m * m,
                            {keep_overlap, min_count, keep_transition_band}, outs, {cap, len, breaks, breaks_cap, n_breaks});
}

int psdc_csm_csd(psdc_csm *h, uint32_t group, int keep_overlap, uint32_t min_count, int keep_transition_band, float *rows,
                 size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    RowOut<float> outs[X_MAX_ROWS];
    const uint32_t nrows = h ? h->rows() : 0;
    block_rows(rows, nrows, cap, outs);
    return unit_stitch_rows(h, group, {keep_overlap, min_count, keep_transition_band}, outs, nrows, {cap, len, breaks, breaks_cap, n_breaks},
                            "psdc_csm_stitch", "psdc_csm_csd");
}

int psdc_csm_stats_read(psdc_csm *h, uint64_t *launches, uint64_t *sample_times_in, int reset)
{
    return stats_impl(h, launches, sample_times_in, reset, "psdc_csm_stats_read");
}

const char *psdc_csm_last_error(const psdc_csm *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- zoom: one real channel a unit, mixed to I and Q in front of stage 0; zoom_kernel, rows upper, lower ----

psdc_zoom *psdc_zoom_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                   int device)
{
    return static_cast<psdc_zoom *>(create_impl(KINDS[K_ZOOM], n, win, power, nenbw, overlap, n_channels, device, "psdc_zoom_create_window"));
}

psdc_zoom *psdc_zoom_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_zoom *>(create_kind(KINDS[K_ZOOM], n, window_kind, n_channels, device, "psdc_zoom_create"));
}

void psdc_zoom_destroy(psdc_zoom *h) { destroy_obj(h); }

int psdc_zoom_reset(psdc_zoom *h) { return reset_impl(h, "psdc_zoom_reset"); }
int psdc_zoom_set_detrend(psdc_zoom *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zoom_set_detrend"); }
int psdc_zoom_set_avg(psdc_zoom *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_zoom_set_avg"); }

int psdc_zoom_set_carrier(psdc_zoom *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_zoom_set_carrier");
}

int psdc_zoom_process(psdc_zoom *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, false, nullptr, "psdc_zoom_process");
}

int psdc_zoom_process_device(psdc_zoom *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, true, producer_event, "psdc_zoom_process_device");
}

int psdc_zoomcascade_process_frames(psdc_zoom *h, const uint32_t *channel_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                             size_t *n_ok)
{
    return frames_host_impl(h, channel_traces, frames, frame_size, n_frames, n_ok, "psdc_zoomcascade_process_frames");
}

int psdc_zoomcascade_process_frames_device(psdc_zoom *h, const uint32_t *channel_traces, const uint8_t *d_frames, size_t frame_size,
                                    size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, channel_traces, d_frames, frame_size, n_frames, n_ok, producer_event,
                              "psdc_zoomcascade_process_frames_device");
}

int psdc_zoomcascade_loss_read(psdc_zoom *h, psdc_loss *out, int reset) { return loss_impl(h, out, reset, "psdc_zoomcascade_loss_read"); }
int psdc_zoom_sync(psdc_zoom *h) { return sync_impl(h, "psdc_zoom_sync"); }
int psdc_zoom_num_stages(psdc_zoom *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_zoom_num_stages"); }

int psdc_zoom_stage_spectra(psdc_zoom *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, float *upper, float *lower)
{
    return two_rows_stage_impl(h, channel, stage, stat, upper, lower, "psdc_zoom_stage_spectra");
}

int psdc_zoom_psd(psdc_zoom *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                  float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return two_rows_psd_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower,
                             {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zoom_psd");
}

int psdc_zoom_stats_read(psdc_zoom *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_zoom_stats_read");
}

const char *psdc_zoom_last_error(const psdc_zoom *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- IQ: one complex channel a unit, its I and Q through the complex mixer in front of stage 0; everything behind is the zoom
// object's (zoom_kernel, rows upper, lower) ----

psdc_iq *psdc_iq_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_iq *>(create_impl(KINDS[K_IQ], n, win, power, nenbw, overlap, n_channels, device, "psdc_iq_create_window"));
}

psdc_iq *psdc_iq_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_iq *>(create_kind(KINDS[K_IQ], n, window_kind, n_channels, device, "psdc_iq_create"));
}

void psdc_iq_destroy(psdc_iq *h) { destroy_obj(h); }

int psdc_iq_reset(psdc_iq *h) { return reset_impl(h, "psdc_iq_reset"); }
int psdc_iq_set_detrend(psdc_iq *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_iq_set_detrend"); }
int psdc_iq_set_avg(psdc_iq *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_iq_set_avg"); }

int psdc_iq_set_carrier(psdc_iq *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_iq_set_carrier");
}

int psdc_iq_process(psdc_iq *h, uint32_t channel, const float *i, const float *q, size_t len)
{
    return iq_feed(h, channel, i, q, false, SampleFmt{}, len, false, nullptr, "psdc_iq_process");
}

int psdc_iq_process_device(psdc_iq *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_i, d_q, false, SampleFmt{}, len, true, producer_event, "psdc_iq_process_device");
}

int psdc_iq_process_interleaved(psdc_iq *h, uint32_t channel, const float *iq, size_t len)
{
    return iq_feed(h, channel, iq, nullptr, true, SampleFmt{}, len, false, nullptr, "psdc_iq_process_interleaved");
}

int psdc_iq_process_interleaved_device(psdc_iq *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_iq, nullptr, true, SampleFmt{}, len, true, producer_event, "psdc_iq_process_interleaved_device");
}

int psdc_iq_process_frames(psdc_iq *h, const uint32_t *channel_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                           size_t *n_ok)
{
    return frames_host_impl(h, channel_traces, frames, frame_size, n_frames, n_ok, "psdc_iq_process_frames");
}

int psdc_iq_process_frames_device(psdc_iq *h, const uint32_t *channel_traces, const uint8_t *d_frames, size_t frame_size,
                                  size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, channel_traces, d_frames, frame_size, n_frames, n_ok, producer_event,
                              "psdc_iq_process_frames_device");
}

int psdc_iq_loss_read(psdc_iq *h, psdc_loss *out, int reset) { return loss_impl(h, out, reset, "psdc_iq_loss_read"); }
int psdc_iq_sync(psdc_iq *h) { return sync_impl(h, "psdc_iq_sync"); }
int psdc_iq_num_stages(psdc_iq *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_iq_num_stages"); }

int psdc_iq_stage_spectra(psdc_iq *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, float *upper, float *lower)
{
    return two_rows_stage_impl(h, channel, stage, stat, upper, lower, "psdc_iq_stage_spectra");
}

int psdc_iq_psd(psdc_iq *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return two_rows_psd_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower,
                             {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iq_psd");
}

int psdc_iq_stats_read(psdc_iq *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_iq_stats_read");
}

const char *psdc_iq_last_error(const psdc_iq *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- zoom cross: two real channels a unit, each mixed to I and Q in front of stage 0; zoom_cross_kernel, the eight rows of
// zoom_cross_fft.h ----

int psdc_zcsd_supported(uint32_t n) { return n <= 4096 && zoom_cross_supported((int)n) ? 1 : 0; }

psdc_zcsd *psdc_zcsd_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                   int device)
{
    return static_cast<psdc_zcsd *>(create_impl(KINDS[K_ZCSD], n, win, power, nenbw, overlap, n_pairs, device, "psdc_zcsd_create_window"));
}

psdc_zcsd *psdc_zcsd_create(uint32_t n, int window_kind, uint32_t n_pairs, int device)
{
    return static_cast<psdc_zcsd *>(create_kind(KINDS[K_ZCSD], n, window_kind, n_pairs, device, "psdc_zcsd_create"));
}

void psdc_zcsd_destroy(psdc_zcsd *h) { destroy_obj(h); }

int psdc_zcsd_reset(psdc_zcsd *h) { return reset_impl(h, "psdc_zcsd_reset"); }
int psdc_zcsd_set_detrend(psdc_zcsd *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zcsd_set_detrend"); }
int psdc_zcsd_set_avg(psdc_zcsd *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_zcsd_set_avg"); }

int psdc_zcsd_set_carrier(psdc_zcsd *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0)
{
    return pair_carrier_impl(h, pair, side, ftw, phase0, "psdc_zcsd_set_carrier");
}

int psdc_zcsd_process(psdc_zcsd *h, uint32_t pair, const float *x, const float *y, size_t len)
{
    const void *xs[2] = {x, y};
    return zoom_feed(h, pair, xs, SampleFmt{}, len, false, nullptr, "psdc_zcsd_process");
}

int psdc_zcsd_process_device(psdc_zcsd *h, uint32_t pair, const float *d_x, const float *d_y, size_t len, void *producer_event)
{
    const void *xs[2] = {d_x, d_y};
    return zoom_feed(h, pair, xs, SampleFmt{}, len, true, producer_event, "psdc_zcsd_process_device");
}

int psdc_zcsd_sync(psdc_zcsd *h) { return sync_impl(h, "psdc_zcsd_sync"); }
int psdc_zcsd_num_stages(psdc_zcsd *h, uint32_t pair) { return num_stages_impl(h, pair, "psdc_zcsd_num_stages"); }

int psdc_zcsd_stage_spectra(psdc_zcsd *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, float *rows)
{
    return stage_block(h, pair, stage, stat, rows, "psdc_zcsd_stage_spectra");
}

int psdc_zcsd_csd(psdc_zcsd *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, float *saa_upper,
                  float *saa_lower, float *sbb_upper, float *sbb_lower, float *sab_upper, float *sab_lower, size_t cap, size_t *len,
                  psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return eight_rows_csd_impl(h, pair, {keep_overlap, min_count, keep_transition_band}, saa_upper, saa_lower, sbb_upper,
                               sbb_lower, sab_upper, sab_lower,
                               {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zcsd_csd");
}

int psdc_zcsd_stats_read(psdc_zcsd *h, uint64_t *launches, uint64_t *pairs_in, int reset)
{
    return stats_impl(h, launches, pairs_in, reset, "psdc_zcsd_stats_read");
}

// the frames calls of a zoom cross object (the prefix follows ZoomCsdCascade, as psdc_zoomcascade_ follows ZoomCascade)
int psdc_zoomcsdcascade_process_frames(psdc_zcsd *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size,
                                       size_t n_frames, size_t *n_ok)
{
    return frames_host_impl(h, pair_traces, frames, frame_size, n_frames, n_ok, "psdc_zoomcsdcascade_process_frames");
}

int psdc_zoomcsdcascade_process_frames_device(psdc_zcsd *h, const uint32_t *pair_traces, const uint8_t *d_frames, size_t frame_size,
                                              size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, pair_traces, d_frames, frame_size, n_frames, n_ok, producer_event,
                              "psdc_zoomcsdcascade_process_frames_device");
}

int psdc_zoomcsdcascade_loss_read(psdc_zcsd *h, psdc_loss *out, int reset)
{
    return loss_impl(h, out, reset, "psdc_zoomcsdcascade_loss_read");
}

const char *psdc_zcsd_last_error(const psdc_zcsd *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- IQ cross: two complex channels a unit, both turned by one pair mixer in front of stage 0; everything behind the mixer is
// the zoom cross object's ----

int psdc_iqcsd_supported(uint32_t n) { return psdc_zcsd_supported(n); }

psdc_iqcsd *psdc_iqcsd_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                     int device)
{
    return static_cast<psdc_iqcsd *>(create_impl(KINDS[K_IQCSD], n, win, power, nenbw, overlap, n_pairs, device, "psdc_iqcsd_create_window"));
}

psdc_iqcsd *psdc_iqcsd_create(uint32_t n, int window_kind, uint32_t n_pairs, int device)
{
    return static_cast<psdc_iqcsd *>(create_kind(KINDS[K_IQCSD], n, window_kind, n_pairs, device, "psdc_iqcsd_create"));
}

void psdc_iqcsd_destroy(psdc_iqcsd *h) { destroy_obj(h); }

int psdc_iqcsd_reset(psdc_iqcsd *h) { return reset_impl(h, "psdc_iqcsd_reset"); }
int psdc_iqcsd_set_detrend(psdc_iqcsd *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_iqcsd_set_detrend"); }
int psdc_iqcsd_set_avg(psdc_iqcsd *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_iqcsd_set_avg"); }

int psdc_iqcsd_set_carrier(psdc_iqcsd *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0)
{
    return pair_carrier_impl(h, pair, side, ftw, phase0, "psdc_iqcsd_set_carrier");
}

int psdc_iqcsd_process(psdc_iqcsd *h, uint32_t pair, const float *ia, const float *qa, const float *ib, const float *qb, size_t len)
{
    const void *const src[4] = {ia, qa, ib, qb};
    return iq_pair_feed(h, pair, src, false, SampleFmt{}, len, false, nullptr, "psdc_iqcsd_process");
}

int psdc_iqcsd_process_device(psdc_iqcsd *h, uint32_t pair, const float *d_ia, const float *d_qa, const float *d_ib, const float *d_qb,
                              size_t len, void *producer_event)
{
    const void *const src[4] = {d_ia, d_qa, d_ib, d_qb};
    return iq_pair_feed(h, pair, src, false, SampleFmt{}, len, true, producer_event, "psdc_iqcsd_process_device");
}

int psdc_iqcsd_process_interleaved(psdc_iqcsd *h, uint32_t pair, const float *za, const float *zb, size_t len)
{
    const void *const src[4] = {za, nullptr, zb, nullptr};
    return iq_pair_feed(h, pair, src, true, SampleFmt{}, len, false, nullptr, "psdc_iqcsd_process_interleaved");
}

int psdc_iqcsd_process_interleaved_device(psdc_iqcsd *h, uint32_t pair, const float *d_za, const float *d_zb, size_t len,
                                          void *producer_event)
{
    const void *const src[4] = {d_za, nullptr, d_zb, nullptr};
    return iq_pair_feed(h, pair, src, true, SampleFmt{}, len, true, producer_event, "psdc_iqcsd_process_interleaved_device");
}

int psdc_iqcsd_process_frames(psdc_iqcsd *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                              size_t *n_ok)
{
    return frames_host_impl(h, pair_traces, frames, frame_size, n_frames, n_ok, "psdc_iqcsd_process_frames");
}

int psdc_iqcsd_process_frames_device(psdc_iqcsd *h, const uint32_t *pair_traces, const uint8_t *d_frames, size_t frame_size,
                                     size_t n_frames, size_t *n_ok, void *producer_event)
{
    return frames_device_impl(h, pair_traces, d_frames, frame_size, n_frames, n_ok, producer_event, "psdc_iqcsd_process_frames_device");
}

int psdc_iqcsd_loss_read(psdc_iqcsd *h, psdc_loss *out, int reset) { return loss_impl(h, out, reset, "psdc_iqcsd_loss_read"); }
int psdc_iqcsd_sync(psdc_iqcsd *h) { return sync_impl(h, "psdc_iqcsd_sync"); }
int psdc_iqcsd_num_stages(psdc_iqcsd *h, uint32_t pair) { return num_stages_impl(h, pair, "psdc_iqcsd_num_stages"); }

int psdc_iqcsd_stage_spectra(psdc_iqcsd *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, float *rows)
{
    return stage_block(h, pair, stage, stat, rows, "psdc_iqcsd_stage_spectra");
}

int psdc_iqcsd_csd(psdc_iqcsd *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, float *saa_upper,
                   float *saa_lower, float *sbb_upper, float *sbb_lower, float *sab_upper, float *sab_lower, size_t cap, size_t *len,
                   psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return eight_rows_csd_impl(h, pair, {keep_overlap, min_count, keep_transition_band}, saa_upper, saa_lower, sbb_upper,
                               sbb_lower, sab_upper, sab_lower,
                               {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqcsd_csd");
}

int psdc_iqcsd_stats_read(psdc_iqcsd *h, uint64_t *launches, uint64_t *pairs_in, int reset)
{
    return stats_impl(h, launches, pairs_in, reset, "psdc_iqcsd_stats_read");
}

const char *psdc_iqcsd_last_error(const psdc_iqcsd *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- integer sample feeds (include/psdcascade.h, "integer sample feeds"): the objects' feeds with an integer SampleFmt ----

int psdc_int_zoom_process(psdc_zoom *h, uint32_t channel, const void *x, int kind, float scale, size_t len)
{
    const void *xs[1] = {x};
    return zoom_feed(h, channel, xs, int_fmt(kind, scale), len, false, nullptr, "psdc_int_zoom_process");
}

int psdc_int_zoom_process_device(psdc_zoom *h, uint32_t channel, const void *d_x, int kind, float scale, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return zoom_feed(h, channel, xs, int_fmt(kind, scale), len, true, producer_event, "psdc_int_zoom_process_device");
}

int psdc_int_zcsd_process(psdc_zcsd *h, uint32_t pair, const void *xa, const void *xb, int kind, float scale, size_t len)
{
    const void *xs[2] = {xa, xb};
    return zoom_feed(h, pair, xs, int_fmt(kind, scale), len, false, nullptr, "psdc_int_zcsd_process");
}

int psdc_int_zcsd_process_device(psdc_zcsd *h, uint32_t pair, const void *d_xa, const void *d_xb, int kind, float scale, size_t len,
                                 void *producer_event)
{
    const void *xs[2] = {d_xa, d_xb};
    return zoom_feed(h, pair, xs, int_fmt(kind, scale), len, true, producer_event, "psdc_int_zcsd_process_device");
}

int psdc_int_iq_process(psdc_iq *h, uint32_t channel, const void *z, int kind, float scale, size_t len)
{
    return iq_feed(h, channel, z, nullptr, true, int_fmt(kind, scale), len, false, nullptr, "psdc_int_iq_process");
}

int psdc_int_iq_process_device(psdc_iq *h, uint32_t channel, const void *d_z, int kind, float scale, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_z, nullptr, true, int_fmt(kind, scale), len, true, producer_event, "psdc_int_iq_process_device");
}

int psdc_int_iqcsd_process(psdc_iqcsd *h, uint32_t pair, const void *za, const void *zb, int kind, float scale, size_t len)
{
    const void *const src[4] = {za, nullptr, zb, nullptr};
    return iq_pair_feed(h, pair, src, true, int_fmt(kind, scale), len, false, nullptr, "psdc_int_iqcsd_process");
}

int psdc_int_iqcsd_process_device(psdc_iqcsd *h, uint32_t pair, const void *d_za, const void *d_zb, int kind, float scale, size_t len,
                                  void *producer_event)
{
    const void *const src[4] = {d_za, nullptr, d_zb, nullptr};
    return iq_pair_feed(h, pair, src, true, int_fmt(kind, scale), len, true, producer_event, "psdc_int_iqcsd_process_device");
}

// ---- integer sample feeds of the real-input objects (include/psdcascade.h): the pair and the matrix object; psdc_sint_process[_device]
// of the PSD object are in runtime.cpp ----

int psdc_sint_cross_process(psdc_cross *h, uint32_t pair, const void *x, const void *y, int kind, float scale, size_t len)
{
    const void *xs[2] = {x, y};
    return process_impl(h, pair, xs, int_fmt(kind, scale), len, "psdc_sint_cross_process");
}

int psdc_sint_cross_process_device(psdc_cross *h, uint32_t pair, const void *d_x, const void *d_y, int kind, float scale, size_t len,
                                   void *producer_event)
{
    const void *xs[2] = {d_x, d_y};
    return process_device_impl(h, pair, xs, int_fmt(kind, scale), len, producer_event, "psdc_sint_cross_process_device");
}

int psdc_sint_csm_process(psdc_csm *h, uint32_t group, const void *const *x, int kind, float scale, size_t len)
{
    return process_impl(h, group, x, int_fmt(kind, scale), len, "psdc_sint_csm_process");
}

int psdc_sint_csm_process_device(psdc_csm *h, uint32_t group, const void *const *d_x, int kind, float scale, size_t len, void *producer_event)
{
    return process_device_impl(h, group, d_x, int_fmt(kind, scale), len, producer_event, "psdc_sint_csm_process_device");
}

} // extern "C"

// ---- spectral kurtosis: one real stream a unit; sk_kernel, rows S1 = sum w P and S2 = sum w P^2 ----

namespace {

// (SK of one bin from its moments: sk_estimate of carrier_readout.h, the text the device read-out runs too)

// the stitch of row 0 (psd != NULL: written) and, with sk != NULL, the SK of every bin the stitch takes, selected by its Breaks
int sk_readout_impl(XObj *h, uint32_t channel, const StitchSel &sel, float *psd, double *sk, const StitchOut &o, const char *who)
{
    const RowOut<float> outs[1] = {{psd}};
    Stitched st;
    int rc = unit_stitch(h, channel, sel, 1, outs, sk != nullptr, o, BreaksOf::OWN, who, who, &st);
    if (rc || !sk)
        return rc;
    const size_t b = bins(h);
    st.each_bin([&](size_t stage, size_t k, size_t out, const psdc_break &br) {
        const double *a = st.snap.stage(stage);
        sk[out] = sk_estimate(br.count, a[k], a[b + k]);
    });
    return PSDC_OK;
}

} // namespace

extern "C" {

int psdc_sk_supported(uint32_t n) { return n <= 4096 && cross_supported((int)n) ? 1 : 0; }

psdc_sk *psdc_sk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_sk *>(create_impl(KINDS[K_SK], n, win, power, nenbw, overlap, n_channels, device, "psdc_sk_create_window"));
}

psdc_sk *psdc_sk_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_sk *>(create_kind(KINDS[K_SK], n, window_kind, n_channels, device, "psdc_sk_create"));
}

void psdc_sk_destroy(psdc_sk *h) { destroy_obj(h); }

int psdc_sk_reset(psdc_sk *h) { return reset_impl(h, "psdc_sk_reset"); }
int psdc_sk_set_detrend(psdc_sk *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_sk_set_detrend"); }
int psdc_sk_set_avg(psdc_sk *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_sk_set_avg"); }

int psdc_sk_process(psdc_sk *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return process_impl(h, channel, xs, SampleFmt{}, len, "psdc_sk_process");
}

int psdc_sk_process_device(psdc_sk *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return process_device_impl(h, channel, xs, SampleFmt{}, len, producer_event, "psdc_sk_process_device");
}

int psdc_sk_sync(psdc_sk *h) { return sync_impl(h, "psdc_sk_sync"); }
int psdc_sk_num_stages(psdc_sk *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_sk_num_stages"); }

int psdc_sk_stage_moments(psdc_sk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1, double *s2)
{
    const RowOut<double> outs[SK_ROWS] = {{s1}, {s2}};
    return stage_rows(h, channel, stage, stat, outs, SK_ROWS, "psdc_sk_stage_moments");
}

int psdc_sk_psd(psdc_sk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *psd, size_t cap,
                size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return sk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, psd, nullptr,
                           {cap, len, breaks, breaks_cap, n_breaks}, "psdc_sk_psd");
}

int psdc_sk_sk(psdc_sk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk, size_t cap,
               size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return sk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, nullptr, sk,
                           {cap, len, breaks, breaks_cap, n_breaks}, "psdc_sk_sk");
}

int psdc_sk_stats_read(psdc_sk *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_sk_stats_read");
}

const char *psdc_sk_last_error(const psdc_sk *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

} // extern "C"

// ---- zoom / IQ spectral kurtosis: the zoom / IQ object on zoom_sk_kernel, rows S1 upper, S1 lower, S2 upper, S2 lower ----

namespace {

// the zoom read-out of rows 0 and 1 (sk_upper == sk_lower == NULL: upper / lower written where given), or the SK of every bin
// that read-out takes, both sides, selected by its Breaks (upper == lower == NULL)
int zsk_readout_impl(XObj *h, uint32_t channel, const StitchSel &sel, float *upper, float *lower, double *sk_upper, double *sk_lower,
                     const StitchOut &o, const char *who)
{
    const RowOut<float> outs[2] = {{upper}, {lower}};
    Stitched st;
    int rc = unit_stitch(h, channel, sel, 2, outs, sk_upper || sk_lower, o, BreaksOf::OWN, who, who, &st);
    if (rc || !(sk_upper || sk_lower))
        return rc;
    const size_t b = bins(h);
    st.each_bin([&](size_t stage, size_t k, size_t out, const psdc_break &br) {
        const double *a = st.snap.stage(stage);
        if (sk_upper)
            sk_upper[out] = sk_estimate(br.count, a[k], a[2 * b + k]);
        if (sk_lower)
            sk_lower[out] = sk_estimate(br.count, a[b + k], a[3 * b + k]);
    });
    return PSDC_OK;
}

// the four f64 rows of one stage (the moments of the SK kinds, the rows of the AM/PM kinds)
int four_rows_stage_impl(XObj *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *r0, double *r1, double *r2, double *r3,
                         const char *who)
{
    const RowOut<double> outs[ZSK_ROWS] = {{r0}, {r1}, {r2}, {r3}};
    return stage_rows(h, channel, stage, stat, outs, ZSK_ROWS, who);
}

} // namespace

extern "C" {

int psdc_zsk_supported(uint32_t n) { return psdc_sk_supported(n); }

psdc_zsk *psdc_zsk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_zsk *>(create_impl(KINDS[K_ZSK], n, win, power, nenbw, overlap, n_channels, device, "psdc_zsk_create_window"));
}

psdc_zsk *psdc_zsk_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_zsk *>(create_kind(KINDS[K_ZSK], n, window_kind, n_channels, device, "psdc_zsk_create"));
}

void psdc_zsk_destroy(psdc_zsk *h) { destroy_obj(h); }
int psdc_zsk_reset(psdc_zsk *h) { return reset_impl(h, "psdc_zsk_reset"); }
int psdc_zsk_set_detrend(psdc_zsk *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zsk_set_detrend"); }
int psdc_zsk_set_avg(psdc_zsk *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_zsk_set_avg"); }

int psdc_zsk_set_carrier(psdc_zsk *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_zsk_set_carrier");
}

int psdc_zsk_process(psdc_zsk *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, false, nullptr, "psdc_zsk_process");
}

int psdc_zsk_process_device(psdc_zsk *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, true, producer_event, "psdc_zsk_process_device");
}

int psdc_zsk_sync(psdc_zsk *h) { return sync_impl(h, "psdc_zsk_sync"); }
int psdc_zsk_num_stages(psdc_zsk *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_zsk_num_stages"); }

int psdc_zsk_stage_moments(psdc_zsk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1_upper, double *s1_lower,
                           double *s2_upper, double *s2_lower)
{
    return four_rows_stage_impl(h, channel, stage, stat, s1_upper, s1_lower, s2_upper, s2_lower, "psdc_zsk_stage_moments");
}

int psdc_zsk_psd(psdc_zsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                 float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, nullptr, nullptr,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zsk_psd");
}

int psdc_zsk_sk(psdc_zsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk_upper,
                double *sk_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, nullptr, nullptr, sk_upper, sk_lower,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zsk_sk");
}

int psdc_zsk_stats_read(psdc_zsk *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_zsk_stats_read");
}

const char *psdc_zsk_last_error(const psdc_zsk *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

int psdc_iqsk_supported(uint32_t n) { return psdc_sk_supported(n); }

psdc_iqsk *psdc_iqsk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_iqsk *>(create_impl(KINDS[K_IQSK], n, win, power, nenbw, overlap, n_channels, device, "psdc_iqsk_create_window"));
}

psdc_iqsk *psdc_iqsk_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_iqsk *>(create_kind(KINDS[K_IQSK], n, window_kind, n_channels, device, "psdc_iqsk_create"));
}

void psdc_iqsk_destroy(psdc_iqsk *h) { destroy_obj(h); }
int psdc_iqsk_reset(psdc_iqsk *h) { return reset_impl(h, "psdc_iqsk_reset"); }
int psdc_iqsk_set_detrend(psdc_iqsk *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_iqsk_set_detrend"); }
int psdc_iqsk_set_avg(psdc_iqsk *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_iqsk_set_avg"); }

int psdc_iqsk_set_carrier(psdc_iqsk *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_iqsk_set_carrier");
}

int psdc_iqsk_process(psdc_iqsk *h, uint32_t channel, const float *i, const float *q, size_t len)
{
    return iq_feed(h, channel, i, q, false, SampleFmt{}, len, false, nullptr, "psdc_iqsk_process");
}

int psdc_iqsk_process_device(psdc_iqsk *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_i, d_q, false, SampleFmt{}, len, true, producer_event, "psdc_iqsk_process_device");
}

int psdc_iqsk_process_interleaved(psdc_iqsk *h, uint32_t channel, const float *iq, size_t len)
{
    return iq_feed(h, channel, iq, nullptr, true, SampleFmt{}, len, false, nullptr, "psdc_iqsk_process_interleaved");
}

int psdc_iqsk_process_interleaved_device(psdc_iqsk *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_iq, nullptr, true, SampleFmt{}, len, true, producer_event, "psdc_iqsk_process_interleaved_device");
}

int psdc_iqsk_sync(psdc_iqsk *h) { return sync_impl(h, "psdc_iqsk_sync"); }
int psdc_iqsk_num_stages(psdc_iqsk *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_iqsk_num_stages"); }

int psdc_iqsk_stage_moments(psdc_iqsk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1_upper, double *s1_lower,
                            double *s2_upper, double *s2_lower)
{
    return four_rows_stage_impl(h, channel, stage, stat, s1_upper, s1_lower, s2_upper, s2_lower, "psdc_iqsk_stage_moments");
}

int psdc_iqsk_psd(psdc_iqsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                  float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, nullptr, nullptr,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqsk_psd");
}

int psdc_iqsk_sk(psdc_iqsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk_upper,
                 double *sk_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, nullptr, nullptr, sk_upper, sk_lower,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqsk_sk");
}

int psdc_iqsk_stats_read(psdc_iqsk *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_iqsk_stats_read");
}

const char *psdc_iqsk_last_error(const psdc_iqsk *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

} // extern "C"

// ---- AM/PM: the zoom / IQ object on zoom_ampm_kernel, rows upper, lower, comp_re, comp_im ----

namespace {

static_assert(ZAMPM_ROWS == ZSK_ROWS, "the AM/PM stage read-out is four_rows_stage_impl: four f64 rows a stage");

// the rows() rows of a unit stitched in f64 into outs[r] (NULL: that row is not wanted): the row stitch picks the stages and bins
// from rows 0 and 1 (one set of Breaks, the zoom read-out's), and every selected bin of the f64 accumulators is scaled by the f32
// factor that stitch applies to the stage
int rows_sidebands_impl(XObj *h, uint32_t channel, const StitchSel &sel, double *const *outs, uint32_t nrows, const StitchOut &o, const char *who)
{
    const RowOut<float> none[2];
    const bool any = std::any_of(outs, outs + nrows, [](double *p) { return p != nullptr; });
    Stitched st;
    int rc = unit_stitch(h, channel, sel, 2, none, any, o, BreaksOf::OWN, who, who, &st);
    if (rc || !any)
        return rc;
    double gsc[X_MAX_STAGES] = {};
    for (size_t i = 0; i < st.nb; ++i)
        if (st.br[i].include)
            gsc[st.snap.ns - 1 - i] = 1.0f / (psdrt::stage_gain(h->n, st.snap.c64[st.snap.ns - 1 - i], h->nenbw, h->power) * (float)st.br[i].decimation);
    const size_t b = bins(h);
    st.each_bin([&](size_t stage, size_t k, size_t out, const psdc_break &) {
        for (uint32_t r = 0; r < nrows; ++r)
            if (outs[r])
                outs[r][out] = st.snap.stage(stage)[r * b + k] * gsc[stage];
    });
    return PSDC_OK;
}

int ampm_sidebands_impl(XObj *h, uint32_t channel, const StitchSel &sel, double *upper, double *lower, double *comp_re, double *comp_im,
                        const StitchOut &o, const char *who)
{
    double *outs[ZAMPM_ROWS] = {upper, lower, comp_re, comp_im};
    return rows_sidebands_impl(h, channel, sel, outs, ZAMPM_ROWS, o, who);
}

} // namespace

extern "C" {

int psdc_zampm_supported(uint32_t n) { return psdc_sk_supported(n); }

psdc_zampm *psdc_zampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_zampm *>(create_impl(KINDS[K_ZAMPM], n, win, power, nenbw, overlap, n_channels, device, "psdc_zampm_create_window"));
}

psdc_zampm *psdc_zampm_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_zampm *>(create_kind(KINDS[K_ZAMPM], n, window_kind, n_channels, device, "psdc_zampm_create"));
}

void psdc_zampm_destroy(psdc_zampm *h) { destroy_obj(h); }
int psdc_zampm_reset(psdc_zampm *h) { return reset_impl(h, "psdc_zampm_reset"); }
int psdc_zampm_set_detrend(psdc_zampm *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zampm_set_detrend"); }
int psdc_zampm_set_avg(psdc_zampm *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_zampm_set_avg"); }

int psdc_zampm_set_carrier(psdc_zampm *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_zampm_set_carrier");
}

int psdc_zampm_process(psdc_zampm *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, false, nullptr, "psdc_zampm_process");
}

int psdc_zampm_process_device(psdc_zampm *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, true, producer_event, "psdc_zampm_process_device");
}

int psdc_zampm_sync(psdc_zampm *h) { return sync_impl(h, "psdc_zampm_sync"); }
int psdc_zampm_num_stages(psdc_zampm *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_zampm_num_stages"); }

int psdc_zampm_stage_rows(psdc_zampm *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *upper, double *lower, double *comp_re,
                          double *comp_im)
{
    return four_rows_stage_impl(h, channel, stage, stat, upper, lower, comp_re, comp_im, "psdc_zampm_stage_rows");
}

int psdc_zampm_psd(psdc_zampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper, float *lower,
                   size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, nullptr, nullptr,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zampm_psd");
}

int psdc_zampm_sidebands(psdc_zampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *upper,
                         double *lower, double *comp_re, double *comp_im, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap,
                         size_t *n_breaks)
{
    return ampm_sidebands_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, comp_re, comp_im,
                               {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zampm_sidebands");
}

int psdc_zampm_stats_read(psdc_zampm *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_zampm_stats_read");
}

const char *psdc_zampm_last_error(const psdc_zampm *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

int psdc_iqampm_supported(uint32_t n) { return psdc_sk_supported(n); }

psdc_iqampm *psdc_iqampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, int device)
{
    return static_cast<psdc_iqampm *>(create_impl(KINDS[K_IQAMPM], n, win, power, nenbw, overlap, n_channels, device, "psdc_iqampm_create_window"));
}

psdc_iqampm *psdc_iqampm_create(uint32_t n, int window_kind, uint32_t n_channels, int device)
{
    return static_cast<psdc_iqampm *>(create_kind(KINDS[K_IQAMPM], n, window_kind, n_channels, device, "psdc_iqampm_create"));
}

void psdc_iqampm_destroy(psdc_iqampm *h) { destroy_obj(h); }
int psdc_iqampm_reset(psdc_iqampm *h) { return reset_impl(h, "psdc_iqampm_reset"); }
int psdc_iqampm_set_detrend(psdc_iqampm *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_iqampm_set_detrend"); }
int psdc_iqampm_set_avg(psdc_iqampm *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_iqampm_set_avg"); }

int psdc_iqampm_set_carrier(psdc_iqampm *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_iqampm_set_carrier");
}

int psdc_iqampm_process(psdc_iqampm *h, uint32_t channel, const float *i, const float *q, size_t len)
{
    return iq_feed(h, channel, i, q, false, SampleFmt{}, len, false, nullptr, "psdc_iqampm_process");
}

int psdc_iqampm_process_device(psdc_iqampm *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_i, d_q, false, SampleFmt{}, len, true, producer_event, "psdc_iqampm_process_device");
}

int psdc_iqampm_process_interleaved(psdc_iqampm *h, uint32_t channel, const float *iq, size_t len)
{
    return iq_feed(h, channel, iq, nullptr, true, SampleFmt{}, len, false, nullptr, "psdc_iqampm_process_interleaved");
}

int psdc_iqampm_process_interleaved_device(psdc_iqampm *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event)
{
    return iq_feed(h, channel, d_iq, nullptr, true, SampleFmt{}, len, true, producer_event, "psdc_iqampm_process_interleaved_device");
}

int psdc_iqampm_sync(psdc_iqampm *h) { return sync_impl(h, "psdc_iqampm_sync"); }
int psdc_iqampm_num_stages(psdc_iqampm *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_iqampm_num_stages"); }

int psdc_iqampm_stage_rows(psdc_iqampm *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *upper, double *lower, double *comp_re,
                           double *comp_im)
{
    return four_rows_stage_impl(h, channel, stage, stat, upper, lower, comp_re, comp_im, "psdc_iqampm_stage_rows");
}

int psdc_iqampm_psd(psdc_iqampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper, float *lower,
                    size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return zsk_readout_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, nullptr, nullptr,
                            {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqampm_psd");
}

int psdc_iqampm_sidebands(psdc_iqampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *upper,
                          double *lower, double *comp_re, double *comp_im, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap,
                          size_t *n_breaks)
{
    return ampm_sidebands_impl(h, channel, {keep_overlap, min_count, keep_transition_band}, upper, lower, comp_re, comp_im,
                               {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqampm_sidebands");
}

int psdc_iqampm_stats_read(psdc_iqampm *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_iqampm_stats_read");
}

const char *psdc_iqampm_last_error(const psdc_iqampm *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

} // extern "C"

// ---- AM/PM cross: the zoom cross / IQ cross object on zoom_ampm_cross_kernel, the twelve rows of zoom_ampm_cross_fft.h ----

namespace {

// the twelve rows stitched in f64 into rows[12][cap] (rows_sidebands_impl: one set of Breaks, from rows 0 and 1 -- the zoom
// read-out's of channel a)
int xampm_sidebands_impl(XObj *h, uint32_t pair, const StitchSel &sel, double *rows, const StitchOut &o, const char *who)
{
    double *outs[ZXAMPM_ROWS];
    for (int r = 0; r < ZXAMPM_ROWS; ++r)
        outs[r] = rows ? rows + (size_t)r * o.cap : nullptr;
    return rows_sidebands_impl(h, pair, sel, outs, ZXAMPM_ROWS, o, who);
}

} // namespace

extern "C" {

// (the twelve-row kernel uses no scratch at any size of the zoom cross object: none is refused beyond that object's)
int psdc_zxampm_supported(uint32_t n) { return psdc_zcsd_supported(n); }

psdc_zxampm *psdc_zxampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs, int device)
{
    return static_cast<psdc_zxampm *>(create_impl(KINDS[K_ZXAMPM], n, win, power, nenbw, overlap, n_pairs, device, "psdc_zxampm_create_window"));
}

psdc_zxampm *psdc_zxampm_create(uint32_t n, int window_kind, uint32_t n_pairs, int device)
{
    return static_cast<psdc_zxampm *>(create_kind(KINDS[K_ZXAMPM], n, window_kind, n_pairs, device, "psdc_zxampm_create"));
}

void psdc_zxampm_destroy(psdc_zxampm *h) { destroy_obj(h); }
int psdc_zxampm_reset(psdc_zxampm *h) { return reset_impl(h, "psdc_zxampm_reset"); }
int psdc_zxampm_set_detrend(psdc_zxampm *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zxampm_set_detrend"); }
int psdc_zxampm_set_avg(psdc_zxampm *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_zxampm_set_avg"); }

int psdc_zxampm_set_carrier(psdc_zxampm *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0)
{
    return pair_carrier_impl(h, pair, side, ftw, phase0, "psdc_zxampm_set_carrier");
}

int psdc_zxampm_process(psdc_zxampm *h, uint32_t pair, const float *x, const float *y, size_t len)
{
    const void *xs[2] = {x, y};
    return zoom_feed(h, pair, xs, SampleFmt{}, len, false, nullptr, "psdc_zxampm_process");
}

int psdc_zxampm_process_device(psdc_zxampm *h, uint32_t pair, const float *d_x, const float *d_y, size_t len, void *producer_event)
{
    const void *xs[2] = {d_x, d_y};
    return zoom_feed(h, pair, xs, SampleFmt{}, len, true, producer_event, "psdc_zxampm_process_device");
}

int psdc_zxampm_sync(psdc_zxampm *h) { return sync_impl(h, "psdc_zxampm_sync"); }
int psdc_zxampm_num_stages(psdc_zxampm *h, uint32_t pair) { return num_stages_impl(h, pair, "psdc_zxampm_num_stages"); }

int psdc_zxampm_stage_rows(psdc_zxampm *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, double *rows)
{
    return stage_block(h, pair, stage, stat, rows, "psdc_zxampm_stage_rows");
}

int psdc_zxampm_sidebands(psdc_zxampm *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, double *rows,
                          size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return xampm_sidebands_impl(h, pair, {keep_overlap, min_count, keep_transition_band}, rows,
                                {cap, len, breaks, breaks_cap, n_breaks}, "psdc_zxampm_sidebands");
}

int psdc_zxampm_stats_read(psdc_zxampm *h, uint64_t *launches, uint64_t *pairs_in, int reset)
{
    return stats_impl(h, launches, pairs_in, reset, "psdc_zxampm_stats_read");
}

const char *psdc_zxampm_last_error(const psdc_zxampm *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

int psdc_iqxampm_supported(uint32_t n) { return psdc_zxampm_supported(n); }

psdc_iqxampm *psdc_iqxampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs, int device)
{
    return static_cast<psdc_iqxampm *>(create_impl(KINDS[K_IQXAMPM], n, win, power, nenbw, overlap, n_pairs, device, "psdc_iqxampm_create_window"));
}

psdc_iqxampm *psdc_iqxampm_create(uint32_t n, int window_kind, uint32_t n_pairs, int device)
{
    return static_cast<psdc_iqxampm *>(create_kind(KINDS[K_IQXAMPM], n, window_kind, n_pairs, device, "psdc_iqxampm_create"));
}

void psdc_iqxampm_destroy(psdc_iqxampm *h) { destroy_obj(h); }
int psdc_iqxampm_reset(psdc_iqxampm *h) { return reset_impl(h, "psdc_iqxampm_reset"); }
int psdc_iqxampm_set_detrend(psdc_iqxampm *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_iqxampm_set_detrend"); }
int psdc_iqxampm_set_avg(psdc_iqxampm *h, uint32_t limit, uint32_t count) { return set_avg_impl(h, limit, count, "psdc_iqxampm_set_avg"); }

int psdc_iqxampm_set_carrier(psdc_iqxampm *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0)
{
    return pair_carrier_impl(h, pair, side, ftw, phase0, "psdc_iqxampm_set_carrier");
}

int psdc_iqxampm_process(psdc_iqxampm *h, uint32_t pair, const float *ia, const float *qa, const float *ib, const float *qb, size_t len)
{
    const void *const src[4] = {ia, qa, ib, qb};
    return iq_pair_feed(h, pair, src, false, SampleFmt{}, len, false, nullptr, "psdc_iqxampm_process");
}

int psdc_iqxampm_process_device(psdc_iqxampm *h, uint32_t pair, const float *d_ia, const float *d_qa, const float *d_ib, const float *d_qb,
                                size_t len, void *producer_event)
{
    const void *const src[4] = {d_ia, d_qa, d_ib, d_qb};
    return iq_pair_feed(h, pair, src, false, SampleFmt{}, len, true, producer_event, "psdc_iqxampm_process_device");
}

int psdc_iqxampm_process_interleaved(psdc_iqxampm *h, uint32_t pair, const float *za, const float *zb, size_t len)
{
    const void *const src[4] = {za, nullptr, zb, nullptr};
    return iq_pair_feed(h, pair, src, true, SampleFmt{}, len, false, nullptr, "psdc_iqxampm_process_interleaved");
}

int psdc_iqxampm_process_interleaved_device(psdc_iqxampm *h, uint32_t pair, const float *d_za, const float *d_zb, size_t len,
                                            void *producer_event)
{
    const void *const src[4] = {d_za, nullptr, d_zb, nullptr};
    return iq_pair_feed(h, pair, src, true, SampleFmt{}, len, true, producer_event, "psdc_iqxampm_process_interleaved_device");
}

int psdc_iqxampm_sync(psdc_iqxampm *h) { return sync_impl(h, "psdc_iqxampm_sync"); }
int psdc_iqxampm_num_stages(psdc_iqxampm *h, uint32_t pair) { return num_stages_impl(h, pair, "psdc_iqxampm_num_stages"); }

int psdc_iqxampm_stage_rows(psdc_iqxampm *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, double *rows)
{
    return stage_block(h, pair, stage, stat, rows, "psdc_iqxampm_stage_rows");
}

int psdc_iqxampm_sidebands(psdc_iqxampm *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, double *rows,
                           size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks)
{
    return xampm_sidebands_impl(h, pair, {keep_overlap, min_count, keep_transition_band}, rows,
                                {cap, len, breaks, breaks_cap, n_breaks}, "psdc_iqxampm_sidebands");
}

int psdc_iqxampm_stats_read(psdc_iqxampm *h, uint64_t *launches, uint64_t *pairs_in, int reset)
{
    return stats_impl(h, launches, pairs_in, reset, "psdc_iqxampm_stats_read");
}

const char *psdc_iqxampm_last_error(const psdc_iqxampm *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

} // extern "C"

// ---- waterfall: the SK / zoom SK object with a ring of row sets a stage, one block of wf_block segments a slot (run_round cuts the
// pieces); read out as raw moment rows or, through wf_image_kernel, as PSD and SK images ----

namespace {

constexpr uint64_t WF_MAX_BLOCK = (uint64_t)1 << 24;
constexpr uint64_t WF_MAX_RING_BYTES = (uint64_t)1 << 27;

// "": block, depth and the ring they make at size n are fine
std::string wf_refusal(const KindDesc &kind, uint32_t n, uint32_t block, uint32_t depth)
{
    if (block < 2 || block > WF_MAX_BLOCK)
        return "block = " + std::to_string(block) + ": block must be in [2, 2^24] segments (SK needs two)";
    if (depth < 1)
        return "depth = 0: depth must be at least 1 ring row a stage";
    if (n > 4096)
        return ""; // (the size is refused by name below)
    const uint64_t bytes = (uint64_t)depth * kind.rows * (n / 2 + 1) * sizeof(double);
    if (bytes > WF_MAX_RING_BYTES)
        return "a stage's ring of depth " + std::to_string(depth) + " x " + std::to_string(kind.rows) + " rows x " +
               std::to_string(n / 2 + 1) + " bins x 8 bytes = " + std::to_string(bytes) + " bytes: it must be at most 2^27 = " +
               std::to_string(WF_MAX_RING_BYTES) + " bytes";
    return "";
}

XObj *wf_create(Kind k, uint32_t n, int window_kind, const float *win, float power, float nenbw, size_t overlap, bool table,
                uint32_t n_channels, uint32_t block, uint32_t depth, int device, const char *who)
{
    const std::string why = wf_refusal(KINDS[k], n, block, depth);
    if (!why.empty()) {
        xfail(nullptr, PSDC_ERR_ARG, std::string(who) + ": " + why);
        return nullptr;
    }
    XObj *h = table ? create_impl(KINDS[k], n, win, power, nenbw, overlap, n_channels, device, who)
                    : create_kind(KINDS[k], n, window_kind, n_channels, device, who);
    if (h) {
        h->wf_block = block;
        h->wf_depth = depth;
    }
    return h;
}

// a drained stage of a waterfall object and what its ring holds
struct WfStage {
    const XStage *s = nullptr;
    uint64_t started = 0;
    uint32_t valid = 0, newest = 0;
};

int wf_stage(XObj *h, uint32_t channel, uint32_t stage, WfStage *out, const char *who)
{
    int rc = check_pair(h, channel);
    if (rc)
        return rc;
    if ((rc = drained_stage(h, channel, stage, &out->s, who)))
        return rc;
    out->started = wf_blocks_started(out->s->segs, h->wf_block);
    out->valid = wf_valid_rows(out->started, h->wf_depth);
    out->newest = wf_newest_count(out->s->segs, h->wf_block);
    return PSDC_OK;
}

int wf_stage_blocks_impl(XObj *h, uint32_t channel, uint32_t stage, psdc_wf_blocks *out, const char *who)
{
    X_HANDLE(h, who);
    if (!out)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output");
    X_ON_DEVICE(h);
    WfStage w;
    int rc = wf_stage(h, channel, stage, &w, who);
    if (rc)
        return rc;
    out->block = h->wf_block;
    out->depth = h->wf_depth;
    out->started = w.started;
    out->rows_valid = w.valid;
    out->newest_count = w.newest;
    out->pending = pending_for(h->geo, w.s->total);
    return PSDC_OK;
}

// the rows a read-out of at most max_rows rows returns: their number, absolute block indices and counts (oldest first)
uint32_t wf_rows_meta(const XObj *h, const WfStage &w, uint32_t max_rows, uint64_t *block_index, uint32_t *counts)
{
    const uint32_t nr = std::min(max_rows, w.valid);
    for (uint32_t r = 0; r < nr; ++r) {
        block_index[r] = wf_row_block(w.started, nr, r);
        counts[r] = r + 1 == nr ? w.newest : h->wf_block;
    }
    return nr;
}

// outs[i]: row i of every returned block, [max_rows][n/2 + 1] f64, NULL: not wanted
int wf_stage_rows_impl(XObj *h, uint32_t channel, uint32_t stage, uint32_t max_rows, uint64_t *block_index, uint32_t *counts,
                       double *const *outs, uint32_t *n_rows, const char *who)
{
    X_HANDLE(h, who);
    if (!block_index || !counts || !n_rows)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output (block_index, counts and n_rows are always written)");
    X_ON_DEVICE(h);
    WfStage w;
    int rc = wf_stage(h, channel, stage, &w, who);
    if (rc)
        return rc;
    const uint32_t nr = wf_rows_meta(h, w, max_rows, block_index, counts);
    *n_rows = nr;
    bool any = false;
    for (uint32_t i = 0; i < h->rows(); ++i)
        any = any || outs[i];
    if (!nr || !any)
        return PSDC_OK;
    if ((rc = sync_all(h)))
        return rc;
    // the nr slots are consecutive in the ring, in at most two runs (one before the ring's end, one from its start)
    const size_t b = bins(h), set = h->rows() * b;
    std::vector<double> host((size_t)nr * set);
    const uint32_t first = wf_row_slot(w.started, h->wf_depth, nr, 0);
    const uint32_t run0 = std::min(nr, h->wf_depth - first);
    XCHK(h, hipMemcpy(host.data(), w.s->acc + (size_t)first * set, sizeof(double) * run0 * set, hipMemcpyDeviceToHost));
    if (nr > run0)
        XCHK(h, hipMemcpy(host.data() + (size_t)run0 * set, w.s->acc, sizeof(double) * (nr - run0) * set, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < nr; ++r)
        for (uint32_t i = 0; i < h->rows(); ++i)
            if (outs[i])
                std::copy(&host[(size_t)r * set + i * b], &host[(size_t)r * set + (i + 1) * b], outs[i] + (size_t)r * b);
    return PSDC_OK;
}

// psd / sk: [rows][sides][n/2 + 1] f32 images of the newest min(max_rows, valid) blocks through wf_image_kernel; device: the two
// are device memory, else host arrays filled through a device buffer of the call's own
int wf_image_impl(XObj *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *psd, float *sk, bool device, uint64_t *block_index,
                  uint32_t *counts, uint32_t *n_rows, const char *who)
{
    X_HANDLE(h, who);
    if (!psd && !sk)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output (give psd, sk or both)");
    if (!block_index || !counts || !n_rows)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output (block_index, counts and n_rows are always written)");
    X_ON_DEVICE(h);
    WfStage w;
    int rc = wf_stage(h, channel, stage, &w, who);
    if (rc)
        return rc;
    const uint32_t nr = wf_rows_meta(h, w, max_rows, block_index, counts);
    *n_rows = nr;
    if (!nr)
        return PSDC_OK;
    const uint32_t sides = h->rows() / 2;
    const size_t image = (size_t)nr * sides * bins(h);
    float *tmp = nullptr;
    if (!device)
        XCHK(h, hipMalloc(&tmp, sizeof(float) * image * 2));
    const float dec = (float)((uint64_t)1 << (3 * stage)); // (the stitch's `decimation` of this stage)
    WfImageJob j{};
    j.ring = w.s->acc;
    j.psd = device ? psd : (psd ? tmp : nullptr);
    j.sk = device ? sk : (sk ? tmp + image : nullptr);
    j.started = w.started;
    j.depth = h->wf_depth;
    j.nr = nr;
    j.nbins = (unsigned)bins(h);
    j.sides = sides;
    j.block = h->wf_block;
    j.newest = w.newest;
    j.gsc_block = 1.0f / (psdrt::stage_gain(h->n, h->wf_block, h->nenbw, h->power) * dec);
    j.gsc_newest = 1.0f / (psdrt::stage_gain(h->n, w.newest, h->nenbw, h->power) * dec);
    hipError_t e = launch_wf_image(j, h->stream);
    if (e == hipSuccess) {
        ++h->launches;
        e = hipStreamSynchronize(h->stream);
    }
    if (e == hipSuccess && !device && psd)
        e = hipMemcpy(psd, tmp, sizeof(float) * image, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !device && sk)
        e = hipMemcpy(sk, tmp + image, sizeof(float) * image, hipMemcpyDeviceToHost);
    if (tmp)
        (void)hipFree(tmp);
    XCHK(h, e);
    return PSDC_OK;
}

// median / min / max / excised: [sides][n/2 + 1] f32 and kept: the same in u32, over the newest min(max_rows, complete blocks,
// 4096) complete blocks through wf_robust_kernel (include/psdcascade_robust.h); device: the five are device memory, else host arrays
// filled through a device buffer of the call's own
int wf_robust_impl(XObj *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *median, float *mn,
                   float *mx, float *excised, uint32_t *kept, bool device, psdcx_robust_info *info, const char *who)
{
    X_HANDLE(h, who);
    if (!info)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null info (it is always written)");
    if (!median && !mn && !mx && !excised && !kept)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": null output (give at least one of median, min, max, excised, kept)");
    if ((excised || kept) && !(sk_lo <= sk_hi)) // (false for a NaN)
        return xfail(h, PSDC_ERR_ARG, std::string(who) + ": sk_lo = " + std::to_string(sk_lo) + ", sk_hi = " + std::to_string(sk_hi) +
                                          ": excised and kept need limits sk_lo <= sk_hi that are not NaN");
    X_ON_DEVICE(h);
    WfStage w;
    int rc = wf_stage(h, channel, stage, &w, who);
    if (rc)
        return rc;
    uint64_t last = 0;
    const uint32_t R = wf_robust_rows(w.started, w.newest, h->wf_block, h->wf_depth, max_rows, &last);
    info->rows = R;
    info->block = h->wf_block;
    info->first_block = R ? last - (R - 1) : 0;
    info->last_block = R ? last : 0;
    if (!R)
        return PSDC_OK;
    const uint32_t sides = h->rows() / 2;
    const size_t row = (size_t)sides * bins(h);
    void *out[5] = {median, mn, mx, excised, kept}; // (f32 and u32: four bytes an element each)
    float *tmp = nullptr;
    if (!device)
        XCHK(h, hipMalloc(&tmp, sizeof(float) * row * 5));
    const float dec = (float)((uint64_t)1 << (3 * stage)); // (the stitch's `decimation` of this stage)
    void *dev[5];
    for (int i = 0; i < 5; ++i)
        dev[i] = device ? out[i] : (out[i] ? tmp + (size_t)i * row : nullptr);
    WfRobustJob j{};
    j.ring = w.s->acc;
    j.median = static_cast<float *>(dev[0]);
    j.min = static_cast<float *>(dev[1]);
    j.max = static_cast<float *>(dev[2]);
    j.excised = static_cast<float *>(dev[3]);
    j.kept = static_cast<unsigned *>(dev[4]);
    j.started = w.started;
    j.last = last;
    j.depth = h->wf_depth;
    j.rows = R;
    j.nbins = (unsigned)bins(h);
    j.sides = sides;
    j.block = h->wf_block;
    j.g = (double)(1.0f / (psdrt::stage_gain(h->n, h->wf_block, h->nenbw, h->power) * dec)); // wf_image_impl's gsc_block
    j.sk_lo = sk_lo;
    j.sk_hi = sk_hi;
    hipError_t e = launch_wf_robust(j, h->stream);
    if (e == hipSuccess) {
        ++h->launches;
        e = hipStreamSynchronize(h->stream);
    }
    for (int i = 0; i < 5 && !device; ++i)
        if (e == hipSuccess && out[i])
            e = hipMemcpy(out[i], dev[i], sizeof(float) * row, hipMemcpyDeviceToHost);
    if (tmp)
        (void)hipFree(tmp);
    XCHK(h, e);
    return PSDC_OK;
}

} // namespace

struct psdc_wf : XObj {};
struct psdc_zwf : XObj {};

extern "C" {

int psdc_wf_supported(uint32_t n) { return psdc_sk_supported(n); }

psdc_wf *psdc_wf_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, uint32_t block,
                               uint32_t depth, int device)
{
    return static_cast<psdc_wf *>(wf_create(K_WF, n, 0, win, power, nenbw, overlap, true, n_channels, block, depth, device, "psdc_wf_create_window"));
}

psdc_wf *psdc_wf_create(uint32_t n, int window_kind, uint32_t n_channels, uint32_t block, uint32_t depth, int device)
{
    return static_cast<psdc_wf *>(wf_create(K_WF, n, window_kind, nullptr, 0, 0, 0, false, n_channels, block, depth, device, "psdc_wf_create"));
}

void psdc_wf_destroy(psdc_wf *h) { destroy_obj(h); }
int psdc_wf_reset(psdc_wf *h) { return reset_impl(h, "psdc_wf_reset"); }
int psdc_wf_set_detrend(psdc_wf *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_wf_set_detrend"); }

int psdc_wf_process(psdc_wf *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return process_impl(h, channel, xs, SampleFmt{}, len, "psdc_wf_process");
}

int psdc_wf_process_device(psdc_wf *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return process_device_impl(h, channel, xs, SampleFmt{}, len, producer_event, "psdc_wf_process_device");
}

int psdc_wf_sync(psdc_wf *h) { return sync_impl(h, "psdc_wf_sync"); }
int psdc_wf_num_stages(psdc_wf *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_wf_num_stages"); }

int psdc_wf_stage_blocks(psdc_wf *h, uint32_t channel, uint32_t stage, psdc_wf_blocks *out)
{
    return wf_stage_blocks_impl(h, channel, stage, out, "psdc_wf_stage_blocks");
}

int psdc_wf_stage_rows(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, uint64_t *block_index, uint32_t *counts, double *s1,
                       double *s2, uint32_t *n_rows)
{
    double *const outs[SK_ROWS] = {s1, s2};
    return wf_stage_rows_impl(h, channel, stage, max_rows, block_index, counts, outs, n_rows, "psdc_wf_stage_rows");
}

int psdc_wf_image(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *psd, float *sk, uint64_t *block_index,
                  uint32_t *counts, uint32_t *n_rows)
{
    return wf_image_impl(h, channel, stage, max_rows, psd, sk, false, block_index, counts, n_rows, "psdc_wf_image");
}

int psdc_wf_image_device(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *d_psd, float *d_sk, uint64_t *block_index,
                         uint32_t *counts, uint32_t *n_rows)
{
    return wf_image_impl(h, channel, stage, max_rows, d_psd, d_sk, true, block_index, counts, n_rows, "psdc_wf_image_device");
}

int psdc_wf_stats_read(psdc_wf *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_wf_stats_read");
}

const char *psdc_wf_last_error(const psdc_wf *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

int psdc_zwf_supported(uint32_t n) { return psdc_zsk_supported(n); }

psdc_zwf *psdc_zwf_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels, uint32_t block,
                                 uint32_t depth, int device)
{
    return static_cast<psdc_zwf *>(wf_create(K_ZWF, n, 0, win, power, nenbw, overlap, true, n_channels, block, depth, device, "psdc_zwf_create_window"));
}

psdc_zwf *psdc_zwf_create(uint32_t n, int window_kind, uint32_t n_channels, uint32_t block, uint32_t depth, int device)
{
    return static_cast<psdc_zwf *>(wf_create(K_ZWF, n, window_kind, nullptr, 0, 0, 0, false, n_channels, block, depth, device, "psdc_zwf_create"));
}

void psdc_zwf_destroy(psdc_zwf *h) { destroy_obj(h); }
int psdc_zwf_reset(psdc_zwf *h) { return reset_impl(h, "psdc_zwf_reset"); }
int psdc_zwf_set_detrend(psdc_zwf *h, int detrend_kind) { return set_detrend_impl(h, detrend_kind, "psdc_zwf_set_detrend"); }

int psdc_zwf_set_carrier(psdc_zwf *h, uint32_t channel, uint64_t ftw, uint64_t phase0)
{
    return set_carrier_impl(h, channel, ftw, phase0, "psdc_zwf_set_carrier");
}

int psdc_zwf_process(psdc_zwf *h, uint32_t channel, const float *x, size_t len)
{
    const void *xs[1] = {x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, false, nullptr, "psdc_zwf_process");
}

int psdc_zwf_process_device(psdc_zwf *h, uint32_t channel, const float *d_x, size_t len, void *producer_event)
{
    const void *xs[1] = {d_x};
    return zoom_feed(h, channel, xs, SampleFmt{}, len, true, producer_event, "psdc_zwf_process_device");
}

int psdc_zwf_sync(psdc_zwf *h) { return sync_impl(h, "psdc_zwf_sync"); }
int psdc_zwf_num_stages(psdc_zwf *h, uint32_t channel) { return num_stages_impl(h, channel, "psdc_zwf_num_stages"); }

int psdc_zwf_stage_blocks(psdc_zwf *h, uint32_t channel, uint32_t stage, psdc_wf_blocks *out)
{
    return wf_stage_blocks_impl(h, channel, stage, out, "psdc_zwf_stage_blocks");
}

int psdc_zwf_stage_rows(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, uint64_t *block_index, uint32_t *counts,
                        double *s1_upper, double *s1_lower, double *s2_upper, double *s2_lower, uint32_t *n_rows)
{
    double *const outs[ZSK_ROWS] = {s1_upper, s1_lower, s2_upper, s2_lower};
    return wf_stage_rows_impl(h, channel, stage, max_rows, block_index, counts, outs, n_rows, "psdc_zwf_stage_rows");
}

int psdc_zwf_image(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *psd, float *sk, uint64_t *block_index,
                   uint32_t *counts, uint32_t *n_rows)
{
    return wf_image_impl(h, channel, stage, max_rows, psd, sk, false, block_index, counts, n_rows, "psdc_zwf_image");
}

int psdc_zwf_image_device(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *d_psd, float *d_sk,
                          uint64_t *block_index, uint32_t *counts, uint32_t *n_rows)
{
    return wf_image_impl(h, channel, stage, max_rows, d_psd, d_sk, true, block_index, counts, n_rows, "psdc_zwf_image_device");
}

int psdc_zwf_stats_read(psdc_zwf *h, uint64_t *launches, uint64_t *samples_in, int reset)
{
    return stats_impl(h, launches, samples_in, reset, "psdc_zwf_stats_read");
}

const char *psdc_zwf_last_error(const psdc_zwf *h) { return h ? h->err.c_str() : x_last_error.c_str(); }

// ---- the robust read-outs of include/psdcascade_robust.h ----

int psdcx_wf_robust(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *median, float *min,
                    float *max, float *excised, uint32_t *kept, psdcx_robust_info *info)
{
    return wf_robust_impl(h, channel, stage, max_rows, sk_lo, sk_hi, median, min, max, excised, kept, false, info, "psdcx_wf_robust");
}

int psdcx_wf_robust_device(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *d_median,
                           float *d_min, float *d_max, float *d_excised, uint32_t *d_kept, psdcx_robust_info *info)
{
    return wf_robust_impl(h, channel, stage, max_rows, sk_lo, sk_hi, d_median, d_min, d_max, d_excised, d_kept, true, info,
                          "psdcx_wf_robust_device");
}

int psdcx_zwf_robust(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *median, float *min,
                     float *max, float *excised, uint32_t *kept, psdcx_robust_info *info)
{
    return wf_robust_impl(h, channel, stage, max_rows, sk_lo, sk_hi, median, min, max, excised, kept, false, info, "psdcx_zwf_robust");
}

int psdcx_zwf_robust_device(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *d_median,
                            float *d_min, float *d_max, float *d_excised, uint32_t *d_kept, psdcx_robust_info *info)
{
    return wf_robust_impl(h, channel, stage, max_rows, sk_lo, sk_hi, d_median, d_min, d_max, d_excised, d_kept, true, info,
                          "psdcx_zwf_robust_device");
}

} // extern "C"

// ---- the bank read-outs of include/psdcascade_crossread.h (pair and matrix objects) ----
// One drain, the stitch of every selected unit planned on the host from XStage's bookkeeping (stitch_impl without an output row
// gives the Breaks, cross_readout.h turns them into jobs), one launch of cross_stitch_kernel and at most one of cross_band_kernel
// (cross_readout.hip) behind the drain on the object's stream.

namespace {

struct XrArgs {
    const char *who;
    const uint32_t *sel;
    uint32_t n_sel;
    int keep_overlap;
    uint32_t min_count;
    int keep_transition_band;
    size_t *lens, *n_breaks;
    psdc_break *breaks;
    size_t breaks_cap;
    psdcxr_info *info;
};

// one output of a call: `rows` rows a unit of `elem` bytes a bin each; p is the caller's memory (NULL: not wanted)
struct XrOut {
    void *p;
    size_t elem;
    uint32_t rows;
};

// which kernels a call runs: the pair and matrix forms of cross_readout.hip (psdcxr_*), a mode of carrier_readout.hip (psdczr_*),
// or a mode of pair_readout.hip (psdcpr_*)
enum class XrMode { PAIR, ROWS, SIDES, SK, AMPM, PCSD, PAMPM };
bool xr_pair_carrier_mode(XrMode m) { return m == XrMode::PCSD || m == XrMode::PAMPM; }
// the modes whose kernels take CarrierReadJob and whose launches count in the object's stats_read
bool xr_carrier_mode(XrMode m) { return m == XrMode::SIDES || m == XrMode::SK || m == XrMode::AMPM || xr_pair_carrier_mode(m); }
// rows of a band sum (0: the mode has no bands)
uint32_t xr_band_rows(XrMode m)
{
    if (xr_pair_carrier_mode(m))
        return PREAD_BAND_ROWS;
    return m == XrMode::PAIR || m == XrMode::AMPM ? XREAD_PAIR_ROWS : m == XrMode::SIDES ? CREAD_SIDE_ROWS : 0;
}
// f64 values of a carrier record
uint32_t xr_record(XrMode m) { return m == XrMode::PAMPM ? PREAD_RECORD : 4; }
constexpr size_t XR_MAX_OUTS = 11; // the outputs of psdcpr_csd

// what an AM/PM call adds: the given carriers on the host (AMPM: the amplitudes [S][2]; PAMPM: [S][5] = p_ab, w, q; NULL: from bin 0
// of stage 0) and the carrier records [S][4] or [S][7] (NULL: not wanted; device or host memory as the call's other outputs)
struct XrCarrier {
    const double *carriers;
    double *out;
};

struct XrPlan {
    std::vector<CarrierReadJob> jobs; // (the pair and matrix forms send the CrossReadJob of each)
    std::vector<BankRow> units;
    std::vector<CarrierUnit> cunits; // AM/PM alone
    std::vector<PairUnit> punits;    // pair AM/PM alone
    size_t max_len = 0;
    uint32_t max_bins = 0;
};

int xr_bad(XObj *h, const XrArgs &a, const char *what) { return xfail(h, PSDC_ERR_ARG, std::string(a.who) + ": " + what); }

// the checks every call shares; *units = the number of selected units
int xr_selection(XObj *h, const XrArgs &a, uint32_t *units)
{
    X_HANDLE(h, a.who);
    if (const char *why = cross_read_layout_refusal(a.lens, a.n_breaks, a.breaks))
        return xr_bad(h, a, why);
    const uint32_t S = a.sel ? a.n_sel : h->n_pairs;
    if (S > BANK_MAX_ROWS)
        return xr_bad(h, a, "more than PSDCXR_MAX_ROWS units selected");
    for (uint32_t i = 0; a.sel && i < S; ++i)
        if (int rc = check_pair(h, a.sel[i], a.who))
            return rc;
    *units = S;
    return PSDC_OK;
}

// Drain, then the layout of every selected unit and its jobs.  Fills lens, n_breaks, info->max_len and info->jobs always, the
// Breaks where they fit; PSDC_ERR_CAPACITY when some unit's Breaks do not.
int xr_plan(XObj *h, const XrArgs &a, uint32_t S, XrPlan *pl)
{
    int rc = drain(h);
    if (rc)
        return rc;
    bool overflow = false;
    pl->units.resize(S);
    for (uint32_t i = 0; i < S; ++i) {
        const std::vector<XStage> &st = h->pairs[a.sel ? a.sel[i] : i];
        UnitSnap in; // (the bookkeeping alone: the kernels read the accumulators where they lie)
        unit_layout(h, a.sel ? a.sel[i] : i, &in);
        uint32_t counts[X_MAX_STAGES];
        for (uint32_t k = 0; k < in.ns; ++k)
            counts[k] = count_report(in.c64[k]);
        psdc_break br[X_MAX_STAGES];
        size_t len = 0, nb = 0;
        rc = psdrt::stitch_impl(h->n, h->nenbw, h->power, h->geo.overlap, in.ns, counts, in.avgs.data(), in.pend.data(), nullptr, a.keep_overlap,
                                a.min_count, a.keep_transition_band, nullptr, 0, &len, br, X_MAX_STAGES, &nb, in.c64.data());
        if (rc)
            return xfail(h, rc, std::string(a.who) + ": internal: a unit with more than 16 stages");
        a.lens[i] = len;
        if (a.n_breaks)
            a.n_breaks[i] = nb;
        if (a.breaks) {
            if (nb <= a.breaks_cap)
                memcpy(a.breaks + (size_t)i * a.breaks_cap, br, sizeof(psdc_break) * nb);
            else
                overflow = true;
        }
        pl->units[i] = cross_row_jobs(
            br, nb, i, h->rows(), (uint32_t)bins(h), pl->jobs, [&](uint32_t stage) { return (const double *)st[stage].acc; },
            [&](uint32_t stage) { return psdrt::stage_gain(h->n, in.c64[stage], h->nenbw, h->power); });
        if (pl->units[i].len != len)
            return xfail(h, PSDC_ERR_ARG, std::string(a.who) + ": internal: the jobs do not cover the row");
        pl->max_len = std::max(pl->max_len, len);
    }
    for (const CrossReadJob &j : pl->jobs)
        pl->max_bins = std::max(pl->max_bins, j.bins_end - j.bins_start);
    if (a.info) {
        a.info->launches = 0;
        a.info->jobs = (uint32_t)pl->jobs.size();
        a.info->max_len = pl->max_len;
    }
    return overflow ? xfail(h, PSDC_ERR_CAPACITY, std::string(a.who) + ": breaks_cap is smaller than a unit's number of breaks") : PSDC_OK;
}

int xr_layout(XObj *h, const XrArgs &a)
{
    uint32_t S = 0;
    int rc = xr_selection(h, a, &S);
    if (rc)
        return rc;
    X_ON_DEVICE(h);
    XrPlan pl;
    return xr_plan(h, a, S, &pl);
}

// The kernels of one call into the device memory dev[]: the table through a free slot, the stitch, the bands, the slot's event.
// PAIR: dev[] = sxx, syy, sxy, freq, coherence, transfer; ROWS: rows, freq; SIDES: upper, lower, freq; SK: those and sk_upper,
// sk_lower; AM/PM: those three and s_am, s_pm, s_ampm, with the carrier records to d_carrier; PCSD: PairCsdOut's eleven in order;
// PAMPM: PairAmPmOut's seven in order, with the carrier records to d_carrier.
int xr_enqueue(XObj *h, const XrArgs &a, const XrPlan &pl, XrMode mode, void *const *dev, size_t stride, const BankBands &bb, double *d_band,
               double *d_carrier)
{
    const uint32_t S = (uint32_t)pl.units.size();
    const bool records = d_carrier && S; // (a channel without an included stage still gets its record)
    if (pl.jobs.empty() && d_band && S) // nothing included anywhere: no band kernel; the band sums are 0.0
        XCHK(h, hipMemsetAsync(d_band, 0, sizeof(double) * S * bb.n * xr_band_rows(mode), h->stream));
    if (pl.jobs.empty() && !records)
        return PSDC_OK;
    if (!h->bank_read)
        h->bank_read = new psdrt::BankRead;
    psdrt::BankRead *st = h->bank_read;
    const bool carrier = xr_carrier_mode(mode);
    const size_t job_size = carrier ? sizeof(CarrierReadJob) : sizeof(CrossReadJob);
    const size_t job_bytes = job_size * pl.jobs.size(), unit_bytes = sizeof(BankRow) * S, cunit_bytes = sizeof(CarrierUnit) * pl.cunits.size();
    const size_t punit_bytes = sizeof(PairUnit) * pl.punits.size(); // (a call has units of one kind at most)
    const size_t bytes = job_bytes + unit_bytes + cunit_bytes + punit_bytes;
    int s = 0;
    XCHK(h, st->take_slot(bytes, &s));
    // The plan keeps one job type for every mode, the 48-byte CarrierReadJob.  The carrier kernels take the vector as it lies; the
    // pair and matrix kernels take CrossReadJob, so their table is packed here from the 40-byte base of each job: the bytes the
    // device saw before, for a copy of 40 bytes a job (a few dozen jobs a call) into pinned memory instead of one memcpy.
    if (carrier)
        memcpy(st->h_tab[s], pl.jobs.data(), job_bytes);
    else
        for (size_t i = 0; i < pl.jobs.size(); ++i)
            memcpy(st->h_tab[s] + i * job_size, &static_cast<const CrossReadJob &>(pl.jobs[i]), job_size);
    memcpy(st->h_tab[s] + job_bytes, pl.units.data(), unit_bytes);
    if (cunit_bytes)
        memcpy(st->h_tab[s] + job_bytes + unit_bytes, pl.cunits.data(), cunit_bytes);
    if (punit_bytes)
        memcpy(st->h_tab[s] + job_bytes + unit_bytes + cunit_bytes, pl.punits.data(), punit_bytes);
    XCHK(h, hipMemcpyAsync(st->d_tab[s], st->h_tab[s], bytes, hipMemcpyHostToDevice, h->stream));
    const CrossReadJob *d_jobs = reinterpret_cast<const CrossReadJob *>(st->d_tab[s]);
    const CarrierReadJob *d_cjobs = reinterpret_cast<const CarrierReadJob *>(st->d_tab[s]);
    const BankRow *d_units = reinterpret_cast<const BankRow *>(st->d_tab[s] + job_bytes);
    const CarrierUnit *d_cunits = cunit_bytes ? reinterpret_cast<const CarrierUnit *>(st->d_tab[s] + job_bytes + unit_bytes) : nullptr;
    const PairUnit *d_punits = punit_bytes ? reinterpret_cast<const PairUnit *>(st->d_tab[s] + job_bytes + unit_bytes + cunit_bytes) : nullptr;
    const uint32_t n_jobs = (uint32_t)pl.jobs.size();
    uint32_t launches = 0;
    if (mode == XrMode::PCSD) {
        const PairCsdOut o{(float *)dev[0], (float *)dev[1], (float *)dev[2],  (float *)dev[3],  (float *)dev[4],  (float *)dev[5],
                           (float *)dev[6], (double *)dev[7], (double *)dev[8], (double *)dev[9], (double *)dev[10], stride};
        if (o.any_row() && n_jobs) {
            XCHK(h, launch_pair_stitch_csd(d_cjobs, n_jobs, pl.max_bins, o, h->stream));
            ++launches;
        }
    } else if (mode == XrMode::PAMPM) {
        const PairAmPmOut o{(float *)dev[0], (double *)dev[1], (double *)dev[2], (double *)dev[3], (double *)dev[4],
                            (double *)dev[5], (double *)dev[6], d_carrier,        stride};
        if ((o.any_row() && n_jobs) || records) {
            XCHK(h, launch_pair_stitch_ampm(d_cjobs, n_jobs, pl.max_bins, o, d_punits, S, h->stream));
            ++launches;
        }
    } else if (mode == XrMode::PAIR) {
        const CrossPairOut o{(float *)dev[0], (float *)dev[1], (float *)dev[2], (float *)dev[3], (double *)dev[4], (double *)dev[5], stride};
        if (o.any()) {
            XCHK(h, launch_cross_stitch_pair(d_jobs, n_jobs, pl.max_bins, o, h->stream));
            ++launches;
        }
    } else if (mode == XrMode::ROWS) {
        if (dev[0] || dev[1]) {
            XCHK(h, launch_cross_stitch_rows(d_jobs, n_jobs, pl.max_bins, (float *)dev[0], (float *)dev[1], stride, h->stream));
            ++launches;
        }
    } else {
        CarrierOut o{(float *)dev[0], (float *)dev[1], (float *)dev[2], nullptr, nullptr, nullptr, nullptr, nullptr, d_carrier, stride};
        if (mode == XrMode::SK) {
            o.sk_upper = (double *)dev[3];
            o.sk_lower = (double *)dev[4];
        } else if (mode == XrMode::AMPM) {
            o.s_am = (double *)dev[3];
            o.s_pm = (double *)dev[4];
            o.s_ampm = (double *)dev[5];
        }
        if ((o.any_row() && n_jobs) || records) {
            const int km = mode == XrMode::SK ? CREAD_SK : mode == XrMode::AMPM ? CREAD_AMPM : CREAD_SIDES;
            XCHK(h, launch_carrier_stitch(km, d_cjobs, n_jobs, pl.max_bins, o, d_cunits, S, h->stream));
            ++launches;
        }
    }
    if (d_band && n_jobs) {
        if (xr_pair_carrier_mode(mode))
            XCHK(h, launch_pair_band(mode == XrMode::PAMPM ? PREAD_AMPM : PREAD_CSD, d_cjobs, d_units, d_punits, S, bb, d_band, h->stream));
        else if (carrier)
            XCHK(h, launch_carrier_band(xr_band_rows(mode), d_cjobs, d_units, d_cunits, S, bb, d_band, h->stream));
        else
            XCHK(h, launch_cross_band(d_jobs, d_units, S, bb, d_band, h->stream));
        ++launches;
    }
    XCHK(h, st->mark_slot(s, h->stream));
    if (carrier)
        h->launches += launches;
    if (a.info)
        a.info->launches = launches;
    return PSDC_OK;
}

// One read-out call of either object in either form.  device: outs[].p and band_out are device memory, else host memory filled
// from the object's buffer through one copy.
int xr_read(XObj *h, const XrArgs &a, XrMode mode, const XrOut *outs, size_t n_outs, size_t stride, const float *bands, uint32_t n_bands,
            double *band_out, bool device, void *done_event, const XrCarrier *car = nullptr)
{
    uint32_t S = 0;
    int rc = xr_selection(h, a, &S);
    if (rc)
        return rc;
    bool any = false;
    for (size_t o = 0; o < n_outs; ++o)
        any = any || outs[o].p;
    double *carrier_out = car ? car->out : nullptr;
    BankBands bb{};
    if (const char *why = cross_read_band_refusal(bands, n_bands, band_out, any || carrier_out, &bb))
        return xr_bad(h, a, why);
    XrPlan pl;
    if (mode == XrMode::AMPM) { // the refusals of the carrier that the host knows: nothing is drained, nothing launched
        const bool split = outs[3].p || outs[4].p || outs[5].p || carrier_out || band_out;
        if (!car->carriers && split && h->detrend != PSDC_DETREND_NONE)
            return xr_bad(h, a, "bin 0 holds the carrier under PSDC_DETREND_NONE only: pass the carriers");
        CarrierUnit u{};
        u.n2p = (double)h->n * (double)h->n * (double)h->power;
        u.bins = (uint32_t)bins(h);
        pl.cunits.assign(S, u);
        for (uint32_t i = 0; car->carriers && i < S; ++i)
            if (const char *why = carrier_given(car->carriers[2 * i], car->carriers[2 * i + 1], &pl.cunits[i]))
                return xr_bad(h, a, why);
    }
    if (mode == XrMode::PAMPM) { // the same for the carriers of a pair
        const bool split = outs[3].p || outs[4].p || outs[5].p || outs[6].p || carrier_out || band_out;
        if (!car->carriers && split && h->detrend != PSDC_DETREND_NONE)
            return xr_bad(h, a, "bin 0 holds the carrier under PSDC_DETREND_NONE only: pass the carriers");
        PairUnit u{};
        u.n2p = (double)h->n * (double)h->n * (double)h->power;
        u.bins = (uint32_t)bins(h);
        pl.punits.assign(S, u);
        for (uint32_t i = 0; car->carriers && i < S; ++i)
            if (const char *why = pair_given(car->carriers + 5 * (size_t)i, &pl.punits[i]))
                return xr_bad(h, a, why);
    }
    X_ON_DEVICE(h);
    if ((rc = xr_plan(h, a, S, &pl)))
        return rc;
    if (any && stride < pl.max_len)
        return xfail(h, PSDC_ERR_CAPACITY, std::string(a.who) + ": stride is smaller than the longest row");
    for (uint32_t i = 0; i < (uint32_t)pl.cunits.size(); ++i) { // (drained: stage 0 of each selected channel as it lies)
        const std::vector<XStage> &st = h->pairs[a.sel ? a.sel[i] : i];
        pl.cunits[i].src0 = st.empty() ? nullptr : st[0].acc;
        pl.cunits[i].count0 = st.empty() ? 0 : count_report(st[0].count64);
    }
    for (uint32_t i = 0; i < (uint32_t)pl.punits.size(); ++i) {
        const std::vector<XStage> &st = h->pairs[a.sel ? a.sel[i] : i];
        pl.punits[i].src0 = st.empty() ? nullptr : st[0].acc;
        pl.punits[i].count0 = st.empty() ? 0 : count_report(st[0].count64);
    }
    void *dev[XR_MAX_OUTS] = {};
    if (device) {
        for (size_t o = 0; o < n_outs; ++o)
            dev[o] = outs[o].p;
        if ((rc = xr_enqueue(h, a, pl, mode, dev, stride, bb, band_out, carrier_out)))
            return rc;
        if (done_event)
            XCHK(h, hipEventRecord(static_cast<hipEvent_t>(done_event), h->stream));
        else
            XCHK(h, hipStreamSynchronize(h->stream));
        return PSDC_OK;
    }
    const size_t band_bytes = sizeof(double) * S * n_bands * xr_band_rows(mode);
    const size_t carrier_bytes = carrier_out ? sizeof(double) * xr_record(mode) * S : 0;
    if (pl.jobs.empty() && !carrier_bytes) { // nothing included anywhere: no row gets a value, the band sums are 0.0
        if (band_out)
            memset(band_out, 0, band_bytes);
        return PSDC_OK;
    }
    // the object's buffer: the wanted outputs one behind the other in rows of max_len bins, then the band sums and the carrier records
    size_t off[XR_MAX_OUTS] = {}, bytes = 0;
    for (size_t o = 0; o < n_outs; ++o) {
        off[o] = bytes;
        if (outs[o].p)
            bytes += (outs[o].elem * outs[o].rows * S * pl.max_len + 15) & ~(size_t)15;
    }
    const size_t o_band = bytes, o_carrier = bytes + band_bytes;
    bytes += band_bytes + carrier_bytes;
    if (!h->bank_read)
        h->bank_read = new psdrt::BankRead;
    psdrt::BankRead *st = h->bank_read;
    XCHK(h, st->room_out(bytes));
    for (size_t o = 0; o < n_outs; ++o)
        dev[o] = outs[o].p ? st->d_out + off[o] : nullptr;
    if ((rc = xr_enqueue(h, a, pl, mode, dev, pl.max_len, bb, band_out ? reinterpret_cast<double *>(st->d_out + o_band) : nullptr,
                         carrier_out ? reinterpret_cast<double *>(st->d_out + o_carrier) : nullptr)))
        return rc;
    XCHK(h, hipMemcpyAsync(st->h_out, st->d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    XCHK(h, hipStreamSynchronize(h->stream));
    for (size_t o = 0; o < n_outs; ++o)
        for (size_t r = 0; outs[o].p && r < (size_t)S * outs[o].rows; ++r)
            memcpy(static_cast<char *>(outs[o].p) + r * stride * outs[o].elem, st->h_out + off[o] + r * pl.max_len * outs[o].elem,
                   outs[o].elem * pl.units[r / outs[o].rows].len);
    if (band_out)
        memcpy(band_out, st->h_out + o_band, band_bytes);
    if (carrier_out)
        memcpy(carrier_out, st->h_out + o_carrier, carrier_bytes);
    return PSDC_OK;
}

// the handle of a psdczr_ call: one of the six single-channel carrier kinds (need: 0 any of them, 1 an SK kind, 2 an AM/PM kind)
int zr_handle(XObj *h, const char *who, int need)
{
    X_HANDLE(h, who);
    const size_t k = (size_t)(h->kind - KINDS);
    const bool sides = k == K_ZOOM || k == K_IQ, sk = k == K_ZSK || k == K_IQSK, ampm = k == K_ZAMPM || k == K_IQAMPM;
    if (need == 1 ? sk : need == 2 ? ampm : sides || sk || ampm)
        return PSDC_OK;
    return xfail(h, PSDC_ERR_ARG, std::string(who) + (need == 1   ? ": takes a zoom SK or IQ SK object"
                                                     : need == 2 ? ": takes a zoom AM/PM or IQ AM/PM object"
                                                                 : ": takes a zoom, IQ, zoom / IQ SK or zoom / IQ AM/PM object"));
}

// the handle of a psdcpr_ call: one of the four pair carrier kinds (ampm: a 12-row kind)
int pr_handle(XObj *h, const char *who, bool ampm)
{
    X_HANDLE(h, who);
    const size_t k = (size_t)(h->kind - KINDS);
    const bool csd = k == K_ZCSD || k == K_IQCSD, xampm = k == K_ZXAMPM || k == K_IQXAMPM;
    if (ampm ? xampm : csd || xampm)
        return PSDC_OK;
    return xfail(h, PSDC_ERR_ARG, std::string(who) + (ampm ? ": takes a zoom AM/PM cross or IQ AM/PM cross object"
                                                           : ": takes a zoom cross, IQ cross or zoom / IQ AM/PM cross object"));
}

int xr_release(XObj *h, const char *who)
{
    X_HANDLE(h, who);
    X_ON_DEVICE(h);
    delete h->bank_read; // (waits for the slots still in flight)
    h->bank_read = nullptr;
    return PSDC_OK;
}

} // namespace

extern "C" {

int psdcxr_cross_layout(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                        int keep_transition_band, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info)
{
    return xr_layout(h, {"psdcxr_cross_layout", pairs, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info});
}

int psdcxr_cross_csd_device(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                            int keep_transition_band, float *d_sxx, float *d_syy, float *d_sxy, float *d_freq, double *d_coherence,
                            double *d_transfer, size_t stride, const float *bands, uint32_t n_bands, double *d_band_sums, void *done_event,
                            size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info)
{
    const XrOut outs[6] = {{d_sxx, 4, 1}, {d_syy, 4, 1}, {d_sxy, 8, 1}, {d_freq, 4, 1}, {d_coherence, 8, 1}, {d_transfer, 16, 1}};
    return xr_read(h, {"psdcxr_cross_csd_device", pairs, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info},
                   XrMode::PAIR, outs, 6, stride, bands, n_bands, d_band_sums, true, done_event);
}

int psdcxr_cross_csd(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                     float *sxx, float *syy, float *sxy, float *freq, double *coherence, double *transfer, size_t stride, const float *bands,
                     uint32_t n_bands, double *band_sums, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                     psdcxr_info *info)
{
    const XrOut outs[6] = {{sxx, 4, 1}, {syy, 4, 1}, {sxy, 8, 1}, {freq, 4, 1}, {coherence, 8, 1}, {transfer, 16, 1}};
    return xr_read(h, {"psdcxr_cross_csd", pairs, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info},
                   XrMode::PAIR, outs, 6, stride, bands, n_bands, band_sums, false, nullptr);
}

int psdcxr_cross_release(psdc_cross *h) { return xr_release(h, "psdcxr_cross_release"); }

int psdcxr_csm_layout(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                      size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info)
{
    return xr_layout(h, {"psdcxr_csm_layout", groups, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info});
}

int psdcxr_csm_rows_device(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                           int keep_transition_band, float *d_rows, float *d_freq, size_t stride, void *done_event, size_t *lens,
                           size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info)
{
    const XrOut outs[2] = {{d_rows, 4, h ? h->rows() : 0}, {d_freq, 4, 1}};
    return xr_read(h, {"psdcxr_csm_rows_device", groups, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info},
                   XrMode::ROWS, outs, 2, stride, nullptr, 0, nullptr, true, done_event);
}

int psdcxr_csm_rows(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                    float *rows, float *freq, size_t stride, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                    psdcxr_info *info)
{
    const XrOut outs[2] = {{rows, 4, h ? h->rows() : 0}, {freq, 4, 1}};
    return xr_read(h, {"psdcxr_csm_rows", groups, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info},
                   XrMode::ROWS, outs, 2, stride, nullptr, 0, nullptr, false, nullptr);
}

int psdcxr_csm_release(psdc_csm *h) { return xr_release(h, "psdcxr_csm_release"); }

// ---- the bank read-outs of include/psdcascade_carrierread.h (zoom, IQ, zoom / IQ SK and zoom / IQ AM/PM objects) ----
// The same plan and the same two table slots; the jobs carry their Break's count, an AM/PM call adds one unit record a channel
// (carrier_readout.h), the kernels are those of carrier_readout.hip.

#define ZR_ARGS(name) {name, channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info}

int psdczr_layout(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_layout", 0))
        return rc;
    return xr_layout(x, ZR_ARGS("psdczr_layout"));
}

int psdczr_sides_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                        float *d_upper, float *d_lower, float *d_freq, size_t stride, const float *bands, uint32_t n_bands,
                        double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                        psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_sides_device", 0))
        return rc;
    const XrOut outs[3] = {{d_upper, 4, 1}, {d_lower, 4, 1}, {d_freq, 4, 1}};
    return xr_read(x, ZR_ARGS("psdczr_sides_device"), XrMode::SIDES, outs, 3, stride, bands, n_bands, d_band_sums, true, done_event);
}

int psdczr_sides(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                 float *upper, float *lower, float *freq, size_t stride, const float *bands, uint32_t n_bands, double *band_sums,
                 size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_sides", 0))
        return rc;
    const XrOut outs[3] = {{upper, 4, 1}, {lower, 4, 1}, {freq, 4, 1}};
    return xr_read(x, ZR_ARGS("psdczr_sides"), XrMode::SIDES, outs, 3, stride, bands, n_bands, band_sums, false, nullptr);
}

int psdczr_sk_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                     float *d_upper, float *d_lower, float *d_freq, double *d_sk_upper, double *d_sk_lower, size_t stride,
                     void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_sk_device", 1))
        return rc;
    const XrOut outs[5] = {{d_upper, 4, 1}, {d_lower, 4, 1}, {d_freq, 4, 1}, {d_sk_upper, 8, 1}, {d_sk_lower, 8, 1}};
    return xr_read(x, ZR_ARGS("psdczr_sk_device"), XrMode::SK, outs, 5, stride, nullptr, 0, nullptr, true, done_event);
}

int psdczr_sk(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
              float *upper, float *lower, float *freq, double *sk_upper, double *sk_lower, size_t stride, size_t *lens, size_t *n_breaks,
              psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_sk", 1))
        return rc;
    const XrOut outs[5] = {{upper, 4, 1}, {lower, 4, 1}, {freq, 4, 1}, {sk_upper, 8, 1}, {sk_lower, 8, 1}};
    return xr_read(x, ZR_ARGS("psdczr_sk"), XrMode::SK, outs, 5, stride, nullptr, 0, nullptr, false, nullptr);
}

int psdczr_ampm_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                       const double *carriers, float *d_upper, float *d_lower, float *d_freq, double *d_s_am, double *d_s_pm,
                       double *d_s_ampm, double *d_carrier, size_t stride, const float *bands, uint32_t n_bands, double *d_band_sums,
                       void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_ampm_device", 2))
        return rc;
    const XrOut outs[6] = {{d_upper, 4, 1}, {d_lower, 4, 1}, {d_freq, 4, 1}, {d_s_am, 8, 1}, {d_s_pm, 8, 1}, {d_s_ampm, 16, 1}};
    const XrCarrier car{carriers, d_carrier};
    return xr_read(x, ZR_ARGS("psdczr_ampm_device"), XrMode::AMPM, outs, 6, stride, bands, n_bands, d_band_sums, true, done_event, &car);
}

int psdczr_ampm(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                const double *carriers, float *upper, float *lower, float *freq, double *s_am, double *s_pm, double *s_ampm,
                double *carrier, size_t stride, const float *bands, uint32_t n_bands, double *band_sums, size_t *lens, size_t *n_breaks,
                psdc_break *breaks, size_t breaks_cap, psdczr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_ampm", 2))
        return rc;
    const XrOut outs[6] = {{upper, 4, 1}, {lower, 4, 1}, {freq, 4, 1}, {s_am, 8, 1}, {s_pm, 8, 1}, {s_ampm, 16, 1}};
    const XrCarrier car{carriers, carrier};
    return xr_read(x, ZR_ARGS("psdczr_ampm"), XrMode::AMPM, outs, 6, stride, bands, n_bands, band_sums, false, nullptr, &car);
}

int psdczr_release(void *h)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = zr_handle(x, "psdczr_release", 0))
        return rc;
    return xr_release(x, "psdczr_release");
}
#undef ZR_ARGS

// ---- the bank read-outs of include/ext/psdcascade_pairread.h (zoom cross, IQ cross and zoom / IQ AM/PM cross objects) ----
// The same plan, jobs and table slots; an AM/PM call adds one unit record a pair (pair_readout.h), the kernels are those of
// pair_readout.hip.

#define PR_ARGS(name) {name, pairs, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info}
#define PR_CSD_OUTS(p) \
    {{p##saa_up, 4, 1}, {p##saa_lo, 4, 1}, {p##sbb_up, 4, 1}, {p##sbb_lo, 4, 1}, {p##sab_up, 8, 1}, {p##sab_lo, 8, 1}, \
     {p##freq, 4, 1},   {p##coh_up, 8, 1}, {p##coh_lo, 8, 1}, {p##h1_up, 16, 1}, {p##h1_lo, 16, 1}}
#define PR_AMPM_OUTS(p) \
    {{p##freq, 4, 1}, {p##cab, 16, 1}, {p##cba, 16, 1}, {p##s_am, 16, 1}, {p##s_pm, 16, 1}, {p##s_am_pm, 16, 1}, {p##s_pm_am, 16, 1}}

int psdcpr_layout(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_layout", false))
        return rc;
    return xr_layout(x, PR_ARGS("psdcpr_layout"));
}

int psdcpr_csd_device(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                      float *d_saa_up, float *d_saa_lo, float *d_sbb_up, float *d_sbb_lo, float *d_sab_up, float *d_sab_lo, float *d_freq,
                      double *d_coh_up, double *d_coh_lo, double *d_h1_up, double *d_h1_lo, size_t stride, const float *bands,
                      uint32_t n_bands, double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks,
                      size_t breaks_cap, psdcpr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_csd_device", false))
        return rc;
    const XrOut outs[11] = PR_CSD_OUTS(d_);
    return xr_read(x, PR_ARGS("psdcpr_csd_device"), XrMode::PCSD, outs, 11, stride, bands, n_bands, d_band_sums, true, done_event);
}

int psdcpr_csd(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
               float *saa_up, float *saa_lo, float *sbb_up, float *sbb_lo, float *sab_up, float *sab_lo, float *freq, double *coh_up,
               double *coh_lo, double *h1_up, double *h1_lo, size_t stride, const float *bands, uint32_t n_bands, double *band_sums,
               size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_csd", false))
        return rc;
    const XrOut outs[11] = PR_CSD_OUTS();
    return xr_read(x, PR_ARGS("psdcpr_csd"), XrMode::PCSD, outs, 11, stride, bands, n_bands, band_sums, false, nullptr);
}

int psdcpr_ampm_device(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                       const double *carriers, float *d_freq, double *d_cab, double *d_cba, double *d_s_am, double *d_s_pm,
                       double *d_s_am_pm, double *d_s_pm_am, double *d_carrier, size_t stride, const float *bands, uint32_t n_bands,
                       double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                       psdcpr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_ampm_device", true))
        return rc;
    const XrOut outs[7] = PR_AMPM_OUTS(d_);
    const XrCarrier car{carriers, d_carrier};
    return xr_read(x, PR_ARGS("psdcpr_ampm_device"), XrMode::PAMPM, outs, 7, stride, bands, n_bands, d_band_sums, true, done_event, &car);
}

int psdcpr_ampm(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                const double *carriers, float *freq, double *cab, double *cba, double *s_am, double *s_pm, double *s_am_pm,
                double *s_pm_am, double *carrier, size_t stride, const float *bands, uint32_t n_bands, double *band_sums, size_t *lens,
                size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_ampm", true))
        return rc;
    const XrOut outs[7] = PR_AMPM_OUTS();
    const XrCarrier car{carriers, carrier};
    return xr_read(x, PR_ARGS("psdcpr_ampm"), XrMode::PAMPM, outs, 7, stride, bands, n_bands, band_sums, false, nullptr, &car);
}

int psdcpr_release(void *h)
{
    XObj *x = static_cast<XObj *>(h);
    if (int rc = pr_handle(x, "psdcpr_release", false))
        return rc;
    return xr_release(x, "psdcpr_release");
}
#undef PR_ARGS
#undef PR_CSD_OUTS
#undef PR_AMPM_OUTS

} // extern "C"
