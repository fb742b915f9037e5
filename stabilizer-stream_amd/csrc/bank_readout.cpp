// bank_readout.cpp -- the bank read-out (psdcr_*, include/psdcascade_readout.h): one drain, the stitch of every selected channel
// planned on the host from its bookkeeping (stitch_impl without an output row gives the Breaks, bank_readout.h turns them into
// jobs), one launch of bank_stitch_kernel and at most one of bank_band_kernel (bank_readout.hip) behind the drain on the handle's
// stream.  The device form writes caller memory and may return before the kernels have run; the host form runs the same kernels
// into the handle's buffer and copies it out once.
#include "../../include/psdcascade_readout.h"
#include "bank_plan.h"

#include <cmath>
#include <cstring>

using namespace psdrt;

namespace psdrt {
namespace bankread { // shared with bank_var.cpp through bank_plan.h

BankRead *state_of(psdc_handle *h)
{
    if (!h->bank_read)
        h->bank_read = std::shared_ptr<void>(new BankRead, [](void *p) { delete static_cast<BankRead *>(p); });
    return static_cast<BankRead *>(h->bank_read.get());
}

int bad(psdc_handle *h, const Args &a, const char *what) { return fail(h, PSDC_ERR_ARG, std::string(a.who) + ": " + what); }

// the checks every call shares; *rows = the number of selected rows
int check_selection(psdc_handle *h, const Args &a, uint32_t *rows)
{
    if (!h)
        return bad(nullptr, a, "null handle");
    if (!a.lens)
        return bad(h, a, "null lens");
    if (a.breaks && !a.n_breaks)
        return bad(h, a, "breaks without n_breaks");
    const uint32_t S = a.channels ? a.n_sel : h->n_channels;
    if (S > psdk::BANK_MAX_ROWS)
        return bad(h, a, "more than PSDCR_MAX_ROWS rows selected");
    for (uint32_t i = 0; a.channels && i < S; ++i)
        if (a.channels[i] >= h->n_channels)
            return bad(h, a, "channel out of range");
    *rows = S;
    return PSDC_OK;
}

// Drain, then the layout of every selected row and its jobs from the host's bookkeeping.  Fills lens, n_breaks, info->max_len and
// info->jobs always, the Breaks where they fit; PSDC_ERR_CAPACITY when some row's Breaks do not.
int plan_rows(psdc_handle *h, const Args &a, uint32_t S, Plan *pl)
{
    int rc = flush_all(h);
    if (rc)
        return rc;
    bool overflow = false;
    pl->rows.resize(S);
    for (uint32_t i = 0; i < S; ++i) {
        const Channel &c = h->ch[a.channels ? a.channels[i] : i];
        const size_t ns = c.st.size();
        uint32_t counts[MAX_STAGES], avgs[MAX_STAGES];
        uint64_t pend[MAX_STAGES], counts64[MAX_STAGES];
        for (size_t k = 0; k < ns; ++k) {
            counts[k] = c.st[k].count;
            counts64[k] = c.st[k].count64;
            avgs[k] = cur_stage_avg(h, k);
            pend[k] = pending_for(h->geo, c.st[k].total);
        }
        psdc_break br[MAX_STAGES];
        size_t len = 0, nb = 0;
        rc = stitch_impl(h->n, h->nenbw, h->power, h->geo.overlap, (uint32_t)ns, counts, avgs, pend, nullptr, a.keep_overlap, a.min_count,
                         a.keep_transition_band, nullptr, 0, &len, br, MAX_STAGES, &nb, counts64);
        if (rc)
            return fail(h, rc, std::string(a.who) + ": internal: a channel with more than MAX_STAGES stages");
        a.lens[i] = len;
        if (a.n_breaks)
            a.n_breaks[i] = nb;
        if (a.breaks) {
            if (nb <= a.breaks_cap)
                memcpy(a.breaks + (size_t)i * a.breaks_cap, br, sizeof(psdc_break) * nb);
            else
                overflow = true;
        }
        pl->rows[i] = psdk::bank_row_jobs(
            br, nb, i, pl->jobs, [&](uint32_t stage) { return (const float *)c.st[stage].spectrum; },
            [&](uint32_t stage) { return stage_gain(h->n, counts64[stage], h->nenbw, h->power); });
        if (pl->rows[i].len != len)
            return fail(h, PSDC_ERR_ARG, std::string(a.who) + ": internal: the jobs do not cover the row");
        pl->max_len = std::max(pl->max_len, len);
    }
    for (const psdk::BankJob &j : pl->jobs)
        pl->max_bins = std::max(pl->max_bins, j.bins_end - j.bins_start);
    if (a.info) {
        a.info->launches = 0;
        a.info->jobs = (uint32_t)pl->jobs.size();
        a.info->max_len = pl->max_len;
    }
    return overflow ? fail(h, PSDC_ERR_CAPACITY, std::string(a.who) + ": breaks_cap is smaller than a row's number of breaks") : PSDC_OK;
}

} // namespace bankread
} // namespace psdrt

using namespace psdrt::bankread;

namespace {

int check_outputs(psdc_handle *h, const Args &a, const void *psd, const void *freq, const float *bands, uint32_t n_bands, const void *band_out,
                  psdk::BankBands *bb)
{
    if (n_bands > PSDCR_MAX_BANDS)
        return bad(h, a, "more than 8 bands");
    if (n_bands && !bands)
        return bad(h, a, "n_bands without a band list");
    if ((n_bands != 0) != (band_out != nullptr))
        return bad(h, a, n_bands ? "bands without a band output" : "a band output without bands");
    if (!psd && !freq && !band_out)
        return bad(h, a, "no output");
    bb->n = n_bands;
    for (uint32_t b = 0; b < psdk::BANK_MAX_BANDS; ++b) {
        bb->lo[b] = b < n_bands ? bands[2 * b] : 0.0f;
        bb->hi[b] = b < n_bands ? bands[2 * b + 1] : 0.0f;
        if (b < n_bands && !(bb->lo[b] <= bb->hi[b])) // (false for a NaN on either side)
            return bad(h, a, "a band with NaN or lo > hi");
    }
    return PSDC_OK;
}

// The kernels of one call into device memory: the table through a free slot, the stitch, the bands, the slot's event.
int enqueue(psdc_handle *h, const Args &a, const Plan &pl, float *d_psd, float *d_freq, size_t stride, const psdk::BankBands &bb,
            double *d_band)
{
    const uint32_t S = (uint32_t)pl.rows.size();
    if (pl.jobs.empty()) { // nothing included anywhere: no kernel; the band powers are 0.0
        if (d_band && S)
            HIPCHK(h, hipMemsetAsync(d_band, 0, sizeof(double) * S * bb.n, h->stream));
        return PSDC_OK;
    }
    BankRead *st = state_of(h);
    const size_t job_bytes = sizeof(psdk::BankJob) * pl.jobs.size(), bytes = job_bytes + sizeof(psdk::BankRow) * S;
    int s = 0;
    HIPCHK(h, st->take_slot(bytes, &s));
    memcpy(st->h_tab[s], pl.jobs.data(), job_bytes);
    memcpy(st->h_tab[s] + job_bytes, pl.rows.data(), bytes - job_bytes);
    HIPCHK(h, hipMemcpyAsync(st->d_tab[s], st->h_tab[s], bytes, hipMemcpyHostToDevice, h->stream));
    const psdk::BankJob *d_jobs = reinterpret_cast<const psdk::BankJob *>(st->d_tab[s]);
    const psdk::BankRow *d_rows = reinterpret_cast<const psdk::BankRow *>(st->d_tab[s] + job_bytes);
    uint32_t launches = 0;
    if (d_psd || d_freq) {
        HIPCHK(h, psdk::launch_bank_stitch(d_jobs, (uint32_t)pl.jobs.size(), pl.max_bins, d_psd, d_freq, stride, h->stream));
        ++launches;
    }
    if (d_band) {
        HIPCHK(h, psdk::launch_bank_band(d_jobs, d_rows, S, bb, d_band, h->stream));
        ++launches;
    }
    HIPCHK(h, st->mark_slot(s, h->stream));
    if (a.info)
        a.info->launches = launches;
    return PSDC_OK;
}

} // namespace

extern "C" {

int psdcr_bank_layout(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                      int keep_transition_band, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info)
{
    const Args a{"psdcr_bank_layout", channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info};
    uint32_t S = 0;
    int rc = check_selection(h, a, &S);
    if (rc)
        return rc;
    ON_DEVICE(h, h->device);
    Plan pl;
    return plan_rows(h, a, S, &pl);
}

int psdcr_bank_psd_device(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                          int keep_transition_band, float *d_psd, float *d_freq, size_t stride, const float *bands, uint32_t n_bands,
                          double *d_band_power, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                          psdcr_info *info)
{
    const Args a{"psdcr_bank_psd_device", channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap,
                 info};
    uint32_t S = 0;
    int rc = check_selection(h, a, &S);
    if (rc)
        return rc;
    psdk::BankBands bb{};
    if ((rc = check_outputs(h, a, d_psd, d_freq, bands, n_bands, d_band_power, &bb)))
        return rc;
    ON_DEVICE(h, h->device);
    Plan pl;
    if ((rc = plan_rows(h, a, S, &pl)))
        return rc;
    if ((d_psd || d_freq) && stride < pl.max_len)
        return fail(h, PSDC_ERR_CAPACITY, "psdcr_bank_psd_device: stride is smaller than the longest row");
    if ((rc = enqueue(h, a, pl, d_psd, d_freq, stride, bb, d_band_power)))
        return rc;
    if (done_event)
        HIPCHK(h, hipEventRecord(static_cast<hipEvent_t>(done_event), h->stream));
    else
        HIPCHK(h, hipStreamSynchronize(h->stream));
    return PSDC_OK;
}

int psdcr_bank_psd(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                   int keep_transition_band, float *psd, float *freq, size_t stride, const float *bands, uint32_t n_bands,
                   double *band_power, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info)
{
    const Args a{"psdcr_bank_psd", channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info};
    uint32_t S = 0;
    int rc = check_selection(h, a, &S);
    if (rc)
        return rc;
    psdk::BankBands bb{};
    if ((rc = check_outputs(h, a, psd, freq, bands, n_bands, band_power, &bb)))
        return rc;
    ON_DEVICE(h, h->device);
    Plan pl;
    if ((rc = plan_rows(h, a, S, &pl)))
        return rc;
    if ((psd || freq) && stride < pl.max_len)
        return fail(h, PSDC_ERR_CAPACITY, "psdcr_bank_psd: stride is smaller than the longest row");
    if (pl.jobs.empty()) { // nothing included anywhere: no row gets a value, the band powers are 0.0
        for (size_t i = 0; band_power && i < (size_t)S * n_bands; ++i)
            band_power[i] = 0.0;
        return PSDC_OK;
    }
    // the handle's buffer: [psd rows][freq rows][band sums], rows of max_len floats
    const size_t row_bytes = sizeof(float) * S * pl.max_len;
    const size_t o_freq = psd ? row_bytes : 0, o_band = (o_freq + (freq ? row_bytes : 0) + 7) & ~(size_t)7;
    const size_t bytes = o_band + sizeof(double) * S * n_bands;
    BankRead *st = state_of(h);
    HIPCHK(h, st->room_out(bytes));
    if ((rc = enqueue(h, a, pl, psd ? reinterpret_cast<float *>(st->d_out) : nullptr, freq ? reinterpret_cast<float *>(st->d_out + o_freq) : nullptr,
                      pl.max_len, bb, band_power ? reinterpret_cast<double *>(st->d_out + o_band) : nullptr)))
        return rc;
    HIPCHK(h, hipMemcpyAsync(st->h_out, st->d_out, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < S; ++i) {
        if (psd)
            memcpy(psd + (size_t)i * stride, st->h_out + sizeof(float) * i * pl.max_len, sizeof(float) * pl.rows[i].len);
        if (freq)
            memcpy(freq + (size_t)i * stride, st->h_out + o_freq + sizeof(float) * i * pl.max_len, sizeof(float) * pl.rows[i].len);
    }
    if (band_power)
        memcpy(band_power, st->h_out + o_band, sizeof(double) * S * n_bands);
    return PSDC_OK;
}

int psdcr_release(psdc_handle *h)
{
    if (!h)
        return fail(nullptr, PSDC_ERR_ARG, "psdcr_release: null handle");
    ON_DEVICE(h, h->device);
    h->bank_read.reset(); // (waits for the slots still in flight)
    return PSDC_OK;
}

} // extern "C"
