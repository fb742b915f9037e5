// bank_var.cpp -- the Var read-out (psdcv_*, include/psdcascade_var.h): the bank forms select, drain and plan as the bank read-out
// does (bank_plan.h), then one launch of bank_var_kernel (bank_var.hip) over the job table behind the drain on the handle's stream;
// the rows form launches the same kernel over caller rows without a drain.  The tables of a call -- descriptors, taus, then jobs and
// rows or the caller rows -- travel in one of the handle's two BankRead slots.
#include "../../include/psdcascade_var.h"
#include "bank_plan.h"
#include "bank_var.h"

#include <cmath>
#include <cstring>

using namespace psdrt;
using namespace psdrt::bankread;

static_assert(sizeof(psdcv_var) == sizeof(psdk::VarDesc) && PSDCV_MAX_VARS == psdk::VAR_MAX_VARS && PSDCV_MAX_TAUS == psdk::VAR_MAX_TAUS &&
                  PSDCV_MAX_EXP == psdk::VAR_MAX_EXP,
              "include/psdcascade_var.h and bank_var.h state the same limits");

namespace {

int bad(psdc_handle *h, const char *who, const char *what) { return fail(h, PSDC_ERR_ARG, std::string(who) + ": " + what); }

int check_vars(psdc_handle *h, const char *who, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus, const void *out)
{
    if (n_vars == 0 || n_vars > PSDCV_MAX_VARS)
        return bad(h, who, "n_vars must be 1 ... 4");
    if (n_taus == 0 || n_taus > PSDCV_MAX_TAUS)
        return bad(h, who, "n_taus must be 1 ... 4096");
    if (!vars)
        return bad(h, who, "null vars");
    if (!taus)
        return bad(h, who, "null taus");
    if (!out)
        return bad(h, who, "null output");
    for (uint32_t v = 0; v < n_vars; ++v) {
        if (std::abs((long)vars[v].x_exp) > PSDCV_MAX_EXP || std::abs((long)vars[v].sinx_exp) > PSDCV_MAX_EXP)
            return bad(h, who, "an exponent beyond +-16");
        if (std::isnan(vars[v].clip))
            return bad(h, who, "a NaN clip");
    }
    for (uint32_t j = 0; j < n_taus; ++j)
        if (!(taus[j] > 0.0f) || std::isinf(taus[j])) // (false for a NaN)
            return bad(h, who, "a tau that is NaN, infinite or <= 0");
    return PSDC_OK;
}

// The table of one call in a free slot: [4 descriptors][taus, padded to 8 bytes], then [jobs][rows] or [caller rows]; the kernel; the
// slot's event.  Exactly one of (jobs, rows) and vrows is given.
int enqueue(psdc_handle *h, const std::vector<psdk::BankJob> *jobs, const std::vector<psdk::BankRow> *rows, const std::vector<psdk::VarRow> *vrows,
            const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus, double *d_out)
{
    BankRead *st = state_of(h);
    const size_t o_taus = sizeof(psdk::VarDesc) * psdk::VAR_MAX_VARS, o_mid = o_taus + ((sizeof(float) * n_taus + 7) & ~(size_t)7);
    const size_t mid = vrows ? sizeof(psdk::VarRow) * vrows->size() : sizeof(psdk::BankJob) * jobs->size();
    const size_t end = vrows ? 0 : sizeof(psdk::BankRow) * rows->size();
    const size_t bytes = o_mid + mid + end;
    int s = 0;
    HIPCHK(h, st->take_slot(bytes, &s));
    memset(st->h_tab[s], 0, o_mid);
    memcpy(st->h_tab[s], vars, sizeof(psdcv_var) * n_vars);
    memcpy(st->h_tab[s] + o_taus, taus, sizeof(float) * n_taus);
    if (vrows)
        memcpy(st->h_tab[s] + o_mid, vrows->data(), mid);
    else {
        memcpy(st->h_tab[s] + o_mid, jobs->data(), mid);
        memcpy(st->h_tab[s] + o_mid + mid, rows->data(), end);
    }
    HIPCHK(h, hipMemcpyAsync(st->d_tab[s], st->h_tab[s], bytes, hipMemcpyHostToDevice, h->stream));
    const char *d = st->d_tab[s];
    const uint32_t n_rows = (uint32_t)(vrows ? vrows->size() : rows->size());
    HIPCHK(h, psdk::launch_bank_var(vrows ? nullptr : reinterpret_cast<const psdk::BankJob *>(d + o_mid),
                                    vrows ? nullptr : reinterpret_cast<const psdk::BankRow *>(d + o_mid + mid),
                                    vrows ? reinterpret_cast<const psdk::VarRow *>(d + o_mid) : nullptr, n_rows,
                                    reinterpret_cast<const psdk::VarDesc *>(d), n_vars, reinterpret_cast<const float *>(d + o_taus), n_taus, d_out,
                                    h->stream));
    HIPCHK(h, st->mark_slot(s, h->stream));
    return PSDC_OK;
}

} // namespace

extern "C" {

int psdcv_bank_var_device(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                          int keep_transition_band, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus,
                          double *d_out, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                          psdcr_info *info)
{
    const Args a{"psdcv_bank_var_device", channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap,
                 info};
    uint32_t S = 0;
    int rc = check_selection(h, a, &S);
    if (rc)
        return rc;
    if ((rc = check_vars(h, a.who, vars, n_vars, taus, n_taus, d_out)))
        return rc;
    ON_DEVICE(h, h->device);
    Plan pl;
    if ((rc = plan_rows(h, a, S, &pl)))
        return rc;
    if (pl.jobs.empty()) { // nothing included anywhere: no kernel; every variance is 0.0
        if (S)
            HIPCHK(h, hipMemsetAsync(d_out, 0, sizeof(double) * S * n_vars * n_taus, h->stream));
    } else {
        if ((rc = enqueue(h, &pl.jobs, &pl.rows, nullptr, vars, n_vars, taus, n_taus, d_out)))
            return rc;
        if (info)
            info->launches = 1;
    }
    if (done_event)
        HIPCHK(h, hipEventRecord(static_cast<hipEvent_t>(done_event), h->stream));
    else
        HIPCHK(h, hipStreamSynchronize(h->stream));
    return PSDC_OK;
}

int psdcv_bank_var(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                   int keep_transition_band, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus, double *out,
                   size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info)
{
    const Args a{"psdcv_bank_var", channels, n_sel, keep_overlap, min_count, keep_transition_band, lens, n_breaks, breaks, breaks_cap, info};
    uint32_t S = 0;
    int rc = check_selection(h, a, &S);
    if (rc)
        return rc;
    if ((rc = check_vars(h, a.who, vars, n_vars, taus, n_taus, out)))
        return rc;
    ON_DEVICE(h, h->device);
    Plan pl;
    if ((rc = plan_rows(h, a, S, &pl)))
        return rc;
    const size_t count = (size_t)S * n_vars * n_taus;
    if (pl.jobs.empty()) {
        for (size_t i = 0; i < count; ++i)
            out[i] = 0.0;
        return PSDC_OK;
    }
    BankRead *st = state_of(h);
    HIPCHK(h, st->room_out(sizeof(double) * count));
    if ((rc = enqueue(h, &pl.jobs, &pl.rows, nullptr, vars, n_vars, taus, n_taus, reinterpret_cast<double *>(st->d_out))))
        return rc;
    if (info)
        info->launches = 1;
    HIPCHK(h, hipMemcpyAsync(st->h_out, st->d_out, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(out, st->h_out, sizeof(double) * count);
    return PSDC_OK;
}

int psdcv_rows_var_device(psdc_handle *h, const float *d_psd, const float *d_freq, size_t stride, const uint32_t *lens,
                          uint32_t n_rows, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus,
                          double *d_out, void *done_event, psdcr_info *info)
{
    const char *who = "psdcv_rows_var_device";
    if (!h)
        return bad(nullptr, who, "null handle");
    if (n_rows > PSDCR_MAX_ROWS)
        return bad(h, who, "more than PSDCR_MAX_ROWS rows");
    if (!d_psd || !d_freq)
        return bad(h, who, "null rows");
    if (!lens)
        return bad(h, who, "null lens");
    int rc = check_vars(h, who, vars, n_vars, taus, n_taus, d_out);
    if (rc)
        return rc;
    std::vector<psdk::VarRow> rows(n_rows);
    size_t max_len = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        if (lens[i] > stride)
            return bad(h, who, "a row longer than the stride");
        rows[i] = psdk::VarRow{d_psd + (size_t)i * stride, d_freq + (size_t)i * stride, lens[i], 0};
        max_len = std::max<size_t>(max_len, lens[i]);
    }
    if (info) {
        info->launches = 0;
        info->jobs = 0;
        info->max_len = max_len;
    }
    ON_DEVICE(h, h->device);
    if (n_rows) {
        if ((rc = enqueue(h, nullptr, nullptr, &rows, vars, n_vars, taus, n_taus, d_out)))
            return rc;
        if (info)
            info->launches = 1;
    }
    if (done_event)
        HIPCHK(h, hipEventRecord(static_cast<hipEvent_t>(done_event), h->stream));
    else
        HIPCHK(h, hipStreamSynchronize(h->stream));
    return PSDC_OK;
}

} // extern "C"
