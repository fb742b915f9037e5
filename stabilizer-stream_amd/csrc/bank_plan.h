// bank_plan.h -- what the read-outs of a psdc_handle share on the host (bank_readout.cpp defines it; psdcr_* there and psdcv_* of
// bank_var.cpp use it): the selection checks, the drain and the plan of every selected row, the handle's BankRead.
#pragma once
#include "../../include/psdcascade_readout.h"
#include "bank_readout.h"
#include "host_runtime.h"

#include <vector>

namespace psdrt {
namespace bankread {

struct Plan {
    std::vector<psdk::BankJob> jobs;
    std::vector<psdk::BankRow> rows;
    size_t max_len = 0;
    uint32_t max_bins = 0;
};

struct Args {
    const char *who;
    const uint32_t *channels;
    uint32_t n_sel;
    int keep_overlap;
    uint32_t min_count;
    int keep_transition_band;
    size_t *lens, *n_breaks;
    psdc_break *breaks;
    size_t breaks_cap;
    psdcr_info *info;
};

// what the handle keeps for these calls (psdc_handle::bank_read): psdrt::BankRead of host_runtime.h, made by the first call
BankRead *state_of(psdc_handle *h);
// PSDC_ERR_ARG with the text "<who>: <what>"
int bad(psdc_handle *h, const Args &a, const char *what);
// the checks every call shares; *rows = the number of selected rows
int check_selection(psdc_handle *h, const Args &a, uint32_t *rows);
// Drain, then the layout of every selected row and its jobs from the host's bookkeeping.  Fills lens, n_breaks, info->max_len and
// info->jobs always (info->launches = 0), the Breaks where they fit; PSDC_ERR_CAPACITY when some row's Breaks do not.
int plan_rows(psdc_handle *h, const Args &a, uint32_t S, Plan *pl);

} // namespace bankread
} // namespace psdrt
