// waterfall_robust.h -- what wf_robust_kernel (waterfall_robust.hip) computes for one (side, bin): the median, the minimum, the
// maximum and the SK-excised mean over the newest R complete blocks of one ring (include/psdcascade_robust.h states the
// semantics).  Host and device: tests/host/waterfall_robust_emul.cpp runs these on the CPU against a sort.
//
// The rows are walked oldest first; row r is block last - (R - 1) + r in slot block mod K (waterfall_read.h).  One pass finds NaN,
// minimum, maximum and the excision sum.  The order statistics come from a bisection on the bit pattern: S1 is a sum of squares, so
// a value that is not NaN is >= +0 and its bits as u64 order like the number (+inf included).  Between bits(min) and bits(max) the
// smallest pattern x with #{V_r <= x} > k is the k-th order statistic: at most 64 passes of R loads, no array a thread indexes
// (that would live in scratch), no LDS, and ties need no care.  An even R takes its upper middle value from one pass more.
#pragma once
#include "waterfall_read.h"

#include <cstddef>

// The rows of a pass are independent loads: unrolled, a thread has eight of them in flight where the rolled loop waits for each
// (the order of the excision sum's adds stays the rows' order).
#if defined(__clang__)
#define PSDK_WF_UNROLL _Pragma("unroll 8")
#else
#define PSDK_WF_UNROLL
#endif

namespace psdk {

constexpr uint32_t WF_ROBUST_MAX_ROWS = 4096;

// The considered rows of a ring with `started` blocks started, the newest of them with `newest` of B segments: R = min(max_rows,
// complete blocks the ring of K slots holds, 4096), and *last the newest complete block (R > 0).  The newest block counts once it
// holds B segments.
PSDK_WF_HD inline uint32_t wf_robust_rows(uint64_t started, uint32_t newest, uint32_t B, uint32_t K, uint32_t max_rows, uint64_t *last)
{
    const uint32_t partial = started && newest < B ? 1 : 0;
    const uint32_t held = wf_valid_rows(started, K) - partial;
    const uint32_t cap = max_rows < WF_ROBUST_MAX_ROWS ? max_rows : WF_ROBUST_MAX_ROWS;
    *last = started - partial - (started ? 1 : 0);
    return held < cap ? held : cap;
}

struct WfRobustBin {
    float median, min, max, excised;
    uint32_t kept;
};

PSDK_WF_HD inline uint64_t wf_bits(double v)
{
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}
PSDK_WF_HD inline double wf_from_bits(uint64_t u)
{
    double v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// The considered rows of one (side, bin): `ring` the stage's ring of K slots of `set` f64, o1 / o2 the offsets of this bin's S1
// and S2 inside a slot, `last` the newest considered block, R = 1 ... min(K, last + 1) rows.
struct WfRobustRows {
    const double *ring;
    uint64_t last;
    uint32_t K, R;
    size_t set, o1, o2;
    PSDK_WF_HD uint32_t first_slot() const { return (uint32_t)((last - (R - 1)) % K); }
    PSDK_WF_HD static uint32_t next_slot(uint32_t slot, uint32_t K) { return slot + 1 == K ? 0 : slot + 1; }
};

// rows with V_r <= the pivot (bit patterns; no row is NaN), and the smallest V_r above it (all ones: none)
PSDK_WF_HD inline uint32_t wf_count_le(const WfRobustRows &w, uint64_t pivot, uint64_t *above)
{
    uint32_t c = 0, slot = w.first_slot();
    uint64_t up = ~(uint64_t)0;
    PSDK_WF_UNROLL
    for (uint32_t r = 0; r < w.R; ++r, slot = WfRobustRows::next_slot(slot, w.K)) {
        const uint64_t u = wf_bits(w.ring[(size_t)slot * w.set + w.o1]);
        c += u <= pivot ? 1u : 0u;
        up = u > pivot && u < up ? u : up;
    }
    if (above)
        *above = up;
    return c;
}

// the k-th smallest V_r (k = 0 ... R - 1) as a bit pattern, given bits(min) and bits(max); no row is NaN
PSDK_WF_HD inline uint64_t wf_select(const WfRobustRows &w, uint32_t k, uint64_t lo, uint64_t hi)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (wf_count_le(w, mid, nullptr) > k)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// g = (double)gsc_block; B the segments of a complete block; a row is kept iff sk_lo <= wf_sk_f64(B, V_r, W_r) <= sk_hi (a NaN
// is not).  want_median / want_sk: skip the bisection / the S2 loads when no such output is asked for (the fields are then unset).
PSDK_WF_HD inline WfRobustBin wf_robust_bin(const WfRobustRows &w, uint32_t B, double g, double sk_lo, double sk_hi, bool want_median,
                                            bool want_sk)
{
    WfRobustBin out{};
    bool nan = false;
    double mn = 0.0, mx = 0.0, sum = 0.0;
    uint32_t kept = 0, slot = w.first_slot();
    PSDK_WF_UNROLL
    for (uint32_t r = 0; r < w.R; ++r, slot = WfRobustRows::next_slot(slot, w.K)) {
        const double v = w.ring[(size_t)slot * w.set + w.o1];
        nan = nan || v != v;
        mn = r == 0 || v < mn ? v : mn;
        mx = r == 0 || v > mx ? v : mx;
        if (want_sk) {
            const double sk = wf_sk_f64(B, v, w.ring[(size_t)slot * w.set + w.o2]);
            if (sk >= sk_lo && sk <= sk_hi) { // (false for a NaN)
                ++kept;
                sum += v;
            }
        }
    }
    const float fnan = __builtin_nanf("");
    out.min = nan ? fnan : (float)(mn * g);
    out.max = nan ? fnan : (float)(mx * g);
    out.kept = kept;
    out.excised = kept ? (float)((sum / (double)kept) * g) : fnan;
    out.median = fnan;
    if (want_median && !nan) {
        const uint32_t k = (w.R - 1) / 2; // the middle row, the lower of the two of an even R
        const uint64_t lo = wf_select(w, k, wf_bits(mn), wf_bits(mx));
        double m = wf_from_bits(lo);
        if (!(w.R & 1)) {
            uint64_t above;
            const uint32_t le = wf_count_le(w, lo, &above);
            m = 0.5 * (m + (le > k + 1 ? m : wf_from_bits(above))); // (le > k + 1: the upper middle row ties with the lower)
        }
        out.median = (float)(m * g);
    }
    return out;
}

} // namespace psdk
