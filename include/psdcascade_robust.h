/* psdcascade_robust.h -- robust read-outs of the waterfall cascades (psdc_wf_*, psdc_zwf_* of psdcascade.h): per bin the median,
 * the minimum, the maximum and the spectral-kurtosis-excised mean over a stage's recent blocks, computed on the device from the
 * ring in one kernel launch.  An extension of psdcascade.h in a header of its own: the entry points carry the prefix psdcx_ and
 * live in the same library; psdcascade.h, its ABI version and its symbols are unchanged.
 *
 * A waterfall stage keeps a ring of its newest K blocks of B segments, each block with its own S1 = sum P and S2 = sum P^2 per
 * bin (psdcascade.h, "waterfall cascades").  psdc_wf_image shows them, a sum over them is a mean: one glitch, overload or
 * intermittent interferer in one block raises it.  The read-outs here take statistics ACROSS the blocks instead.
 *
 * Considered rows.  The statistics are taken over the newest R COMPLETE blocks of one stage (blocks that hold B segments),
 * oldest first, with R = min(max_rows, complete blocks the ring holds, PSDCX_ROBUST_MAX_ROWS).  The newest block is left out
 * while it holds fewer than B segments.  Block b lives in ring slot b mod K.  Below V_r is S1 of row r at one side and bin, W_r its
 * S2, and g = (double)gsc with gsc the f32 factor psdc_wf_image applies to a row of B segments of this stage
 * (psd[r][k] = float32(S1[r][k] * (double)gsc)).  Everything is computed in f64 and rounded to f32 once:
 *
 *   median   NaN if any V_r is NaN.  Otherwise, with the V_r sorted ascending as v_0 ... v_(R-1): m = v_((R-1)/2) for odd R and
 *            m = 0.5 * (v_(R/2-1) + v_(R/2)) for even R; the output is (float)(m * g).
 *   min/max  NaN if any V_r is NaN, otherwise (float)(min_r V_r * g) and (float)(max_r V_r * g): min / max hold over the R blocks.
 *   excised  sk_r = (B + 1) / (B - 1) * (B * W_r / (V_r * V_r) - 1) in f64 (NaN where V_r == 0): the estimator psdc_wf_image
 *   kept     rounds to f32 for its sk image, here before that rounding.  Row r is kept iff sk_r is not NaN and
 *            sk_lo <= sk_r <= sk_hi, compared in f64.  kept = the number of kept rows; sum = the kept V_r added in f64, oldest
 *            first; excised = kept ? (float)((sum / (double)kept) * g) : NaN.  A row with a NaN moment or without power is
 *            never kept (nor one whose V_r and W_r have both overflowed to +inf: its sk_r is NaN).  For stationary Gaussian noise sk_r scatters around 1 (2 at the real-valued bins 0 and n/2)
 *            with a standard deviation of about 2 / sqrt(B).
 *
 * The median of B-segment averages of Gaussian noise lies below their mean by about the factor (1 - 1 / (9 B))^3 (the median of
 * a gamma variate of shape B; less exact for overlapped segments): the outputs are not corrected for it.
 *
 * Method: one thread a (side, bin).  One pass over the rows finds NaN, minimum, maximum and the excision sum; the order statistics
 * come from a bisection on the bit pattern of the non-negative f64 values between bits(min) and bits(max), counting the rows at or
 * below the pivot: at most 64 passes more, exact, ties need no care.
 *
 * Out of scope: partial blocks (the newest block while it fills) are never part of the statistics; every row has weight 1 (no
 * weights, no set_avg); only the two waterfall kinds have rings, no other object of psdcascade.h is taken; more than
 * PSDCX_ROBUST_MAX_ROWS = 4096 rows are not considered (a deeper ring is read over its newest 4096 complete blocks).
 *
 * Calls.  Outputs of a psdc_wf are [n/2 + 1], of a psdc_zwf [2][n/2 + 1] with side 0 the upper and side 1 the lower sideband.
 * Any output may be NULL (not wanted); `info` is required and always written on success.  The calls drain the object as every
 * read-out does and cost exactly one kernel launch (counted by stats_read), whatever is asked for.  The _device forms take the
 * five outputs in device memory and return when the kernel has completed.  With R == 0 (no complete block yet, or max_rows == 0)
 * they return PSDC_OK with info->rows == 0, write no output and launch nothing.
 * PSDC_ERR_ARG, with a text through psdc_wf_last_error / psdc_zwf_last_error: a NULL handle; a NULL info; all five outputs NULL;
 * excised or kept given while sk_lo or sk_hi is NaN or sk_lo > sk_hi (-inf and +inf are allowed: they keep every row with a
 * finite SK); a channel or a stage out of range. */
#ifndef PSDCASCADE_ROBUST_H
#define PSDCASCADE_ROBUST_H

#include "psdcascade.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psdcx_robust_info {
    uint32_t rows;        /* R: complete blocks the statistics were taken over */
    uint32_t block;       /* B */
    uint64_t first_block; /* absolute index of the oldest considered block (rows > 0) */
    uint64_t last_block;  /* ... of the newest */
} psdcx_robust_info;
#define PSDCX_ROBUST_MAX_ROWS 4096u

int psdcx_wf_robust(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *median, float *min,
                    float *max, float *excised, uint32_t *kept, psdcx_robust_info *info);
int psdcx_wf_robust_device(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *d_median,
                           float *d_min, float *d_max, float *d_excised, uint32_t *d_kept, psdcx_robust_info *info);
int psdcx_zwf_robust(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *median, float *min,
                     float *max, float *excised, uint32_t *kept, psdcx_robust_info *info);
int psdcx_zwf_robust_device(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, double sk_lo, double sk_hi, float *d_median,
                            float *d_min, float *d_max, float *d_excised, uint32_t *d_kept, psdcx_robust_info *info);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_ROBUST_H */
