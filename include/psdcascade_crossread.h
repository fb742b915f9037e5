/* psdcascade_crossread.h -- bank read-out on the device for the pair object (psdc_cross: CsdCascadeBank, CsdCascade) and the matrix
 * object (psdc_csm: CsmCascadeBank, CsmCascade): the stitched rows of every selected pair or group, their frequencies and, for
 * pairs, coherence, the H1 transfer function and the sums of up to 8 frequency bands, in ONE call: one drain, one kernel launch
 * that stitches every selected unit at once into caller memory on the device (or on the host through one copy), at most one launch
 * more for the bands.  An extension of psdcascade.h in a header of its own, the sibling of psdcascade_readout.h (psdcr_*, the same
 * for a psdc_handle): the entry points carry the prefix psdcxr_ and live in the same library; psdcascade.h, psdcascade_readout.h,
 * psdcascade_robust.h, the ABI version and their symbols are unchanged.
 *
 * psdc_cross_csd / psdc_csm_csd read ONE unit through the host: they drain and synchronise both streams of the object, copy every
 * stage's f64 accumulators out with a blocking copy each, cast them to f32 and stitch on the host; coherence and H1 are then the
 * caller's arithmetic.  A caller that repaints every pair pays that per pair; a consumer that stays on the GPU has no path.  The
 * calls here return the same Break records, and every f32 value and every frequency equals what psdc_cross_csd / psdc_csm_csd and
 * psdc_frequencies return, byte for byte.
 *
 * Selection.  `pairs` / `groups` == NULL selects every unit of the object in order (n_sel is ignored; S = the object's units);
 * otherwise it names S = n_sel unit indices in any order, duplicates allowed (each gets a row of its own).  keep_overlap,
 * min_count and keep_transition_band are the MergeOpts of psdc_cross_csd.  S is limited to PSDCXR_MAX_ROWS = 65536 a call.
 *
 * Layout outputs (host memory), per selected unit i: lens[i] = the stitched length of its rows (psdc_cross_csd's *len),
 * n_breaks[i] = its number of Breaks, breaks[i * breaks_cap ... i * breaks_cap + n_breaks[i]) = the Breaks, deepest stage first, as
 * psdc_cross_csd / psdc_csm_csd write them.  lens is required; n_breaks and breaks may be NULL (breaks needs n_breaks).  `info`
 * may be NULL; otherwise info->max_len = the largest lens[i], info->jobs = the included stages of all selected units,
 * info->launches = the kernels the call enqueued beyond the drain.
 *
 * Drain and counters.  Every call drains the object exactly as psdc_cross_csd does (every pipeline round is enqueued on the
 * object's stream) and nothing more: it does not synchronise the streams.  The kernels of this call are enqueued behind that on
 * the same stream.  Counts, averaging limits and pendings are the host's bookkeeping after that drain: no synchronisation is
 * needed to know them, so the layout calls and the done_event form never wait for the device.  A read-out changes nothing in the
 * object.
 *
 * Jobs.  Per selected unit the host runs the stitch of psdc_cross_csd without an output row and gets the Breaks.  Every included
 * Break becomes one job: the stage's f64 accumulator on the device, laid out [rows][n/2 + 1] (a pair: xx, yy, re xy, im xy; a
 * group: the m * m rows of psdc_csm_csd), bins [bins_start, bins_end), output offset `start`, and two f32 factors computed on the
 * host, gsc = 1.0f / (gain(stage) * (float)decimation) exactly as the stitch computes it and
 * rbw = 1.0f / (float)(fft_size * decimation) of psdc_frequencies.  The kernel computes value = (float)acc[r][k] * gsc -- the f32
 * cast psdc_cross_csd makes on the host, then the stitch's one f32 multiply -- and freq = (float)k * rbw: which is why the bytes are
 * psdc_cross_csd's.
 *
 * Coherence and H1 (pairs) are formed in f64 from the f64 accumulators of the same bin, in the same launch; the scale cancels, so
 * no f32 rounding enters:
 *     den       = xx * yy
 *     coherence = den != 0 ? (re * re + im * im) / den : NaN
 *     transfer  = xx != 0 ? (re / xx, im / xx) : (NaN, NaN)          (H1 = Sxy / Sxx, Sxy = sum conj(X) Y)
 *
 * Band sums (pairs).  The trapezoid of psdcascade_readout.h, with its f32 band comparison, its thread stride and its reduction
 * tree, applied to each of the four stitched f32 rows p = sxx, syy, re sxy, im sxy of a pair (p may be negative for re / im) with
 * their frequencies f:
 *     t_k    = 0.5 * ((double)p[k] + (double)p[k-1]) * ((double)f[k] - (double)f[k-1]),   p[-1] = f[-1] = 0
 *     band_b = the sum of t_k over the k with lo_b <= f[k] <= hi_b, compared in f32
 * `bands` is HOST memory, [n_bands][2] = (lo, hi) in cycles per sample, n_bands <= PSDCXR_MAX_BANDS; the output is
 * [S][n_bands][4] f64 = (xx, yy, re xy, im xy).  Every product is rounded on its own before it is added (the kernel TU is built
 * with -ffp-contract=off); the summation order is a function of the row length alone (no atomics): two calls on the same state
 * give the same bits, and the host and device forms give the same bits.  One workgroup serves a pair.  The band kernel reads the
 * accumulators, not the stitched rows: bands may be asked for alone.  Bands cost one launch more.  The band coherence
 * (re^2 + im^2) / (xx yy) and the band H1 (re / xx, im / xx) of the four sums are the caller's arithmetic.
 *
 * Launches.  info->launches is 1 without bands, 2 with bands (1 for bands alone), and 0 when no selected unit has an included
 * stage (band sums are then set to 0.0 without a kernel).  One launch covers any selection: jobs are indexed along the grid's x
 * dimension.
 *
 * Job table.  The jobs travel in a table the call writes into pinned host memory and copies to the device asynchronously.  The
 * object keeps TWO table slots with an event each: a slot is rewritten only after the kernels that read its last table have
 * completed, so two done_event calls back to back never wait for each other, and a third waits for the first.
 *
 * Buffers and who frees them.  The table slots, and for the host forms a device buffer of the outputs with its pinned image, are
 * made on first use, grow to the largest call and belong to the OBJECT: psdc_cross_destroy / psdc_csm_destroy free them with it (no
 * psdcxr_ call is needed, nothing leaks), and psdcxr_cross_release / psdcxr_csm_release free them earlier (they wait for the calls in
 * flight; the next read-out makes them again).
 *
 * Calls.
 *   psdcxr_cross_layout      drains and fills lens, n_breaks, breaks and info.  It launches nothing: the form of psdc_cross_csd
 *                            without output rows, for a selection.
 *   psdcxr_cross_csd_device  every output pointer is device memory and optional, but at least one of the seven must be given.
 *                            `stride` is in bins.  Row i of d_sxx, d_syy and d_freq (f32) and of d_coherence (f64) starts at
 *                            i * stride elements, row i of d_sxy (f32) and d_transfer (f64), which hold (re, im) interleaved, at
 *                            2 * i * stride; a row receives lens[i] bins; elements [lens[i], stride) of a row are not written, nor
 *                            is anything behind the last row.  d_band_sums is [S][n_bands][4] f64 (NULL with n_bands == 0).  With
 *                            done_event == NULL the call returns when the kernels have completed; otherwise it records that
 *                            hipEvent_t behind them on the object's stream and returns without synchronising the host (the event
 *                            is recorded even when nothing was launched).
 *   psdcxr_cross_csd         the same with HOST outputs: the same kernels into the object's device buffer, one device-to-host
 *                            copy through pinned memory, one synchronise.  Its bytes are the device form's.
 *   psdcxr_cross_release     see above.
 *   psdcxr_csm_layout, psdcxr_csm_rows_device, psdcxr_csm_rows, psdcxr_csm_release
 *                            the same for a matrix object.  `rows` is f32 [S][m * m][stride] in the row order of psdc_csm_csd
 *                            (row a * m + a is S_aa; for a < b row a * m + b is Re S_ab and row b * m + a is Im S_ab), freq is f32
 *                            [S][stride]; either may be NULL, not both.  There are no derived quantities and no bands.
 *
 * Edge cases.  A unit without stages gives lens[i] = 0, n_breaks[i] = 0 and band sums 0.0; its rows are untouched.
 * PSDC_ERR_CAPACITY: stride < max_len (the read-out calls, when an output other than the band sums is given), or breaks is given
 * and breaks_cap is smaller than some n_breaks[i].  lens, n_breaks and info->max_len are filled (and the Breaks of the units that
 * fit) so that the caller can retry; nothing is launched and no output is written.
 * PSDC_ERR_ARG, with a text through psdc_cross_last_error / psdc_csm_last_error: a NULL handle; a unit out of range (or more than
 * PSDCXR_MAX_ROWS selected); n_bands > 8; bands without a band output, a band output without bands, or n_bands > 0 with a NULL band
 * list; a band with NaN or lo > hi; NULL lens; breaks without n_breaks; every output NULL in the read-out calls.
 *
 * Out of scope: the zoom, IQ, spectral kurtosis, AM/PM and waterfall objects (the job carries the row count: they can follow with
 * a wrapper each), phase, magnitude and decibel outputs, and the multi-input quantities of a matrix. */
#ifndef PSDCASCADE_CROSSREAD_H
#define PSDCASCADE_CROSSREAD_H

#include "psdcascade.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psdcxr_info {
    uint32_t launches; /* kernels enqueued beyond the drain */
    uint32_t jobs;     /* included stages over all selected units */
    uint64_t max_len;  /* the largest lens[i] */
} psdcxr_info;
#define PSDCXR_MAX_BANDS 8u
#define PSDCXR_MAX_ROWS 65536u

int psdcxr_cross_layout(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                        int keep_transition_band, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info);
int psdcxr_cross_csd_device(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                            int keep_transition_band, float *d_sxx, float *d_syy, float *d_sxy, float *d_freq, double *d_coherence,
                            double *d_transfer, size_t stride, const float *bands, uint32_t n_bands, double *d_band_sums, void *done_event,
                            size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info);
int psdcxr_cross_csd(psdc_cross *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                     float *sxx, float *syy, float *sxy, float *freq, double *coherence, double *transfer, size_t stride, const float *bands,
                     uint32_t n_bands, double *band_sums, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                     psdcxr_info *info);
int psdcxr_cross_release(psdc_cross *h);

int psdcxr_csm_layout(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                      size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info);
int psdcxr_csm_rows_device(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                           int keep_transition_band, float *d_rows, float *d_freq, size_t stride, void *done_event, size_t *lens,
                           size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcxr_info *info);
int psdcxr_csm_rows(psdc_csm *h, const uint32_t *groups, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                    float *rows, float *freq, size_t stride, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                    psdcxr_info *info);
int psdcxr_csm_release(psdc_csm *h);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_CROSSREAD_H */
