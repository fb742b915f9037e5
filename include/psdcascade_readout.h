/* psdcascade_readout.h -- bank read-out on the device: the stitched PSD of every selected channel of a psdc_handle (PsdCascadeBank,
 * PsdCascade), its frequencies and the integrated power of up to 8 frequency bands a channel, in ONE call: one drain, one kernel
 * launch that stitches every selected channel at once into caller memory on the device (or on the host through one copy), at most
 * one launch more for the bands.  An extension of psdcascade.h in a header of its own: the entry points carry the prefix psdcr_
 * and live in the same library; psdcascade.h, its ABI version and its symbols are unchanged.
 *
 * psdc_psd reads ONE channel through the host: it drains and synchronises the stream, launches a copy-out of that channel's
 * accumulators, synchronises again and stitches on the host.  A caller that repaints every trace (src/bin/psd.rs:172-216) pays
 * that per channel; a consumer that stays on the GPU has no path.  The calls here return the same Break records as psdc_psd, and
 * every PSD value and every frequency equals what psdc_psd / psdc_frequencies return, byte for byte.
 *
 * Selection.  `channels` == NULL selects every channel of the handle in order (n_sel is ignored; S = n_channels rows); otherwise
 * it names S = n_sel channel indices in any order, duplicates allowed (each gets a row of its own).  keep_overlap, min_count and
 * keep_transition_band are MergeOpts of psdc_psd.
 *
 * Layout outputs (host memory), per selected row i: lens[i] = the stitched length of the row (psdc_psd's *psd_len), n_breaks[i] =
 * its number of Breaks, breaks[i * breaks_cap ... i * breaks_cap + n_breaks[i]) = the Breaks, deepest stage first, as psdc_psd
 * writes them.  lens is required; n_breaks and breaks may be NULL (breaks needs n_breaks).  `info` may be NULL; otherwise
 * info->max_len = the largest lens[i], info->jobs = the included stages of all rows, info->launches = the kernels the call
 * enqueued beyond the drain.
 *
 * Drain and counters.  Every call drains the handle exactly as psdc_psd does (host staging is submitted, every pipeline round and
 * the pending epilogue are enqueued on the handle's stream); the kernels of this call are enqueued behind that on the same
 * stream.  Counts, averaging limits and pendings are the host's bookkeeping after that drain: no synchronisation is needed to
 * know them, so psdcr_bank_layout and the done_event form never wait for the device.  A read-out changes nothing in the handle.
 *
 * Jobs.  Per selected row the host runs the stitch of psdc_psd without an output row and gets the Breaks.  Every included Break
 * becomes one job: the stage's accumulator row on the device, bins [bins_start, bins_end), output offset `start`, and two f32
 * factors computed on the host, gsc = 1.0f / (gain(stage) * (float)decimation) exactly as psdc_psd computes it and
 * rbw = 1.0f / (float)(fft_size * decimation) of psdc_frequencies.  The kernel computes psd = spectrum[k] * gsc and
 * freq = (float)k * rbw: one f32 multiply an element each, which is why the bytes are psdc_psd's.
 *
 * Band power.  The reference's Trapezoidal (src/bin/psd.rs:98-116; psdc_trace_plot restates it in f32) carried in f64 over one
 * stitched row p[0 .. L) with its frequencies f[0 .. L):
 *     t_k    = 0.5 * ((double)p[k] + (double)p[k-1]) * ((double)f[k] - (double)f[k-1]),   p[-1] = f[-1] = 0
 *     band_b = the sum of t_k over the k with lo_b <= f[k] <= hi_b, compared in f32
 * Frequencies are in cycles per sample (0 ... 0.5): a caller with a sample rate divides its limits by it.  `bands` is HOST memory,
 * [n_bands][2] = (lo, hi), n_bands <= PSDCR_MAX_BANDS; the output is [S][n_bands] f64.  Every product t_k is rounded on its own before
 * it is added (the kernel TU is built with -ffp-contract=off: no fused multiply-add).  The summation order is a function of L
 * alone (a fixed stride a thread, a fixed tree across threads, no atomics): two calls on the same state give the same bits, and
 * the host and device forms give the same bits.  The band kernel reads the accumulators, not the stitched rows: bands may be asked
 * for alone.  Bands cost one launch more.
 *
 * Launches.  info->launches is 1 without bands, 2 with bands (1 for bands alone), and 0 when no selected row has an included stage
 * (band powers are then set to 0.0 without a kernel).  One launch covers any selection: jobs are indexed along the grid's x dimension.
 * S is limited to PSDCR_MAX_ROWS = 65536 rows a call.
 *
 * Job table.  The jobs travel in a table the call writes into pinned host memory and copies to the device asynchronously.  The
 * handle keeps TWO table slots with an event each: a slot is rewritten only after the kernels that read its last table have
 * completed, so two done_event calls back to back never wait for each other, and a third waits for the first.
 *
 * Buffers and who frees them.  The table slots, and for psdcr_bank_psd a device buffer of S * max_len values an output with its
 * pinned image, are made on first use, grow to the largest call and belong to the HANDLE: psdc_destroy frees them with it (no
 * psdcr_ call is needed, nothing leaks), and psdcr_release(h) frees them earlier (it waits for the calls in flight; the next
 * read-out makes them again).  psdc_clone does not copy them.
 *
 * Calls.
 *   psdcr_bank_layout      drains and fills lens, n_breaks, breaks and info.  It launches nothing: the psd_out == NULL form of
 *                          psdc_psd for a selection.
 *   psdcr_bank_psd_device  row i of d_psd and d_freq (either may be NULL: not wanted) starts at i * stride floats and receives
 *                          lens[i] values; elements [lens[i], stride) are not written, nor is anything behind the last row.
 *                          d_band_power is [S][n_bands] f64 (NULL with n_bands == 0).  With done_event == NULL the call returns
 *                          when the kernels have completed; otherwise it records that hipEvent_t behind them on the handle's
 *                          stream and returns without synchronising the host (the event is recorded even when nothing was
 *                          launched).
 *   psdcr_bank_psd         the same with HOST outputs: the same kernels into the handle's device buffer, one device-to-host
 *                          copy through pinned memory, one synchronise.  Its bytes are the device form's.
 *   psdcr_release          see above.
 *
 * Edge cases.  A channel without stages gives lens[i] = 0, n_breaks[i] = 0 and band powers 0.0; its rows are untouched.
 * PSDC_ERR_CAPACITY: stride < max_len (the two read-out calls, when d_psd / d_freq is given), or breaks is given and breaks_cap is
 * smaller than some n_breaks[i].  lens, n_breaks and info->max_len are filled (and the Breaks of the rows that fit) so that the caller can
 * retry; nothing is launched and no output is written.
 * PSDC_ERR_ARG, with a text through psdc_last_error: a NULL handle; a channel out of range (or more than PSDCR_MAX_ROWS
 * selected rows); n_bands > 8; bands without a band output, a band output without bands, or n_bands > 0 with a NULL band list;
 * a band with NaN or lo > hi; NULL lens; breaks without n_breaks; all of psd, freq and the band output NULL in the two read-out
 * calls.
 *
 * Out of scope: the cross-runtime objects (psdc_cross_* ... the waterfalls: f64 accumulators behind other handle types) and
 * Trace::plot's decibel conversion.  Var (the Allan-type variance curves of the same selection) is psdcascade_var.h's. */
#ifndef PSDCASCADE_READOUT_H
#define PSDCASCADE_READOUT_H

#include "psdcascade.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psdcr_info {
    uint32_t launches; /* kernels enqueued beyond the drain */
    uint32_t jobs;     /* included stages over all selected rows */
    uint64_t max_len;  /* the largest lens[i] */
} psdcr_info;
#define PSDCR_MAX_BANDS 8u
#define PSDCR_MAX_ROWS 65536u

int psdcr_bank_layout(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                      int keep_transition_band, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info);
int psdcr_bank_psd_device(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                          int keep_transition_band, float *d_psd, float *d_freq, size_t stride, const float *bands, uint32_t n_bands,
                          double *d_band_power, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                          psdcr_info *info);
int psdcr_bank_psd(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                   int keep_transition_band, float *psd, float *freq, size_t stride, const float *bands, uint32_t n_bands,
                   double *band_power, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info);
int psdcr_release(psdc_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_READOUT_H */
