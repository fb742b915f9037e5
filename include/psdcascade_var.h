/* psdcascade_var.h -- Var read-out on the device: the Allan, modified Allan and main-lobe variance (the reference's Var::eval,
 * src/var.rs:26-45) of every selected channel of a psdc_handle (PsdCascadeBank, PsdCascade) for up to 4096 taus and up to 4
 * descriptors, in ONE call: one drain, one kernel launch that reads the accumulators through the job table of the bank read-out
 * (include/psdcascade_readout.h) and writes the curves [S][n_vars][n_taus] f64 into caller memory on the device (or on the host
 * through one copy).  No stitched row is written.  A second form takes stitched rows that already lie on the device.  An
 * extension of psdcascade.h in a header of its own: the entry points carry the prefix psdcv_ and live in the same library;
 * psdcascade.h, its ABI version and its symbols are unchanged, and so is psdc_var_eval (one row, one tau, a sequential f32 fold on
 * the host).
 *
 * Definition.  For one row of L elements with f32 values p[e] (a phase PSD) and f32 frequencies f[e] (cycles per sample), one
 * descriptor (x_exp, sinx_exp, clip, dc_cut) and one f32 tau (in samples):
 *   Limit.      lim = clip / tau in f32.  E = the first e >= dc_cut with !(f[e] <= lim), compared in f32, or L if there is none:
 *               the reference's skip + take_while.  The first violation ends the row, also where keep_overlap makes f step back
 *               across a stage boundary later on.
 *   Sine.       For e in [dc_cut, E), everything in f64 on the f32 inputs: x = (double)f[e] * (double)tau, w = M_PI * x, and
 *               s = sin(pi x) by an exact fold: r = fmod(x, 2.0); r > 1: r -= 1 and the sign flips; r > 0.5: r = 1 - r;
 *               s = +-sin(M_PI * r).  Every step before the sin is exact and its argument lies in [0, pi/2].
 *   Term.       h = powi(s, sinx_exp) * powi(w, x_exp), powi by square and multiply with 1 / r for a negative exponent (the loop
 *               of psdc_var_eval);  a[e] = (((double)p[e] * (double)f[e]) * (double)f[e]) * h.
 *   Trapezoid.  t[e] = (a[e] + a[e-1]) * ((double)f[e] - (double)f[e-1]), with a[dc_cut-1] = f[dc_cut-1] = 0: the fold's initial
 *               state, NOT the element before.
 *   Sum.        var = the sum of t[e] over [dc_cut, E).  Every product is rounded on its own (the kernel TU is built with
 *               -ffp-contract=off: no fused multiply-add); the order is a function of L alone (thread t of 256 takes the elements
 *               t, t + 256, ..., then a fixed tree across the threads; no atomics); an element outside [dc_cut, E) adds +0.0.  Two
 *               calls on the same state give the same bits, the host and device forms give the same bits, and the rows form on
 *               the output of psdcr_bank_psd_device gives the bank form's bits.
 *   No special cases.  dc_cut = 0 on a row that starts at f = 0 gives 0 * inf = NaN, as the reference does.  A row without an
 *               included term (dc_cut >= E, L = 0) gives 0.0.
 * AVAR is (x_exp, sinx_exp) = (-2, 4), MVAR (-4, 6), both with clip = FLT_MAX; FVAR is AVAR's with clip = 1; dc_cut defaults to 2.
 * With a sample rate fs, Var on (f fs, tau / fs) and a density per Hz is fs^2 times the result here.
 *
 * Against the reference.  Var::eval computes the same formula in f32, with sin(fl32(pi fl32(f tau))).  Beyond pi f tau of a few
 * tens the rounding of that f32 argument is visible: the reference's own test vector (p = 1000, 100, 1.2, 3.4, 5.6 at f = 0, 1, 3,
 * 6, 9; tau = 2.7; the defaults) gives 0.13478442 there and 0.134782674 by the definition above, 1.75e-6 apart, from the rounding of
 * pi f tau = 76.3 at f = 9.  Bit parity with the f32 fold is not a goal (and could not be one: two sinf implementations differ).
 *
 * Selection, MergeOpts, layout outputs (lens, n_breaks, breaks, breaks_cap, info), the drain: as psdcr_bank_psd_device.
 * info->launches is 1, or 0 when no selected row has an included stage: the outputs are then set to 0.0 without a kernel.
 *
 * Calls.  `vars` (n_vars <= PSDCV_MAX_VARS descriptors; they share one sine a term), `taus` (n_taus <= PSDCV_MAX_TAUS) and `lens`
 * are HOST memory.
 *   psdcv_bank_var_device  d_out is [S][n_vars][n_taus] f64 on the device; nothing else is written.  done_event as in
 *                          psdcr_bank_psd_device (NULL: the call returns when the kernel has completed).
 *   psdcv_bank_var         the same into HOST memory through the handle's buffer: one copy, one synchronise; the device form's bits.
 *   psdcv_rows_var_device  n_rows caller rows on the device: row i is d_psd[i * stride ...) and d_freq[i * stride ...) with
 *                          lens[i] <= stride elements (what psdcr_bank_psd_device, psdcxr_bank_csd_device or an uploaded row left
 *                          there); d_out is [n_rows][n_vars][n_taus].  It does not drain; it enqueues on the handle's stream and
 *                          so orders behind a done_event read-out of the same handle without a host synchronisation.
 *                          info (may be NULL): launches, jobs = 0, max_len = the largest lens[i].
 *
 * Tables and buffers.  The job, row, descriptor and tau tables travel in the handle's two table slots of psdcascade_readout.h; its
 * two-slot rule holds across psdcr_ and psdcv_ calls.  The host form uses the handle's read-out buffer.  psdcr_release and
 * psdc_destroy free everything.
 *
 * PSDC_ERR_ARG, with a text through psdc_last_error: a NULL handle; n_vars of 0 or above 4; n_taus of 0 or above 4096; NULL vars,
 * taus or output; an exponent beyond +-PSDCV_MAX_EXP; a NaN clip; a tau that is NaN, infinite or <= 0; the selection errors of
 * psdcr_; for the rows form NULL rows or lens, lens[i] > stride, or n_rows > PSDCR_MAX_ROWS.  PSDC_ERR_CAPACITY for breaks_cap, as
 * in psdcr_ (lens, n_breaks and info are filled; nothing is launched). */
#ifndef PSDCASCADE_VAR_H
#define PSDCASCADE_VAR_H

#include "psdcascade_readout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psdcv_var {
    int32_t x_exp, sinx_exp;
    float clip;
    uint32_t dc_cut;
} psdcv_var;
#define PSDCV_MAX_VARS 4u /* descriptors a call: AVAR, MVAR, FVAR share one sine a term */
#define PSDCV_MAX_TAUS 4096u
#define PSDCV_MAX_EXP 16 /* |x_exp|, |sinx_exp| */

int psdcv_bank_var_device(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                          int keep_transition_band, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus,
                          double *d_out, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                          psdcr_info *info);
int psdcv_bank_var(psdc_handle *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count,
                   int keep_transition_band, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus, double *out,
                   size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcr_info *info);
int psdcv_rows_var_device(psdc_handle *h, const float *d_psd, const float *d_freq, size_t stride, const uint32_t *lens,
                          uint32_t n_rows, const psdcv_var *vars, uint32_t n_vars, const float *taus, uint32_t n_taus,
                          double *d_out, void *done_event, psdcr_info *info);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_VAR_H */
