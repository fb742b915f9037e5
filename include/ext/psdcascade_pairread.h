/* psdcascade_pairread.h -- bank read-out on the device for the four pair carrier objects: the stitched auto and cross spectra of
 * both sides of every selected pair, their frequencies, coherence, H1 and band sums, and for the AM/PM cross kinds the carriers,
 * the complementary cross spectra cab / cba, the AM/PM cross split that depends on the carriers and its band integrals (column 2:
 * the integrated cross-correlated phase noise), in ONE call: one drain, one kernel launch for all pairs, at most one more for the
 * bands.  An extension of psdcascade.h in a header of its own, the sibling of psdcascade_crossread.h (psdcxr_*) and
 * psdcascade_carrierread.h: the entry points carry the prefix psdcpr_ and live in the same library; psdcascade.h, the
 * other extension headers, the ABI version and their symbols are unchanged.
 *
 * Objects (`h` is one of these handles, passed as void *; the call looks at the object's kind and refuses every other object of
 * the cross-spectral runtime with PSDC_ERR_ARG "<name>: takes a zoom cross, IQ cross or zoom / IQ AM/PM cross object"; the ampm
 * calls refuse the 8-row kinds with "<name>: takes a zoom AM/PM cross or IQ AM/PM cross object"; a handle of another runtime must
 * not be passed):
 *     psdc_zcsd, psdc_iqcsd        eight f64 accumulator rows a stage
 *     psdc_zxampm, psdc_iqxampm    twelve
 * Rows (include/psdcascade.h): 0, 1 S_aa upper, lower; 2, 3 S_bb upper, lower; 4, 5 Re S_ab upper, lower; 6, 7 Im S_ab upper,
 * lower; 8, 9 Re cab, Im cab; 10, 11 Re cba, Im cba (12-row kinds only).
 *
 * The rules are those of psdcascade_crossread.h, word for word, with "pair" for "unit": the selection (`pairs` == NULL selects
 * every pair in order, else n_sel indices in any order, duplicates allowed, at most PSDCXR_MAX_ROWS), the MergeOpts triple
 * keep_overlap / min_count / keep_transition_band, the layout outputs lens, n_breaks, breaks, breaks_cap and info,
 * PSDC_ERR_CAPACITY (lens, n_breaks and info->max_len are filled for a retry, nothing is launched, no output is written), `stride`
 * in bins with elements [lens[i], stride) of a row never written, the done_event form, "drain and nothing more, no host
 * synchronisation", the job table in two slots, and the buffers that belong to the object and go with its destroy (psdcpr_release
 * frees them earlier).  lens, n_breaks and the Breaks equal what psdc_zcsd_csd, psdc_zxampm_sidebands and their IQ siblings
 * return.  Only what differs is listed below.
 *
 * Errors.  A NULL handle gives PSDC_ERR_ARG and "<name>: null handle" through psdc_zcsd_last_error(NULL) (or any sibling's: the
 * cross-spectral runtime keeps one text a thread).  The texts of the argument rules are those of psdcascade_crossread.h.
 *
 * CSD (psdcpr_csd, all four kinds).  Every output is optional; at least one output or band sums must be given.
 *     saa_up, saa_lo, sbb_up, sbb_lo, freq   f32 [S][stride]
 *     sab_up, sab_lo                         f32 (re, im) interleaved, row i at 2 * i * stride
 *     coh_up, coh_lo                         f64 [S][stride]
 *     h1_up, h1_lo                           f64 (re, im) interleaved
 * Stitched values are (float)acc[r][k] * gsc and freq = (float)k * rbw with the two f32 factors of psdcascade_crossread.h: for the
 * 8-row kinds the bytes of psdc_zcsd_csd / psdc_iqcsd_csd and of psdc_frequencies.  Coherence and H1 come from the f64
 * accumulators of the same stage and bin, a side each (the scale cancels, no f32 rounding enters):
 *     coh_up = (acc4^2 + acc6^2) / (acc0 * acc2),  h1_up = (acc4 / acc0, acc6 / acc0)
 *     coh_lo = (acc5^2 + acc7^2) / (acc1 * acc3),  h1_lo = (acc5 / acc1, acc7 / acc1)
 * NaN where the denominator is 0.  Band sums are f64 [S][n_bands][8]: the trapezoid of psdcascade_readout.h (its f32 band
 * comparison, thread stride and reduction tree; `bands` is HOST memory, [n_bands][2], n_bands <= PSDCXR_MAX_BANDS) over the
 * stitched f32 values of rows 0 to 7, in row order.  A band that holds no bin, and every band of a pair without an included
 * stage, sums to 0.0.
 *
 * AM/PM (psdcpr_ampm, 12-row kinds).  freq is f32 [S][stride]; cab, cba, s_am, s_pm, s_am_pm, s_pm_am are f64 (re, im)
 * interleaved, row i at 2 * i * stride; carrier is f64 [S][7] = (p_ab, re w, im w, re q, im q, lock_w, lock_q).  Everything is
 * f64 and every product rounds before it is added.  cab and cba are acc * (double)gsc: the bytes of rows 8 to 11 of
 * psdc_zxampm_sidebands.
 * `carriers` is HOST memory: NULL, or [S][5] f64 = (p_ab, re w, im w, re q, im q) of each selected pair.
 *   Given:  w and q are divided by their magnitude (hypot) on the host; the locks are reported as NaN.
 *   NULL:   from the raw accumulators of bin 0 of stage 0 of the pair, whatever the MergeOpts include.  With u = (acc4[0], acc6[0])
 *           and c = (acc8[0], acc9[0]):
 *               |u| = sqrt(ur^2 + ui^2), |c| likewise,  P = |u| / ((double)count0 * (double)n * (double)n * (double)power),
 *               w = u / |u|,  q = c / |c|,  lock_w = |u| / sqrt(acc0[0] * acc2[0]),  lock_q = |c| / sqrt(acc0[0] * acc3[0])
 *           count0 the count psdc_zxampm_stage_rows reports for stage 0, power the object's f32 window power.
 * Per bin, with g = (double)gsc of the bin's stage:
 *     U = (acc4, acc6) g,  L = (acc5, acc7) g,  Cab = (acc8, acc9) g,  Cba = (acc10, acc11) g
 *     T1 = (Ur wr + Ui wi, Ui wr - Ur wi)            T2 = (Cabr qr + Cabi qi, Cabr qi - Cabi qr)
 *     T3 = (Cbar qr + Cbai qi, Cbai qr - Cbar qi)    T4 = (Lr wr + Li wi, Lr wi - Li wr)            d = 4 P
 *     s_am = (((T1 + T2) + T3) + T4) / d             s_pm = (((T1 - T2) - T3) + T4) / d             per component
 *     X = ((T1 - T2) + T3) - T4,  s_am_pm = (Xi / d, -Xr / d)
 *     Y = ((T1 + T2) - T3) - T4,  s_pm_am = (-Yi / d, Yr / d)
 * Band sums are f64 [S][n_bands][8] = the integrals of (re, im) of s_am, s_pm, s_am_pm, s_pm_am over the f64 values WITHOUT an f32
 * cast; column 2 is the integrated cross-correlated phase noise.
 * PSDC_ERR_ARG, nothing launched: carriers == NULL with an AM/PM output, the carrier output or band sums while the object's detrend
 * is not PSDC_DETREND_NONE (a detrend removes the carriers from bin 0); given carriers with a p_ab that is not > 0, a w or q that
 * is 0, or any value that is NaN or infinite.
 * Not errors: a selected pair whose stage 0 has no average, or whose |u| or |c| is 0 (an all-zero stream), gets the carrier record
 * (0, NaN x 6); its AM/PM rows are NaN, as are its band sums over bands that hold a bin; its cab, cba and freq are unaffected.  A
 * pair without an included stage still gets its carrier record.
 *
 * Launches.  info->launches is 1 without bands, 2 with bands (1 for bands alone), and 0 only when no selected pair has an
 * included stage and no carrier record is asked for (band sums are then set to 0.0 without a kernel).  The launches count in the
 * object's stats_read.
 *
 * Calls.
 *   psdcpr_layout        all four kinds; drains and fills lens, n_breaks, breaks and info; launches nothing.
 *   psdcpr_csd_device    all four kinds, outputs in device memory.
 *   psdcpr_csd           the same with HOST outputs through the object's buffer and one copy: the device form's bytes.
 *   psdcpr_ampm_device, psdcpr_ampm
 *                        12-row kinds.
 *   psdcpr_release       frees the object's read-out buffers (they are made again by the next call).
 *
 * Out of scope: the waterfall rings; the real spectral kurtosis object; two-sided reordering and dB / dBc outputs; the command
 * line tool; feeding psdcv_rows_var_device (psdcascade_var.h), which takes a psdc_handle. */
#ifndef PSDCASCADE_PAIRREAD_H
#define PSDCASCADE_PAIRREAD_H

#include "../psdcascade.h"
#include "../psdcascade_crossread.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef psdcxr_info psdcpr_info;

int psdcpr_layout(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info);
int psdcpr_csd_device(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                      float *d_saa_up, float *d_saa_lo, float *d_sbb_up, float *d_sbb_lo, float *d_sab_up, float *d_sab_lo, float *d_freq,
                      double *d_coh_up, double *d_coh_lo, double *d_h1_up, double *d_h1_lo, size_t stride, const float *bands,
                      uint32_t n_bands, double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks,
                      size_t breaks_cap, psdcpr_info *info);
int psdcpr_csd(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
               float *saa_up, float *saa_lo, float *sbb_up, float *sbb_lo, float *sab_up, float *sab_lo, float *freq, double *coh_up,
               double *coh_lo, double *h1_up, double *h1_lo, size_t stride, const float *bands, uint32_t n_bands, double *band_sums,
               size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info);
int psdcpr_ampm_device(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                       const double *carriers, float *d_freq, double *d_cab, double *d_cba, double *d_s_am, double *d_s_pm,
                       double *d_s_am_pm, double *d_s_pm_am, double *d_carrier, size_t stride, const float *bands, uint32_t n_bands,
                       double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                       psdcpr_info *info);
int psdcpr_ampm(void *h, const uint32_t *pairs, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                const double *carriers, float *freq, double *cab, double *cba, double *s_am, double *s_pm, double *s_am_pm,
                double *s_pm_am, double *carrier, size_t stride, const float *bands, uint32_t n_bands, double *band_sums, size_t *lens,
                size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdcpr_info *info);
int psdcpr_release(void *h);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_PAIRREAD_H */
