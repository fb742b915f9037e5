/* psdcascade_carrierread.h -- bank read-out on the device for the six single-channel carrier objects: the stitched sidebands of
 * every selected channel, their frequencies and band sums, for the spectral kurtosis kinds SK of both sides, for the AM/PM kinds
 * the carrier, the AM/PM split that depends on it and the band integrals of S_am and S_pm (integrated amplitude and phase noise),
 * in ONE call: one drain, one kernel launch for all channels, at most one more for the bands.  An extension of psdcascade.h in a
 * header of its own, the sibling of psdcascade_crossread.h (psdcxr_*, the same for the pair and matrix objects): the entry points
 * carry the prefix psdczr_ and live in the same library; psdcascade.h, the other extension headers, the ABI version and their
 * symbols are unchanged.
 *
 * Objects (`h` is one of these handles, passed as void *; the call looks at the object's kind and refuses every other object of
 * the cross-spectral runtime with PSDC_ERR_ARG "<name>: takes a zoom, IQ, ... object"; a handle of another runtime must not be
 * passed):
 *     psdc_zoom, psdc_iq         accumulator rows of a stage: upper, lower
 *     psdc_zsk, psdc_iqsk        S1 upper, S1 lower, S2 upper, S2 lower
 *     psdc_zampm, psdc_iqampm    upper, lower, comp re, comp im
 * Rows 0 and 1 are upper / lower in all six.
 *
 * The rules are those of psdcascade_crossread.h, word for word, with "channel" for "unit": the selection (`channels` == NULL
 * selects every channel in order, else n_sel indices in any order, duplicates allowed, at most PSDCXR_MAX_ROWS), the MergeOpts
 * triple keep_overlap / min_count / keep_transition_band, the layout outputs lens, n_breaks, breaks, breaks_cap and info,
 * PSDC_ERR_CAPACITY (lens, n_breaks and info->max_len are filled for a retry, nothing is launched, no output is written), `stride`
 * in bins with elements [lens[i], stride) of a row never written, the done_event form, "drain and nothing more, no host
 * synchronisation", the job table in two slots, and the buffers that belong to the object and go with its destroy (psdczr_release
 * frees them earlier).  lens, n_breaks and the Breaks equal what psdc_zoom_psd and its five siblings return.  Only what differs
 * is listed below.
 *
 * Errors.  A NULL handle gives PSDC_ERR_ARG and "<name>: null handle" through psdc_zoom_last_error(NULL) (or any sibling's: the
 * cross-spectral runtime keeps one text a thread).  The texts of the argument rules are those of psdcascade_crossread.h.
 *
 * Values.  upper / lower = (float)acc[r][k] * gsc and freq = (float)k * rbw with the two f32 factors of psdcascade_crossread.h:
 * the bytes of psdc_zoom_psd (and siblings) and of psdc_frequencies.
 *
 * Band sums.  The trapezoid of psdcascade_readout.h (its f32 band comparison, thread stride and reduction tree; `bands` is HOST
 * memory, [n_bands][2], n_bands <= PSDCXR_MAX_BANDS) on the stitched f32 rows: psdczr_sides gives [S][n_bands][2] f64 = (upper,
 * lower); psdczr_ampm gives [S][n_bands][4] = (upper, lower, s_am, s_pm), where the last two integrate the f64 values of the same
 * bins WITHOUT an f32 cast.  A band that holds no bin, and every band of a channel without an included stage, sums to 0.0.  The sk
 * calls have no bands (psdczr_sides takes an SK object).
 *
 * Spectral kurtosis (psdczr_sk, SK kinds).  sk_upper / sk_lower are f64 [S][stride]: of the same stage and bin as the stitched
 * value, with M the count the Break of that stage reports (what psdc_zsk_sk uses, so the bytes are its bytes),
 *     sk = M < 2 || s1 == 0 ? NaN : (M + 1) / (M - 1) * (M * s2 / (s1 * s1) - 1)
 *
 * AM/PM (psdczr_ampm, AM/PM kinds).  s_am, s_pm are f64 [S][stride]; s_ampm is f64 (re, im) interleaved, row i at 2 * i * stride;
 * carrier is f64 [S][4] = (power, u re, u im, lock).  Everything is f64 and every product rounds before it is added.
 * `carriers` is HOST memory: NULL, or [S][2] f64 = the complex amplitude A of the baseband carrier of each selected channel.
 *   Given:  P = re^2 + im^2, u = (A A) / P, formed on the host; lock is reported as NaN.
 *   NULL:   from the raw accumulators of bin 0 of stage 0 of the channel, whatever the MergeOpts include:
 *               mag = sqrt(cr0^2 + ci0^2),  P = mag / ((double)count0 * (double)n * (double)n * (double)power),
 *               u = (cr0 / mag, ci0 / mag),  lock = mag / sqrt(U0 * L0)
 *           count0 the count psdc_zampm_stage_rows reports for stage 0, power the object's f32 window power.
 * Per bin, with g = (double)gsc of the bin's stage:
 *     Us = U g, Ls = L g, cr = CR g, ci = CI g;  Dr = cr ur + ci ui,  Di = ci ur - cr ui,  mean = 0.5 (Us + Ls)
 *     s_am = (mean + Dr) / (2 P),  s_pm = (mean - Dr) / (2 P),  s_ampm = (Di / (2 P), (Ls - Us) / (4 P))
 * PSDC_ERR_ARG, nothing launched: carriers == NULL with an AM/PM output, the carrier output or band sums while the object's detrend
 * is not PSDC_DETREND_NONE (a detrend removes the carrier from bin 0); a given amplitude that is 0, NaN or infinite.  Band sums
 * are refused there as a whole because columns 2 and 3 need the carrier: an AM/PM object under a detrend gets the band sums of
 * upper / lower alone, without carriers, from psdczr_sides (or its upper / lower / freq rows from psdczr_ampm without bands).
 * Not errors: a selected channel whose stage 0 has no average, or whose comp[0] is 0 (an all-zero stream), gets the carrier
 * record (0, NaN, NaN, NaN); its AM/PM rows are NaN, as are its AM/PM band sums over bands that hold a bin; its upper / lower are
 * unaffected.  A channel without an included stage still gets its carrier record.
 *
 * Launches.  info->launches is 1 without bands, 2 with bands (1 for bands alone), and 0 only when no selected channel has an
 * included stage and no carrier record is asked for (band sums are then set to 0.0 without a kernel).  The launches count in the
 * object's stats_read.
 *
 * Calls.
 *   psdczr_layout        all six kinds; drains and fills lens, n_breaks, breaks and info; launches nothing.
 *   psdczr_sides_device  all six kinds.  d_upper, d_lower, d_freq: f32 [S][stride] on the device, each optional; d_band_sums f64
 *                        [S][n_bands][2] (NULL with n_bands == 0); at least one output.
 *   psdczr_sides         the same with HOST outputs through the object's buffer and one copy: the device form's bytes.
 *   psdczr_sk_device, psdczr_sk
 *                        SK kinds: the three outputs above and sk_upper, sk_lower.
 *   psdczr_ampm_device, psdczr_ampm
 *                        AM/PM kinds: the three outputs above, s_am, s_pm, s_ampm, carrier and band_sums [S][n_bands][4].
 *   psdczr_release       frees the object's read-out buffers (they are made again by the next call).
 *
 * Out of scope: the real spectral kurtosis object (psdc_sk); the pair kinds (psdc_zcsd, psdc_iqcsd, psdc_zxampm, psdc_iqxampm),
 * which ext/psdcascade_pairread.h reads; the waterfall rings; two-sided reordering and dB / dBc outputs; the command line tool; feeding
 * psdcv_rows_var_device (psdcascade_var.h), which takes a psdc_handle. */
#ifndef PSDCASCADE_CARRIERREAD_H
#define PSDCASCADE_CARRIERREAD_H

#include "psdcascade.h"
#include "psdcascade_crossread.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef psdcxr_info psdczr_info;

int psdczr_layout(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_sides_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                        float *d_upper, float *d_lower, float *d_freq, size_t stride, const float *bands, uint32_t n_bands,
                        double *d_band_sums, void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap,
                        psdczr_info *info);
int psdczr_sides(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                 float *upper, float *lower, float *freq, size_t stride, const float *bands, uint32_t n_bands, double *band_sums,
                 size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_sk_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                     float *d_upper, float *d_lower, float *d_freq, double *d_sk_upper, double *d_sk_lower, size_t stride,
                     void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_sk(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
              float *upper, float *lower, float *freq, double *sk_upper, double *sk_lower, size_t stride, size_t *lens, size_t *n_breaks,
              psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_ampm_device(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                       const double *carriers, float *d_upper, float *d_lower, float *d_freq, double *d_s_am, double *d_s_pm,
                       double *d_s_ampm, double *d_carrier, size_t stride, const float *bands, uint32_t n_bands, double *d_band_sums,
                       void *done_event, size_t *lens, size_t *n_breaks, psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_ampm(void *h, const uint32_t *channels, uint32_t n_sel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                const double *carriers, float *upper, float *lower, float *freq, double *s_am, double *s_pm, double *s_ampm,
                double *carrier, size_t stride, const float *bands, uint32_t n_bands, double *band_sums, size_t *lens, size_t *n_breaks,
                psdc_break *breaks, size_t breaks_cap, psdczr_info *info);
int psdczr_release(void *h);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_CARRIERREAD_H */
