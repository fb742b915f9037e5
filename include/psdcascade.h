/*
 * psdcascade.h -- C ABI of the MI355X-native cascaded PSD estimator.
 *
 * Drop-in boundary for the hot path of quartiq/stabilizer-stream src/psd.rs
 * (`Psd<N>` / `PsdCascade<N>`).  The reference has no FFI of its own; the
 * boundary is the Rust type surface its binaries use.
 * Each entry point below names the reference item it replaces (file:line under
 * the reference checkout).  INTEGRATION.md shows the Rust `extern "C"` shim and
 * the `PsdCascade<N>` wrapper a maintainer would add on the reference side.
 *
 * Conventions
 *   - opaque handle, plain pointers and sizes, int status: 0 ok, <0 error
 *     (PSDC_ERR_*).  Nothing unwinds across the ABI.  Where the reference
 *     panics on misuse (assert!/unimplemented!, src/psd.rs:110,138,139,247) the
 *     call returns an error and `psdc_last_error` describes it; the Rust shim
 *     turns that back into panic!.
 *   - a handle is used from one thread at a time (like `&mut self`); it may be
 *     moved between threads (Send, not Sync).  Distinct handles are independent.
 *   - one handle holds `n_channels` independent cascades (one `PsdCascade` per
 *     trace, src/bin/psd.rs:174-182) that are batched onto one GPU.
 *   - all sample data is IEEE f32, native endian (src/bin/stream_to_raw.rs:24-25), except the integer feeds below
 *     ("integer sample feeds").
 *   - there is NO CPU fallback: without a usable HIP device `psdc_create` fails.
 *   - call chunking: like the reference (src/psd.rs:196-208) every result is a function of the CONCATENATED stream of a
 *     channel.  Counters (stage count, count, pending, processed, Break fields, frequencies, Loss) are exactly independent of
 *     how the stream was cut into process() calls.  Spectra are independent of it only to rounding: the reference adds
 *     segment after segment into one f32 accumulator and is bit-identical under any chunking; here the segments a call brings
 *     are summed in groups (per workgroup run in f32, across runs in f64, one f32 add into the accumulator per round) whose
 *     boundaries follow the calls, so two chunkings of one stream agree to <= 2e-6 relative per bin (asserted by
 *     tests/test_gpu_parity.py::test_chunking_invariance).  The same stream fed by the same CALLS is bit-reproducible, run to
 *     run and whatever the host's timing (tests/test_gpu_parity.py::test_same_calls_same_bits: the same spans with sleeps
 *     injected between the calls): which device spans share a round -- hence the grouping of the sums -- is decided by the call
 *     sequence alone (PSDC_OPT_COALESCE), never by how busy the device happens to be.  Only a handle switched to
 *     PSDC_OPT_EAGER gives that up: its held spans go out as soon as the device is seen idle, so its round composition
 *     follows host timing and repeated runs agree to the same <= 2e-6, not to the bit (host-fed samples and one-span feeds
 *     stay bit-reproducible there too).  This is stated for an environment with none of the library's A/B and debugging
 *     switches set (PSDC_NO_*, PSDC_DBG_*, PSDC_FFT3: tools/README.md); they are read when a handle is made.
 *     Either grouping is closer to the exact sum than the reference's sequential f32 accumulation.
 */
#ifndef PSDCASCADE_H
#define PSDCASCADE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSDC_ABI_VERSION 3

/* status codes */
#define PSDC_OK 0
#define PSDC_ERR_ARG (-1)           /* bad argument (reference: assert!/index panic) */
#define PSDC_ERR_DEVICE (-2)        /* HIP error / no device */
#define PSDC_ERR_NOMEM (-3)
#define PSDC_ERR_UNIMPLEMENTED (-4) /* Detrend::Linear: unimplemented!() src/psd.rs:110 */
#define PSDC_ERR_FRAME_HEADER (-5)  /* de::Error::InvalidHeader  src/de/frame.rs:27-29 */
#define PSDC_ERR_FRAME_FORMAT (-6)  /* de::Error::UnknownFormat  src/de/frame.rs:30 */
#define PSDC_ERR_FRAME_SIZE (-7)    /* de::Error::PayloadSize / batches mismatch src/de/data.rs:23-24 */
#define PSDC_ERR_CAPACITY (-8)      /* caller-provided output too small */

/* Window<N> constructors (src/psd.rs:24-32, :42-55) */
#define PSDC_WINDOW_RECTANGULAR 0
#define PSDC_WINDOW_HANN 1
#define PSDC_WINDOW_CUSTOM 2 /* a caller-built Window<N> (pub fields, src/psd.rs:12-20): psdc_create_window */

/* `device` argument of the constructors: a HIP device index, or PSDC_DEVICE_DEFAULT = the index in the
 * environment variable PSDC_DEVICE (0 when unset) -- what a shim whose constructor has no device argument
 * (PsdCascade::<N>::default(), src/psd.rs:408) passes, so that one process per GPU selects its device from outside. */
#define PSDC_DEVICE_DEFAULT (-1)

/* Detrend (src/psd.rs:59-72) */
#define PSDC_DETREND_NONE 0
#define PSDC_DETREND_MIDPOINT 1
#define PSDC_DETREND_SPAN 2
#define PSDC_DETREND_MEAN 3
#define PSDC_DETREND_LINEAR 4 /* accepted by the enum, rejected like the reference */

/* DEPTH (src/psd.rs:117): each stage decimates by 1 << 3 */
#define PSDC_DEPTH 3

/* options for psdc_configure */
#define PSDC_OPT_QUANTUM 1 /* host-fed samples buffered per channel before a launch (default 1<<22) */
#define PSDC_OPT_COALESCE 3 /* in-place device spans of a channel that share one round (1..16; default: 8 -- more of short spans,
                             * so that a round of all channels holds ~2^28 samples and stays one launch -- and at most 2^29 samples a channel; a handle of ONE channel: 16 and at most 2^30 samples, and of f32 spans shorter than 2^24 samples
                             * as many as make a round of ~2^28 samples, up to 128 -- a round costs 5 ... 20 us whatever it holds;
                             * 1 = every span its own round).  A span is HELD until its channel holds that many samples or a call arrives
                             * that cannot join them (one span more than that many, host-fed or short spans, settings changes, every
                             * read-out, psdc_flush, psdc_sync, psdc_record_consumed): which spans share a round depends on the calls alone, so results are
                             * bit-reproducible.  Held spans are caller memory the library has not read yet: the rule of
                             * psdc_process_device (unmodified until sync / read-out / consumed event) covers them.
                             * (-k is accepted and means k: through ABI 3's first builds it asked for exactly this hold.) */
#define PSDC_OPT_MERGE 6 /* 1 (default): a device span that starts where the last HELD span of its channel ends (d_x == previous d_x +
                          * previous len: a ring or capture buffer handed over piece by piece) extends that span instead of becoming
                          * one of its own -- no seam between them, whatever the call size; a span stops growing at 2^29 samples.
                          * 0: every call is a span of its own (tests of the multi-span planner). */
#define PSDC_OPT_EAGER 5 /* 1: a held span also goes out as soon as the device is seen idle (hipStreamQuery) -- the first span of a
                          * burst starts at once instead of waiting for its round to fill, at the price of a round composition
                          * that follows host timing: repeated runs then agree to rounding (<= 2e-6), not to the bit.  Default 0. */
#define PSDC_OPT_PROFILE 2 /* 1: time the dominant kernel with HIP events (psdc_profile_read) */
#define PSDC_OPT_MIN_PAIRS 4 /* segment pairs a decimated stage (k >= 1) collects before it issues work on the ingest
                              * path (default 32 x teams per workgroup: 256 at n = 1024; 0 = issue at once).  Read-outs,
                              * psdc_flush and psdc_sync always issue everything: results do not depend on it. */

typedef struct psdc_handle psdc_handle;

/* Break (src/psd.rs:290-311); `bins: Range<usize>` is flattened. */
typedef struct psdc_break {
    uint64_t start;      /* start index in PSD and frequencies */
    uint32_t include;    /* was included in output */
    uint32_t count;      /* number of averages */
    uint32_t avg;        /* averaging limit */
    uint32_t _pad;
    uint64_t bins_start; /* FFT bins [bins_start, bins_end) */
    uint64_t bins_end;
    uint64_t fft_size;
    uint64_t decimation;
    uint64_t pending;    /* unprocessed input samples (includes overlap) */
    uint64_t processed;  /* total samples processed (excluding overlap) */
} psdc_break;

/* PsdStage accessors (src/psd.rs:271-287) + Break bookkeeping in one record */
typedef struct psdc_stage_stat {
    uint32_t count; /* PsdStage::count  src/psd.rs:275-277; saturates at u32::MAX where the reference's
                     * u32 wraps after 2^32 segments (the library counts in 64 bits; gain() follows that) */
    uint32_t avg;   /* Psd::avg         src/psd.rs:133 */
    uint64_t pending;   /* PsdStage::buf().len()  src/psd.rs:285-287 */
    uint64_t processed; /* src/psd.rs:511-512 */
} psdc_stage_stat;

typedef struct psdc_profile {
    uint64_t launches;      /* dominant-kernel launches bracketed so far */
    double kernel_ms;       /* sum of their HIP-event durations */
    uint64_t samples;       /* input samples those launches consumed (all stages) */
    uint64_t stage0_samples;/* of which stage-0 (raw stream) samples */
} psdc_profile;

/* ---- lifecycle ----------------------------------------------------------- */

/* PsdCascade::<N>::default() (src/psd.rs:408-423) for `n_channels` traces on HIP
 * device `device`.  n: a power of two 16 ... 131072, or ANY size 16 < n <= 8192 (the reference takes any
 * N >= 2 with (N - overlap) % 8 == 0, src/psd.rs:138,247 -- rustfft plans any length, :418; with the Hann
 * window's overlap N/2 that is every multiple of 16).  Returns NULL on failure; psdc_last_error(NULL)
 * explains.
 * Which kernels run: the single-pass fused kernels (stream read once: detrend +
 * window + FFT + |X|^2 + /8 decimator in one launch) exist for n = 256 ... 16384 (powers of two) and every window
 * whose overlap is n / 2 -- the HANN window (what the reference's binaries and BASELINE configs use) and caller-built
 * tables with that overlap; they read the table and assume only the hop -- or 0: Window::rectangular() and caller-built
 * tables without overlap, where two disjoint segments share one transform (faster than the Hann path: half the FFT work).
 * Caller-built windows of another overlap, n < 256 and sizes that are not powers of two take the generic
 * two-pass kernels (welch + hbf_dec8: same results, the stream is read twice, about half the rate;
 * sizes that are not powers of two evaluate the DFT in chirp-z form on a power-of-two transform of at
 * least twice the length: two such transforms per segment pair); the powers of two 32768 ... 131072 a four-step FFT with
 * one intermediate frame in device memory (100 ... 120 GS/s, +256 MiB per handle). */
psdc_handle *psdc_create(uint32_t n, int window_kind, uint32_t n_channels, int device);

/* The same with a caller-supplied `Window<N>` -- the struct is public with public fields `win`, `power`,
 * `nenbw`, `overlap` (src/psd.rs:12-20) and `Psd::new(fft, win)` takes any (src/psd.rs:137) --: `win` holds n
 * f32 weights (host memory, copied), `power` / `nenbw` feed gain() (src/psd.rs:279-283), `overlap` the segment
 * hop.  The reference asserts (n - overlap) % 8 == 0 when the first segment is decimated (src/psd.rs:246-247);
 * here that -- and overlap < n -- is checked at construction (PSDC_ERR_ARG through psdc_last_error(NULL)).
 * A table that compares equal, bit for bit and in its three constants, to Window::hann() or
 * Window::rectangular() is recognised as such; any table with overlap == n / 2 (Hann, a caller's Hamming,
 * Blackman, ...) runs the single-pass fused kernels, any other overlap the generic two-pass kernels (same
 * results, about half the rate). */
psdc_handle *psdc_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap,
                                uint32_t n_channels, int device);

/* The Window of a handle as the library holds it: kind (PSDC_WINDOW_*), constants, and the n weights
 * (win may be NULL).  What a gather of raw spectra needs beside them to run the stitch elsewhere. */
int psdc_window_get(const psdc_handle *h, int *kind, float *power, float *nenbw, size_t *overlap, float *win);

/* Window::hann() / Window::rectangular() (src/psd.rs:24-55) as the library builds them: n weights + constants
 * (pure host; any n >= 2).  For callers that want to derive a table from them or compare. */
int psdc_window_table(uint32_t n, int window_kind, float *win, float *power, float *nenbw, size_t *overlap);

/* Drop (src/bin/psd.rs:190 `dec.clear()`). */
void psdc_destroy(psdc_handle *h);

/* #[derive(Clone)] (src/psd.rs:399): deep copy of every channel's state. */
psdc_handle *psdc_clone(psdc_handle *h);

/* Cmd::Reset (src/bin/psd.rs:190): forget all stages of all channels, keep settings. */
int psdc_reset(psdc_handle *h);

int psdc_configure(psdc_handle *h, int option, int64_t value);

/* ---- settings ------------------------------------------------------------ */

/* PsdCascade::set_detrend (src/psd.rs:438-443); applies to segments completed
 * after the call (pending complete segments are flushed first). */
int psdc_set_detrend(psdc_handle *h, int detrend_kind);

/* PsdCascade::set_avg(AvgOpts{limit, count}) (src/psd.rs:431-436); stage i uses
 * min(count >> (3 i), limit). */
int psdc_set_avg(psdc_handle *h, uint32_t limit, uint32_t count);

/* ---- ingest -------------------------------------------------------------- */

/* PsdCascade::process(&[f32]) (src/psd.rs:456-468) for one channel.  `x` is host
 * memory and is copied before returning.  GPU work may be deferred until
 * PSDC_OPT_QUANTUM samples are buffered or a read-out/flush happens; results
 * depend only on the concatenated stream, not on call chunking (counters exactly, spectra to rounding: Conventions). */
int psdc_process(psdc_handle *h, uint32_t channel, const float *x, size_t len);

/* Same, but `d_x` is device memory on the handle's device and is read in place
 * (no staging copy).  The work is enqueued asynchronously on the handle's own stream, possibly
 * after this call returns (PSDC_OPT_COALESCE): whatever produced `d_x` must have COMPLETED before
 * the call (host-synchronised; or use psdc_process_device_after), and `d_x` must stay valid and
 * unmodified until psdc_sync()/any read-out returns or a psdc_record_consumed event completes. */
int psdc_process_device(psdc_handle *h, uint32_t channel, const float *d_x, size_t len);

/* psdc_process_device for a producer that runs on ANOTHER HIP stream (a decode kernel, torch's
 * current stream, ...).  The handle works on a private non-blocking stream and, with
 * PSDC_OPT_COALESCE, may not even have enqueued the kernels that read `d_x` when the call
 * returns, so plain psdc_process_device requires that the producer has FINISHED (host-synchronised)
 * before the call.  Here `producer_event` -- a hipEvent_t the caller recorded behind the work that
 * writes d_x, passed as void*; NULL = none -- is waited for on the device by the handle's stream
 * before anything reads the span: no host synchronisation. */
int psdc_process_device_after(psdc_handle *h, uint32_t channel, const float *d_x, size_t len,
                              void *producer_event);

/* The other direction: enqueue everything held so far and record `consumed_event` (hipEvent_t as
 * void*) on the handle's stream.  When it has completed, every span handed to psdc_process_device*
 * before this call has been read for the last time and its memory may be overwritten (the producer
 * waits for it with hipStreamWaitEvent).  Does not wait on the host. */
int psdc_record_consumed(psdc_handle *h, void *consumed_event);

/* Frame::from_bytes + AdcDac::traces (src/de/frame.rs:49-60, src/de/data.rs:11-82)
 * + process() of the four traces ADC0, ADC1, DAC0, DAC1 into channels 0..3
 * (src/bin/psd.rs:174-182), for `n_frames` frames of `frame_size` bytes each,
 * as read by Source::get for Data::File (src/source.rs:135-142).  Host memory.
 * Headers are validated on the host; payloads are de-interleaved on the device.
 * On a bad frame: frames before it are ingested, *n_ok says how many, and the
 * frame's de::Error is returned.  Needs n_channels >= 4. */
int psdc_process_adcdac_frames(psdc_handle *h, const uint8_t *frames, size_t frame_size,
                               size_t n_frames, size_t *n_ok);

/* Frame::from_bytes + Payload::traces for ANY of the reference's four payload formats (src/de/mod.rs:12-17,
 * src/de/frame.rs:49-60, src/de/data.rs): AdcDac (id 1: traces ADC0, ADC1, DAC0, DAC1, eight samples per batch), Fls (2: AR, AP,
 * BI, BQ), ThermostatEem (3: T00, T20, I0, I1), Mpll (4: "phase (rad)", "frequency (kHz)", "amplitude (V/G10)") -- one sample
 * per batch for the last three --, + Loss::update + process() of trace i into channel i (src/bin/psd.rs:174-182: the trace's
 * index picks the cascade, whatever the frame's format), for `n_frames` frames of `frame_size` bytes each in host memory.
 * The format is each frame's own (header byte 2); the frames of a call are taken in runs of one format, headers validated on
 * the host, payloads decoded on the device -- the decoded traces are bit-identical to Payload::traces (same f32 operations in
 * the same order).  On a bad frame: frames before it are ingested, *n_ok says how many, and the frame's de::Error is returned
 * (PSDC_ERR_FRAME_HEADER / _FORMAT / _SIZE).  Needs n_channels >= the traces of every format met (4, 4, 4, 3), else
 * PSDC_ERR_ARG at the first frame that carries more.  (The reference CLI's default --frame-size 1448 is 60 Mpll batches,
 * src/source.rs:31.)  psdc_process_adcdac_frames is this call restricted to AdcDac. */
int psdc_process_frames(psdc_handle *h, const uint8_t *frames, size_t frame_size, size_t n_frames, size_t *n_ok);

/* The same for frames that already sit in device memory (a capture buffer filled by a NIC / another kernel).
 * Headers: Header::parse and the AdcDac size checks of every frame plus the Loss sums are ONE small launch on a side stream
 *   of the handle; the call waits for that launch alone, so `*n_ok` and the returned de::Error are final when it returns.
 * Payloads: at every size with a fused kernel (powers of two 256 ... 16384, windows with overlap n/2) the four traces are
 *   read IN PLACE, as wire words, by the stage-0 loads of the fused kernels -- the f32 traces never exist in memory --, under
 *   the same rules as psdc_process_device: spans may be held back and share a round with later calls (PSDC_OPT_COALESCE), and
 *   the seam / tail of a span is read by the FIRST launch of the next round, i.e. possibly after this call AND the next one
 *   have returned.  Elsewhere (other sizes and windows, pieces shorter than 4 (n + 288) samples per trace) a decode kernel
 *   writes the four traces into the stage-0 stream buffers.
 * Lifetime: d_frames must stay valid and its PAYLOAD bytes unmodified until psdc_sync(), any read-out, or an event from
 *   psdc_record_consumed has completed.  The 8 header bytes of each frame are read by this call's verdict launch only, which
 *   has completed when the call returns: a ring that re-stamps `seq` words (or a replay that moves them on, bench.py
 *   FrameReplay) may rewrite headers as soon as the call is back
 *   (tests/test_gpu_frames_inplace.py::test_headers_may_change_once_the_call_has_returned).  Ordering: the handle works on its own non-blocking streams and there is no implicit null-stream order:
 *   the producer of d_frames must have COMPLETED before the call (or use psdc_process_device_after's event for f32 spans).
 * Alignment: any base address is accepted.  The in-place path needs d_frames to be a multiple of 8 bytes (frame_size =
 *   8 + 64 batches keeps every later frame aligned); other bases take the byte-wise decode kernel -- same results, slower. */
int psdc_process_adcdac_frames_device(psdc_handle *h, const uint8_t *d_frames, size_t frame_size,
                                      size_t n_frames, size_t *n_ok);

/* psdc_process_frames for frames that already sit in device memory: any of the four formats, in runs.  The headers (8 of every
 * frame_size bytes) are gathered into pinned memory by one small kernel on a side stream and validated on the host; the payloads stay on the device -- Fls /
 * ThermostatEem / Mpll runs are decoded straight from `d_frames` into the stage-0 streams, AdcDac runs take
 * psdc_process_adcdac_frames_device (whose lifetime, ordering and alignment rules apply to the whole call: d_frames valid and
 * unmodified until psdc_sync() / a read-out / a psdc_record_consumed event, its producer COMPLETED before the call). */
int psdc_process_frames_device(psdc_handle *h, const uint8_t *d_frames, size_t frame_size, size_t n_frames, size_t *n_ok);

/* Loss (src/loss.rs:3-26): sequence-gap accounting over the frames ingested by
 * psdc_process_frames / psdc_process_adcdac_frames[_device].  received counts batches; dropped the batches missing
 * between consecutive frames (u32 wrapping_sub); gaps are counted, never zero-filled. */
typedef struct psdc_loss {
    uint64_t received;
    uint64_t dropped;
    uint32_t next_seq;  /* seq expected from the next frame */
    uint32_t have_seq;  /* 0 until the first frame was seen */
} psdc_loss;

int psdc_loss_read(psdc_handle *h, psdc_loss *out, int reset);

/* Enqueue every complete segment of every stage now (does not wait). */
int psdc_flush(psdc_handle *h);

/* Wait until all enqueued device work of this handle has finished. */
int psdc_sync(psdc_handle *h);

/* ---- read-out (each implies flush + sync) -------------------------------- */

/* PsdCascade.stages.len() (src/psd.rs:401,445-453): stages are created when
 * the first sample reaches them. */
int psdc_num_stages(psdc_handle *h, uint32_t channel);

int psdc_stage_info(psdc_handle *h, uint32_t channel, uint32_t stage, psdc_stage_stat *out);

/* PsdStage::spectrum (src/psd.rs:271-273): n/2+1 un-normalised accumulators. */
int psdc_stage_spectrum(psdc_handle *h, uint32_t channel, uint32_t stage, float *out);

/* PsdStage::gain (src/psd.rs:279-283). */
int psdc_stage_gain(psdc_handle *h, uint32_t channel, uint32_t stage, float *out);

/* PsdStage::buf (src/psd.rs:285-287): the pending input samples of a stage. */
int psdc_stage_buf(psdc_handle *h, uint32_t channel, uint32_t stage, float *out, size_t cap,
                   size_t *len);

/* Bulk read-out of one channel: stage count, per-stage records and the raw accumulators of
 * every stage (stage 0 first, n/2+1 floats each) with one flush, one sync and one copy.
 * stats / spectra may be NULL; cap = stages the caller has room for.  What a multi-GPU
 * gather or a GUI refresh (src/bin/psd.rs:201) needs per trace. */
int psdc_read_channel(psdc_handle *h, uint32_t channel, uint32_t cap, uint32_t *n_stages,
                      psdc_stage_stat *stats, float *spectra);

/* PsdCascade::psd(&MergeOpts) (src/psd.rs:479-543).  psd_out needs room for
 * num_stages*(n/2+1) floats, breaks for num_stages records (lowest rate first).
 * Either output pointer may be NULL to query sizes only. */
int psdc_psd(psdc_handle *h, uint32_t channel, int keep_overlap, uint32_t min_count,
             int keep_transition_band, float *psd_out, size_t psd_cap, size_t *psd_len,
             psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);

/* PsdCascade::rbw (src/psd.rs:427-429). */
float psdc_rbw(const psdc_handle *h);

/* ---- Psd<N>: one stage (src/psd.rs:122-288) ------------------------------ */

/* `Psd<N>` with its `PsdStage` trait (src/psd.rs:163-193), the type the reference's own test
 * drives directly (src/psd.rs:615-632).  Same kernels as the cascade: one stage analyses the
 * stream, and the /8-decimated stream it emits is handed back instead of feeding a next stage. */
typedef struct psdc_stage psdc_stage;

/* Psd::new(fft, win) (src/psd.rs:137-152): the FFT plan is the library's own (n as in psdc_create),
 * window_kind one of PSDC_WINDOW_*; detrend None, avg = u32::MAX, drain = hbf_dec_response_length(3). */
psdc_stage *psdc_stage_create(uint32_t n, int window_kind, int device);
/* Psd::new(fft, win) (src/psd.rs:137-152) with the caller's Window<N> (see psdc_create_window); the FFT plan
 * argument of the reference has no counterpart: the library's own FFT of length n is used, and the shim keeps the
 * reference's assert_eq!(N, fft.len()) (src/psd.rs:139) on its side. */
psdc_stage *psdc_stage_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap,
                                     int device);
void psdc_stage_destroy(psdc_stage *s);
psdc_stage *psdc_stage_clone(psdc_stage *s); /* #[derive(Clone)] src/psd.rs:122 */
int psdc_stage_set_avg(psdc_stage *s, uint32_t avg);             /* Psd::set_avg      src/psd.rs:154-156 */
int psdc_stage_set_detrend(psdc_stage *s, int detrend_kind);      /* Psd::set_detrend  src/psd.rs:158-160 */

/* PsdStage::process(x, y) -> &mut y[..n] (src/psd.rs:196-269): buffers x, completes every full
 * segment (detrend, window, FFT, accumulate), decimates the samples new to each segment by 8 and
 * writes the outputs -- minus the one-time drain of hbf_dec_response_length(3) -- to y; *n_out is
 * the length of the returned slice.  It depends only on the samples fed so far: after T samples in
 * total, (N + (J-1)(N-overlap))/8 - 35 outputs have been returned, J the segments completed.  cap <
 * that many new outputs fails with PSDC_ERR_CAPACITY where the reference panics on the slice index
 * (src/psd.rs:253).  x and y are host memory. */
int psdc_stage_process(psdc_stage *s, const float *x, size_t len, float *y, size_t cap, size_t *n_out);

/* The same with x and y in device memory (y complete and x free to reuse on return). */
int psdc_stage_process_device(psdc_stage *s, const float *d_x, size_t len, float *d_y, size_t cap,
                              size_t *n_out);

int psdc_stage_get_spectrum(psdc_stage *s, float *out /* n/2+1 */); /* PsdStage::spectrum src/psd.rs:271-273 */
int psdc_stage_get_count(psdc_stage *s, uint32_t *count);           /* PsdStage::count    src/psd.rs:275-277 */
int psdc_stage_get_gain(psdc_stage *s, float *gain);                /* PsdStage::gain     src/psd.rs:279-283 */
int psdc_stage_get_buf(psdc_stage *s, float *out, size_t cap, size_t *len); /* PsdStage::buf src/psd.rs:285-287 */
const char *psdc_stage_last_error(const psdc_stage *s);

/* ---- pure host helpers (no device needed) -------------------------------- */

/* Break::frequencies (src/psd.rs:315-327).  Returns the number written, or the
 * number required if out is NULL / cap too small. */
size_t psdc_frequencies(const psdc_break *breaks, size_t n_breaks, float *out, size_t cap);

/* idsp::hbf::hbf_dec_response_length(depth) (src/psd.rs:149,622). */
int psdc_hbf_response_length(int depth);

/* The stitch of PsdCascade::psd (src/psd.rs:479-543) on caller-provided stage
 * data: spectra is n_stages rows of (n/2+1) floats, stage 0 (highest rate)
 * first; window_kind selects nenbw/power/overlap.  Used by psdc_psd and by
 * multi-GPU read-out after a gather of raw spectra. */
int psdc_stitch(uint32_t n, int window_kind, uint32_t n_stages, const uint32_t *counts,
                const uint32_t *avgs, const uint64_t *pendings, const float *spectra,
                int keep_overlap, uint32_t min_count, int keep_transition_band, float *psd_out,
                size_t psd_cap, size_t *psd_len, psdc_break *breaks, size_t breaks_cap,
                size_t *n_breaks);

/* The same stitch with the window given by its constants (any Window<N>) and the counts in 64 bits: a handle
 * counts segments in 64 bits where the reference's u32 wraps (psdc_stage_stat.count saturates), and psd() divides
 * by gain() of the 64-bit count; a gathered read-out must do the same to equal single-GPU psd() past 2^32
 * segments.  `counts` (u32, as reported) fills Break.count / Break.processed. */
int psdc_stitch_window(uint32_t n, float power, float nenbw, size_t overlap, uint32_t n_stages,
                       const uint64_t *counts64, const uint32_t *avgs, const uint64_t *pendings,
                       const float *spectra, int keep_overlap, uint32_t min_count, int keep_transition_band,
                       float *psd_out, size_t psd_cap, size_t *psd_len, psdc_break *breaks, size_t breaks_cap,
                       size_t *n_breaks);

/* ---- read-out for a gather (multi-GPU, src/bin/psd.rs:174-182 one cascade per trace) ------------------
 * One trace per cascade shards by channel: every GPU (one process per GPU, or one process with one handle per
 * device) runs whole cascades and nothing is exchanged during ingest.  At read-out every shard packs its raw
 * accumulators and counters into a flat, fixed-size byte record -- psdc_readout_bytes(n, n_channels) bytes,
 * the same on every shard with the same n and channel count, so one all-gather / gather of equal blocks over
 * ANY transport (RCCL ncclAllGather on device copies, MPI, a socket, or plain memcpy between the handles of one
 * process) collects them -- and the receiver stitches any channel of any record with psdc_unpack_stitch:
 * bit-identical to psdc_psd on the shard itself (raw accumulators travel, normalisation happens after).
 * A record is UNTRUSTED input to the psdc_unpack_* calls: every header field is held to the range the library can produce
 * (2 <= n <= 131072, n_channels <= 4096, overlap < n, power and nenbw > 0, stage counts <= 16) and the length to what those
 * fields imply, before anything is indexed; a record that fails is PSDC_ERR_ARG, never an out-of-bounds read.
 * psdc_readout_bytes returns 0 for dimensions outside those ranges (no such record exists). */
size_t psdc_readout_bytes(uint32_t n, uint32_t n_channels);
/* flush + sync + copy: fills `buf` (cap >= psdc_readout_bytes(n, n_channels) of this handle) */
int psdc_pack_readout(psdc_handle *h, void *buf, size_t cap, size_t *len);
/* The same record built from stage data the caller holds (pure host): psdc_pack_init writes the header of an empty
 * record of n_channels channels (no stages), psdc_pack_channel fills one channel (stage 0 first; spectra =
 * n_stages rows of n/2+1 floats).  psdc_pack_readout is these two over a handle's own state. */
int psdc_pack_init(void *buf, size_t cap, uint32_t n, float power, float nenbw, size_t overlap, uint32_t n_channels);
int psdc_pack_channel(void *buf, size_t len, uint32_t channel, uint32_t n_stages, const uint64_t *counts64,
                      const uint32_t *avgs, const uint64_t *pendings, const float *spectra);
/* A record copied into a larger one of `n_channels` channels, the added ones empty (no stages): a gather moves equal blocks,
 * so with channels % world != 0 every shard pads its record to the largest shard's channel count.  Pure host; the counters stay
 * the 64-bit ones.  cap >= psdc_readout_bytes(n, n_channels); out must not alias rec. */
int psdc_pack_pad(const void *rec, size_t len, void *out, size_t cap, uint32_t n_channels);
/* record header: FFT size, channels in the record, stages of `channel` (pure host) */
int psdc_unpack_info(const void *buf, size_t len, uint32_t channel, uint32_t *n, uint32_t *n_channels,
                     uint32_t *n_stages);
/* PsdCascade::psd (src/psd.rs:479-543) of one channel of a packed record (pure host; outputs as psdc_psd) */
int psdc_unpack_stitch(const void *buf, size_t len, uint32_t channel, int keep_overlap, uint32_t min_count,
                       int keep_transition_band, float *psd_out, size_t psd_cap, size_t *psd_len,
                       psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);

/* Stream bookkeeping of src/psd.rs:196-269 in closed form: after `total`
 * samples have entered stage 0, how many stages exist and, per stage, samples
 * received, segments completed (= count when averaging is unbounded) and
 * pending samples.  Arrays hold up to `cap` stages. Returns the stage count. */
int psdc_plan_counts(uint32_t n, int window_kind, uint64_t total, uint32_t cap,
                     uint64_t *received, uint64_t *segments, uint64_t *pending);

/* Var::eval (src/var.rs:26-45) on a merged PSD (host, f32). */
float psdc_var_eval(int x_exp, int sinx_exp, float clip, size_t dc_cut, const float *phase_psd,
                    const float *frequencies, size_t n, float tau);

/* Trace::plot (src/bin/psd.rs:125-157) on a merged PSD: the Trapezoidal integrator for irregular
 * sampling (src/bin/psd.rs:98-116) runs over (frequencies[i], psd[i]); *rms = sqrt of the integral over
 * the bins with integral_start <= fs * f <= integral_end (no interpolation at the limits, like the
 * reference); the plot points -- for every bin whose f is a normal float -- are
 * x = log10(f) + log10(fs), y = integrate ? sqrt(running integral) : 10 (log10(p) - log10(fs)), written
 * as pairs of doubles to plot_xy (room for plot_cap points; NULL to skip).  Host, f32 like the reference. */
int psdc_trace_plot(const float *psd, const float *frequencies, size_t n, float fs, int integrate,
                    float integral_start, float integral_end, float *rms, double *plot_xy,
                    size_t plot_cap, size_t *n_points);

/* ---- device utilities ---------------------------------------------------- */

/* HbfDec8 block processing (src/psd.rs:246-253) of a whole host array from zero
 * state on the device: y[m], m < len/8.  Standalone check of the decimator. */
int psdc_hbf_dec8(int device, const float *x, size_t len, float *y);

/* Fill device memory with the bench/test stream: x_i = (u_i - 0.5) * sqrt(12),
 * u_i = (r_i >> 40) * 2^-24 with r_i output first_index + i of SplitMix64 seeded
 * with mix64(seed + GAMMA), i.e. r_i = mix64(key + (first_index + i + 1) * GAMMA)
 * (unit-variance uniform noise, the reference's own test signal src/psd.rs:604-606). */
int psdc_fill_noise_device(int device, float *d_x, size_t len, uint64_t seed,
                           uint64_t first_index);

int psdc_profile_read(psdc_handle *h, psdc_profile *out, int reset);

/* ---- cross-spectral density cascade ---------------------------------------------------------------------
 * The design PsdCascade's doc comment names as its model (src/psd.rs:393, `csdl`): `n_pairs` independent pairs of
 * real f32 streams (x, y), always fed together with equal lengths.  Per stage a pair is two Psd<N> stages
 * (src/psd.rs:195-269) in lockstep: the same segmentation, Window<N>, Detrend (applied to each channel's segment
 * separately), /8 half-band decimation of each channel with the drain of 35 outputs, and lazy stages
 * (src/psd.rs:445-468) -- a pair has exactly the stages and counts of a PsdCascade fed x alone.  Per bin k <= N/2 a
 * stage keeps, with the EWMA factor g of src/psd.rs:218-233:
 *     Sxx[k] = g Sxx[k] + |X[k]|^2,   Syy[k] = g Syy[k] + |Y[k]|^2,   Sxy[k] = g Sxy[k] + conj(X[k]) Y[k]
 * Sign convention: conj(X) Y, that of scipy.signal.csd(x, y): the transfer function is H1 = Sxy / Sxx, the coherence
 * |Sxy|^2 / (Sxx Syy).  The read-out is PsdCascade::psd (src/psd.rs:479-543) applied to each of the four real rows
 * (Sxx, Syy, Re Sxy, Im Sxy) with the same bins, Breaks and 1 / (gain() decimation): Sxx IS the psd() of a
 * PsdCascade fed x, and y = x gives Sxy == Sxx up to rounding.  The accumulators are f64 on the device.
 * Sizes: n a power of two 64 ... 4096; Window::hann(), Window::rectangular(), or a caller's table with
 * (n - overlap) % 8 == 0.  Anything else is PSDC_ERR_ARG (psdc_cross_last_error(NULL) says why).
 * Stream ordering: an object works on a non-blocking stream of its own.  psdc_cross_process_device copies the samples
 * on that stream; with `producer_event` (a hipEvent_t recorded behind the producer) the copy waits for it on the
 * device, without it the producer must have completed.  The caller keeps d_x / d_y unchanged until psdc_cross_sync or a
 * read-out returns.  Every call restores the caller's current device.  Counts are 64-bit as in psdc_stitch_window.
 * A process call runs one round of the pipeline: three kernel launches (the segments of every (pair, stage), the
 * decimators, the fold + stream tails) whatever the depth, as long as a round's job tables fit one launch each: 128
 * (pair, stage) segment jobs, 320 decimator jobs (two a (pair, stage)), 128 folds and 256 tail carries.  A round with
 * more -- from about 12 pairs with 10 stages each -- takes one more launch of a kind per table it overflows.  Read-outs
 * run rounds until no stage has work.
 * Memory: per (pair, stage) two ping-pong buffers per channel, each sized to the largest call the stage has seen
 * (x 1.25, never shrunk: a 2^26-sample call leaves about 1.3 GB at stage 0 of its pair), plus 64 MB of pinned host
 * staging per object. */
typedef struct psdc_cross psdc_cross;
/* PsdCascade::<N>::default() (src/psd.rs:408-423) for n_pairs pairs; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_cross *psdc_cross_create(uint32_t n, int window_kind, uint32_t n_pairs, int device);
/* the same with a caller-built Window<N> (src/psd.rs:12-20), as psdc_create_window */
psdc_cross *psdc_cross_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap,
                                     uint32_t n_pairs, int device);
void psdc_cross_destroy(psdc_cross *h);
/* back to the state of a fresh object (stages, buffers, settings and statistics) */
int psdc_cross_reset(psdc_cross *h);
/* PsdCascade::set_detrend (src/psd.rs:438-443); samples fed before the call are analysed with the old setting */
int psdc_cross_set_detrend(psdc_cross *h, int detrend_kind);
/* PsdCascade::set_avg (src/psd.rs:431-436) */
int psdc_cross_set_avg(psdc_cross *h, uint32_t limit, uint32_t count);
/* PsdCascade::process (src/psd.rs:456-468) of x and y: host memory (copied through pinned staging) */
int psdc_cross_process(psdc_cross *h, uint32_t pair, const float *x, const float *y, size_t len);
/* the same from device memory; producer_event: hipEvent_t or NULL (see Stream ordering above) */
int psdc_cross_process_device(psdc_cross *h, uint32_t pair, const float *d_x, const float *d_y, size_t len,
                              void *producer_event);
/* run every pending round and wait for the device */
int psdc_cross_sync(psdc_cross *h);
/* PsdCascade stages of a pair (src/psd.rs:400) */
int psdc_cross_num_stages(psdc_cross *h, uint32_t pair);
/* raw accumulators of one stage (PsdStage::spectrum / count, src/psd.rs:271-287): sxx, syy n/2+1 floats, sxy
 * 2(n/2+1) floats (re, im); any may be NULL */
int psdc_cross_stage_spectra(psdc_cross *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat,
                             float *sxx, float *syy, float *sxy);
/* PsdCascade::psd (src/psd.rs:479-543) of the four rows: sxx, syy `cap` floats, sxy 2 cap floats (re, im) */
int psdc_cross_csd(psdc_cross *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band,
                   float *sxx, float *syy, float *sxy, size_t cap, size_t *len,
                   psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* the stitch of psdc_cross_csd on caller-provided rows (n_stages x 4 x (n/2+1): xx, yy, re, im; stage 0 first):
 * psdc_stitch_window (src/psd.rs:479-543) on each row.  Pure host code. */
int psdc_cross_stitch(uint32_t n, float power, float nenbw, size_t overlap, uint32_t n_stages,
                      const uint64_t *counts64, const uint32_t *avgs, const uint64_t *pendings,
                      const float *rows, int keep_overlap,
                      uint32_t min_count, int keep_transition_band, float *sxx, float *syy, float *sxy,
                      size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and sample pairs accepted since creation or the last reset of the statistics */
int psdc_cross_stats_read(psdc_cross *h, uint64_t *launches, uint64_t *pairs_in, int reset);
/* last error text of an object; with h == NULL, of the calling thread's last failed cross call */
const char *psdc_cross_last_error(const psdc_cross *h);

/* ---- stream frames into a cross object ------------------------------------------------------------------
 * Frames in, cross spectra out: the frames of psdc_process_frames (any of the four formats, in runs) feed pairs of their
 * traces.  Pair p takes x = trace pair_traces[2p] and y = trace pair_traces[2p + 1] of every frame, in Payload::traces order:
 * AdcDac ADC0 ADC1 DAC0 DAC1, Fls AR AP BI BQ, ThermostatEem T00 T20 I0 I1, Mpll phase frequency amplitude.  The map has
 * 2 n_pairs entries; a pair whose two entries are PSDC_TRACE_NONE is not fed by the call.  A trace may feed several pairs and
 * x == y is allowed.  The map belongs to the call and is not stored.  Example: the map {2, 0} (pair 0 = (DAC0, ADC0)) of AdcDac
 * frames makes transfer() = H1 from DAC0 to ADC0 and coherence() that of the two.
 * Frames: headers, runs of one format, de::Error codes and *n_ok work exactly as in psdc_process_frames: on a bad frame the
 * frames before it are ingested, *n_ok says how many, and the frame's PSDC_ERR_FRAME_HEADER / _FORMAT / _SIZE is returned.
 * Header-only frames (0 batches) count in Loss only.  The decoded traces are bit-identical to Payload::traces.
 * Map errors: PSDC_ERR_ARG without ingesting anything for a NULL map, an entry with exactly one PSDC_TRACE_NONE, or a trace
 * index >= 4.  A run whose format carries fewer traces than the map names (Mpll has 3) is PSDC_ERR_ARG at the run's first
 * frame: the frames before it are ingested and *n_ok counts them.
 * Loss: one psdc_loss per object over every frame either call ingested (src/loss.rs:11-26); a reset zeroes it.
 * Rounds: a call is cut into pieces of whole frames of at most 2^22 samples a trace, in runs of one format; each piece is decoded
 * on the device (one launch per 16 fed pairs) into the stage-0 streams of its pairs and followed by one round, as a sample
 * call is.  The cut depends on the frames alone and is the same for both calls: the same calls give the same bits, and frames
 * in host memory the same bits as the same frames in device memory.
 * Memory: the first host-memory call allocates a 32 MB device buffer the frames go up through (in the object's pinned
 * staging); the device call keeps 8 bytes of pinned memory a frame of its largest call (at least 64 KB) and a third stream. */
#define PSDC_TRACE_NONE 0xFFFFFFFFu
/* frames in host memory */
int psdc_csd_process_frames(psdc_cross *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size,
                            size_t n_frames, size_t *n_ok);
/* frames in device memory.  The headers are gathered by one small launch on a side stream of the object and validated on the
 * host; the call waits for that launch alone, so *n_ok and the de::Error are final when it returns.  producer_event: a
 * hipEvent_t recorded behind the producer of d_frames, or NULL when the producer has completed; the gather and the decode wait
 * for it on the device.  Header bytes may be rewritten once the call has returned; payload bytes must stay unchanged until
 * the object's sync or a read-out returns.  Any base address is accepted. */
int psdc_csd_process_frames_device(psdc_cross *h, const uint32_t *pair_traces, const uint8_t *d_frames,
                                   size_t frame_size, size_t n_frames, size_t *n_ok, void *producer_event);
/* the Loss counters of the frames the object ingested (psdc_loss_read); reset != 0 zeroes them after reading */
int psdc_csd_loss_read(psdc_cross *h, psdc_loss *out, int reset);

/* ---- cross-spectral matrix cascade -------------------------------------------------------------------------
 * The full spectral matrix of a group of channels from ONE transform per channel: `n_groups` independent groups of `m`
 * real f32 streams (2 <= m <= 4, fixed per object), the channels of a group always fed together with equal lengths.
 * Per stage a group is m Psd<N> stages in lockstep exactly as a pair is two (see the cross-spectral density cascade
 * above): the same segmentation, Window<N>, Detrend of each channel's segment separately, /8 half-band decimation of
 * each channel with the drain of 35 outputs, lazy stages, EWMA factor g of src/psd.rs:218-233, 64-bit counts.  A group
 * has exactly the stages, counts, pendings and Breaks of a PsdCascade fed channel 0 alone.  Per bin k <= N/2 a stage
 * keeps the Hermitian matrix
 *     S_ab[k] = g S_ab[k] + conj(X_a[k]) X_b[k],   0 <= a <= b < m
 * with the pair object's sign convention (conj(X) Y, scipy.signal.csd).
 * Row layout: m*m real rows of n/2 + 1 values, f64 on the device: row a*m + a is S_aa; for a < b, row a*m + b is
 * Re S_ab and row b*m + a is Im S_ab.  For m = 2 these are the pair object's rows in the order xx, re, im, yy.
 * The read-out is PsdCascade::psd (src/psd.rs:479-543) applied to each real row with the same bins, Breaks and
 * 1 / (gain() decimation), as psdc_cross_csd does for its four rows.
 * Each channel of a group is loaded, detrended, windowed, transformed and decimated once per segment and stage and has
 * one stream buffer set per stage: six pairs of four traces cost four transforms and four decimations a segment, not
 * twelve.
 * Sizes: n a power of two 64 ... 2048 for every m, and 4096 for m = 2 and m = 3 (psdc_csm_supported).  n = 4096 with
 * m = 4 is refused: its 144 accumulators a thread do not fit the registers beside the transform.  A refused size is
 * PSDC_ERR_ARG with a text that names it (psdc_csm_last_error(NULL)).  Windows as for pairs.
 * Stream ordering, the caller-keeps-memory rule, errors and the device rule are those of psdc_cross_*: status codes, a
 * text per object, with a NULL object the calling thread's last failure; every call restores the caller's current
 * device; there is no CPU fallback.
 * Rounds: a process call is one round of three kernel launches (the segments of every (group, stage), the decimators, the
 * fold + stream tails) whatever the depth and whatever m, as long as the round's job tables fit one launch each: 128
 * (group, stage) segment jobs and 128 folds; 320 decimator jobs and 256 tail carries, m a (group, stage): 80 and 64
 * (group, stage) at m = 4, 106 and 85 at m = 3, 160 and 128 at m = 2.  A round with more takes one more launch of a
 * kind per table it overflows.  Read-outs run rounds until no stage has work.
 * Determinism: workgroup partial rows are folded in f64 in a fixed order: the same calls give the same bits, and frames
 * in host memory the same bits as the same frames in device memory.
 * Memory: per (group, stage) two ping-pong buffers per channel as for pairs (m channels, not 2 per pair), plus 32 MB of
 * pinned host staging per channel and object (2 x m x 16 MB). */
typedef struct psdc_csm psdc_csm;
/* 1 if an object of (n, m) can be created, else 0.  Pure host code. */
int psdc_csm_supported(uint32_t n, uint32_t m);
/* n_groups groups of m channels; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_csm *psdc_csm_create(uint32_t n, int window_kind, uint32_t m, uint32_t n_groups, int device);
/* the same with a caller-built Window<N>, as psdc_cross_create_window */
psdc_csm *psdc_csm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t m,
                                 uint32_t n_groups, int device);
void psdc_csm_destroy(psdc_csm *h);
int psdc_csm_reset(psdc_csm *h);
/* Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere */
int psdc_csm_set_detrend(psdc_csm *h, int detrend_kind);
int psdc_csm_set_avg(psdc_csm *h, uint32_t limit, uint32_t count);
/* x: m pointers to len samples each, host memory */
int psdc_csm_process(psdc_csm *h, uint32_t group, const float *const *x, size_t len);
/* d_x: m device pointers (the array itself is host memory); producer_event and the caller-keeps-memory rule as
 * psdc_cross_process_device */
int psdc_csm_process_device(psdc_csm *h, uint32_t group, const float *const *d_x, size_t len, void *producer_event);
/* Stream frames into groups: the map has m * n_groups entries; channel c of group g takes trace group_traces[g*m + c]
 * of every frame.  A group whose entries are all PSDC_TRACE_NONE is not fed; a group with some but not all
 * PSDC_TRACE_NONE is PSDC_ERR_ARG before anything is ingested.  Headers, runs of one format, de::Error codes, *n_ok,
 * header-only frames, the too-few-traces rule (PSDC_ERR_ARG at the run's first frame) and the cut into pieces of at
 * most 2^22 samples a trace are those of psdc_csd_process_frames.  A cell is decoded once and stored once per group
 * (one launch per 32 / m fed groups). */
int psdc_csm_process_frames(psdc_csm *h, const uint32_t *group_traces, const uint8_t *frames, size_t frame_size,
                            size_t n_frames, size_t *n_ok);
int psdc_csm_process_frames_device(psdc_csm *h, const uint32_t *group_traces, const uint8_t *d_frames,
                                   size_t frame_size, size_t n_frames, size_t *n_ok, void *producer_event);
int psdc_csm_loss_read(psdc_csm *h, psdc_loss *out, int reset);
int psdc_csm_sync(psdc_csm *h);
int psdc_csm_num_stages(psdc_csm *h, uint32_t group);
/* raw accumulators of one stage: rows m*m*(n/2+1) floats in the row layout above; stat and rows may be NULL */
int psdc_csm_stage_spectra(psdc_csm *h, uint32_t group, uint32_t stage, psdc_stage_stat *stat, float *rows);
/* PsdCascade::psd of every row: rows holds m*m rows of `cap` floats each, the first *len of each filled */
int psdc_csm_csd(psdc_csm *h, uint32_t group, int keep_overlap, uint32_t min_count, int keep_transition_band,
                 float *rows, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* the stitch of psdc_csm_csd on caller-provided stages (rows_in: n_stages x m*m x (n/2+1), stage 0 first):
 * psdc_stitch_window on each of the m*m rows, into rows (m*m rows of cap floats).  Pure host code. */
int psdc_csm_stitch(uint32_t n, uint32_t m, float power, float nenbw, size_t overlap, uint32_t n_stages,
                    const uint64_t *counts64, const uint32_t *avgs, const uint64_t *pendings, const float *rows_in,
                    int keep_overlap, uint32_t min_count, int keep_transition_band, float *rows, size_t cap,
                    size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and sample times accepted (one sample time = one sample of every channel of a group) */
int psdc_csm_stats_read(psdc_csm *h, uint64_t *launches, uint64_t *sample_times_in, int reset);
const char *psdc_csm_last_error(const psdc_csm *h);

/* ---- zoom cascade: log-resolution spectrum around a carrier --------------------------------------------------
 * The cascade resolves 1 / (N 8^k) at stage k, but only towards frequency 0.  A zoom object puts an NCO mixer in front of
 * the same cascade, as a phase-noise analyser does: `n_channels` independent real f32 streams, each with its own carrier,
 * each mixed to a complex baseband pair (I, Q) whose two-sided spectrum is kept.
 * Carrier: a 64-bit frequency tuning word `ftw` and a start phase `phase0`, both uint64_t in units of 2^-64 turn.  Sample
 * j of the channel's stream, counted from create or reset in 64 bits, has the phase phi_j = phase0 + ftw j mod 2^64, exact
 * in integer arithmetic however the stream is cut into calls; f0 = ftw / 2^64 cycles per sample.  The default is ftw = 0,
 * phase0 = 0.  A carrier may be set only while the channel has taken no sample since create or reset (a reset also puts
 * every carrier back to the default); otherwise PSDC_ERR_ARG with a text.
 * Mixing: z_j = x_j exp(-2 pi i phi_j / 2^64), so I_j = x_j c and Q_j = -x_j s in f32 with (c, s) the f32 cosine and sine of
 * the top 32 bits of phi_j: an exact integer octant reduction, then polynomials of explicit fused multiply-adds (csrc/zoom_lo.h,
 * absolute error <= 2^-23, the same bits on host and device).  Quarter turns give exactly (+-1, 0) and (0, +-1).
 * Stages: per stage (I, Q) are two Psd<N> stages (src/psd.rs:195-269) in lockstep exactly as a pair's two channels are (see
 * the cross-spectral density cascade above): the same segmentation, Window<N>, Detrend applied to I and Q separately, /8
 * half-band decimation of each with the drain of 35 outputs, lazy stages, the EWMA factor g of src/psd.rs:218-233 and
 * 64-bit counts.  Mixing happens once, in front of stage 0.  A channel has exactly the stages, counts, pendings and Breaks of
 * a PsdCascade fed x.
 * Rows: each segment is ONE N-point complex transform Z of I + i Q.  A stage keeps two f64 rows of n/2 + 1 bins,
 *     upper[k] = g upper[k] + |Z[k]|^2,   lower[k] = g lower[k] + |Z[(N - k) mod N]|^2,   k = 0 ... N/2
 * (bins 0 and N/2 appear in both).  Nothing is subtracted anywhere: a single sideband does not leak into its image beyond
 * the transform's own rounding, which the sums Sii + Sqq -+ 2 Im Siq of a pair object fed (I, Q) cannot offer.
 * Read-out: PsdCascade::psd (src/psd.rs:479-543) applied to each row with the same bins, Breaks and 1 / (gain() decimation).
 * With that unchanged gain `upper` at offset f is the reference's one-sided PSD of x at f0 + f and `lower` that at f0 - f (a
 * real x has a two-sided density of half its one-sided one, and the factor N/2 of the cascade's gain restores it): white noise
 * of variance 1 reads 2 in every bin of both rows.
 * Sizes and windows are those of pairs: n a power of two 64 ... 4096; Window::hann(), Window::rectangular(), or a caller's
 * table with (n - overlap) % 8 == 0.  Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere.  There is no CPU fallback.
 * Stream ordering, the caller-keeps-memory rule, errors and the device rule are those of the pair object.  The mixer takes
 * the place of the pair object's input copy, on the same side stream under the same events, so it overlaps the round before;
 * host samples go up through the pinned staging into a 16 MB device landing buffer first (made by the first host call).  A
 * steady-state call is 1 + 3 kernel launches (mixer; segments, decimators, fold + tails) whatever the depth, with the pair
 * object's table limits.  Host and device calls of the same samples, and the same calls twice, give the same bits.
 * A bank's channel equals a single object fed the same calls bit for bit only when its rounds are that object's: each
 * channel fed and read out in turn.  A round plans every channel with work, so interleaved calls put a channel's decimated
 * stages into other channels' rounds, cut a round's segments elsewhere and reorder f32 partial sums: the same spectra
 * within 2e-6, as for the pairs of a pair object.
 * Memory: per (channel, stage) two ping-pong buffers for each of I and Q as for a pair, plus 32 MB of pinned staging. */
typedef struct psdc_zoom psdc_zoom;
/* n_channels channels; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_zoom *psdc_zoom_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
/* the same with a caller-built Window<N> (src/psd.rs:12-20), as psdc_create_window */
psdc_zoom *psdc_zoom_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap,
                                   uint32_t n_channels, int device);
void psdc_zoom_destroy(psdc_zoom *h);
/* back to the state of a fresh object: stages, buffers, settings, carriers and statistics */
int psdc_zoom_reset(psdc_zoom *h);
int psdc_zoom_set_detrend(psdc_zoom *h, int detrend_kind);
int psdc_zoom_set_avg(psdc_zoom *h, uint32_t limit, uint32_t count);
/* the channel's carrier (see Carrier above); PSDC_ERR_ARG once the channel has taken a sample */
int psdc_zoom_set_carrier(psdc_zoom *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* len real samples of a channel from host memory */
int psdc_zoom_process(psdc_zoom *h, uint32_t channel, const float *x, size_t len);
/* the same from device memory (any 4-byte aligned address and any length); producer_event: hipEvent_t or NULL */
int psdc_zoom_process_device(psdc_zoom *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
/* Stream frames into zoom channels (mirrors psdc_csd_process_frames).  The three frames calls of a psdc_zoom object carry the
 * prefix psdc_zoomcascade_, after ZoomCascade, the object's name in the mirrors, as a psdc_cross object's carry psdc_csd_
 * after CsdCascade: the psdc_zoom_ set is the sample-fed object's and stays as it was.  The map has n_channels entries; channel c takes trace
 * channel_traces[c] of every frame, in Payload::traces order (see "stream frames into a cross object").  PSDC_TRACE_NONE: the
 * channel is not fed by this call and its stream index does not move.  A trace may feed any number of channels (a carrier
 * and its harmonics on one input).  The map belongs to the call and is not stored.
 * Map errors: PSDC_ERR_ARG without ingesting anything for a NULL map, a trace index >= 4 or a map that feeds no channel.  A
 * run whose format carries fewer traces than the map names is PSDC_ERR_ARG at the run's first frame: the frames before it
 * are ingested and *n_ok counts them.
 * Frames: headers, runs of one format, de::Error codes, *n_ok, header-only frames (Loss only) and Loss are those of
 * psdc_csd_process_frames, from the same scanner.  A call is cut into pieces of whole frames of at most 2^22 samples a trace,
 * in runs of one format, as the pair object's is; each piece is ONE decode-and-mix launch per 16 fed channels
 * (zoom_frames_kernel: a cell is read and converted once, mixed in registers with every channel's carrier that takes it and
 * stored to the channel's I and Q streams; the f32 trace never exists in memory) and then one round.  The launch stands
 * where the mixer of psdc_zoom_process_device stands: on the side stream, behind a grown buffer and round R - 2, in front of
 * round R.  Host frames go up through the pinned staging into a 16 MB device landing buffer (a zoom object's staging slots
 * are 16 MB, half the pair object's: made by the first host-frames call), one decode-and-mix launch a slot.
 * Carrier rule: unchanged -- psdc_zoom_set_carrier is PSDC_ERR_ARG once the channel has taken a sample, by either route.
 * samples_in of psdc_zoom_stats_read counts the samples accepted over all fed channels.  A reset zeroes Loss.
 * Invariants:
 *  (a) a call that is one piece gives the same bits as psdc_zoom_process fed Payload::traces of the same frames in one call
 *      (the decode is bit-identical to Payload::traces, a sample's phase comes from its 64-bit stream index, and the round
 *      is the same);
 *  (b) the same frames in host and in device memory give the same bits (the cut depends on the headers alone);
 *  (c) sample and frame calls may be mixed on one channel: the stream index, and so the phase, continues across them;
 *  (d) a steady-state call of one piece that feeds up to 16 channels is 1 + 3 kernel launches on the side and compute
 *      streams (decode-and-mix; segments, decimators, fold + tails), for host frames that fit one staging slot.  The device
 *      call's header gather on its own stream is one more launch and psdc_zoom_stats_read counts it, as the pair object's
 *      statistics do: such a device call reads 5. */
int psdc_zoomcascade_process_frames(psdc_zoom *h, const uint32_t *channel_traces, const uint8_t *frames, size_t frame_size,
                             size_t n_frames, size_t *n_ok);
/* the same for frames in device memory (mirrors psdc_csd_process_frames_device): the side-stream header gather, the host
 * wait for that launch alone, producer_event, the keep-unchanged rule and "any base address" are that call's */
int psdc_zoomcascade_process_frames_device(psdc_zoom *h, const uint32_t *channel_traces, const uint8_t *d_frames,
                                    size_t frame_size, size_t n_frames, size_t *n_ok, void *producer_event);
/* the Loss counters of the frames the object ingested (mirrors psdc_csd_loss_read); reset != 0 zeroes them after reading */
int psdc_zoomcascade_loss_read(psdc_zoom *h, psdc_loss *out, int reset);
int psdc_zoom_sync(psdc_zoom *h);
int psdc_zoom_num_stages(psdc_zoom *h, uint32_t channel);
/* raw accumulators of one stage: upper, lower n/2 + 1 floats each; any may be NULL */
int psdc_zoom_stage_spectra(psdc_zoom *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, float *upper,
                            float *lower);
/* PsdCascade::psd (src/psd.rs:479-543) of both rows: upper, lower `cap` floats each (either may be NULL) */
int psdc_zoom_psd(psdc_zoom *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  float *upper, float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap,
                  size_t *n_breaks);
/* kernel launches issued and samples accepted since creation or the last reset of the statistics */
int psdc_zoom_stats_read(psdc_zoom *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_zoom_last_error(const psdc_zoom *h);

/* ---- zoom cross cascade: two streams around a carrier ------------------------------------------------------------
 * The cross spectrum of two receivers that watch the same carrier, at the cascade's log resolution: their own noise is
 * uncorrelated and averages out of S_ab; what stays is the source's noise at f0 +- f.  A zoom cross object holds `n_pairs`
 * independent pairs.  A pair is two real f32 streams a and b, always fed together with equal lengths.  Each of the two has
 * its own carrier, a tuning word and start phase exactly as psdc_zoom_set_carrier's (2^-64 turn, the phase of sample j
 * from its 64-bit stream index in integers, however the stream is cut into calls); both default to ftw = 0, phase0 = 0.  A
 * carrier may be set only while the pair has taken no sample since create or reset; a reset puts both back to the default.
 * Stages: every one of the four streams (I_a, Q_a, I_b, Q_b) the two mixers make is a Psd<N> stage in lockstep with the
 * others, exactly as a zoom channel's two are: segmentation, Window<N>, Detrend of each separately, /8 half-band decimation
 * of each (four decimator jobs a (pair, stage)) with the drain of 35 outputs, lazy stages, EWMA factor g, 64-bit counts.  A
 * pair has exactly the stages, counts, pendings and Breaks of a PsdCascade (or a psdc_zoom channel) fed a.
 * Rows: per segment Z_a and Z_b are the N-point complex transforms of the detrended, windowed I + i Q of the SAME segment of
 * the two channels.  A stage keeps eight f64 rows of n/2 + 1 bins, k = 0 ... N/2, each accumulated as row = g row + value:
 *     value                 row `upper`: bin k      row `lower`: bin (N - k) mod N
 *     S_aa = |Z_a|^2             0                       1
 *     S_bb = |Z_b|^2             2                       3
 *     Re S_ab                    4                       5
 *     Im S_ab                    6                       7
 * Sign: S_ab[j] = conj(Z_a[j]) Z_b[j], that of the pair object (conj(X) Y, scipy.signal.csd): the transfer function from a to
 * b is S_ab / S_aa, the coherence |S_ab|^2 / (S_aa S_bb).  lower[k] is the value AT bin N - k, not conjugated: the spectrum
 * at f0 - f, as `upper` is that at f0 + f (bins 0 and N/2 appear in both).  The products are formed per bin from the two
 * transforms' registers; nothing is separated and nothing is subtracted across bins or rows, so a single sideband leaks into
 * its image by the transform's own rounding only (a matrix object fed the four mixed streams rebuilds these rows from sums
 * and differences of sixteen rows f32 has already rounded).
 * Rows 0 ... 3 are the rows of two psdc_zoom channels fed a and b with the same carriers (within the chunking bound below:
 * the partial sums are ordered differently).  With ftw = 0 on both sides Q is 0 and S_ab upper is psdc_cross_csd's Sxy of (a, b).
 * Recipe, AM / PM separation: feed the SAME stream to both sides with the carriers ftw and -ftw (phase0 = 0).  Then Z_b[k] =
 * conj(Z_a[-k]) for a real input, S_bb upper is S_aa lower, and S_ab upper = conj(Z_a[k] Z_a[-k]): the term whose real part
 * (relative to the carrier's own phase) separates amplitude from phase noise.  No helper is built on it.
 * Read-out: PsdCascade::psd (src/psd.rs:479-543) applied to each of the eight real rows with the same bins, Breaks and
 * 1 / (gain() decimation), as psdc_zoom_psd does for its two: the auto rows read as psdc_zoom_psd's.
 * Sizes: n a power of two 64 ... 4096 (psdc_zcsd_supported; every size builds without scratch memory); a refused size is
 * PSDC_ERR_ARG with a text that names n.  Windows as for pairs.  Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere.
 * Stream ordering, the caller-keeps-memory rule, errors, the device rule, determinism and the bank rule (a pair equals a
 * single object bit for bit when fed and read out in turn, within 2e-6 interleaved or when the stream is cut into other calls)
 * are those of psdc_zoom_*.  The two mixers stand where the zoom object's one stands; host samples go up through the pinned
 * staging into a 32 MB device landing buffer.  A steady-state call on one pair is 2 + 3 kernel launches whatever the depth
 * (PSDC_ZCSD_STEADY_LAUNCHES: two mixers; segments, decimators, fold + tails), with the matrix object's table limits at
 * m = 4.  Host and device calls of the same samples run the same launches on the same data and give the same bits.
 * Memory: per (pair, stage) two ping-pong buffers for each of the four streams, plus 64 MB of pinned staging.
 * Stream frames feed this object through the three psdc_zoomcsdcascade_ calls below ("Stream frames into zoom cross pairs"). */
#define PSDC_ZCSD_STEADY_LAUNCHES 5
typedef struct psdc_zcsd psdc_zcsd;
/* 1 if an object of size n can be created, else 0.  Pure host code. */
int psdc_zcsd_supported(uint32_t n);
/* n_pairs pairs; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_zcsd *psdc_zcsd_create(uint32_t n, int window_kind, uint32_t n_pairs, int device);
/* the same with a caller-built Window<N> (src/psd.rs:12-20), as psdc_create_window */
psdc_zcsd *psdc_zcsd_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap,
                                   uint32_t n_pairs, int device);
void psdc_zcsd_destroy(psdc_zcsd *h);
/* back to the state of a fresh object: stages, buffers, settings, carriers and statistics */
int psdc_zcsd_reset(psdc_zcsd *h);
int psdc_zcsd_set_detrend(psdc_zcsd *h, int detrend_kind);
int psdc_zcsd_set_avg(psdc_zcsd *h, uint32_t limit, uint32_t count);
/* the carrier of one side of a pair (side 0: channel a, 1: channel b); PSDC_ERR_ARG once the pair has taken a sample */
int psdc_zcsd_set_carrier(psdc_zcsd *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0);
/* len real samples of each channel from host memory */
int psdc_zcsd_process(psdc_zcsd *h, uint32_t pair, const float *x, const float *y, size_t len);
/* the same from device memory (any 4-byte aligned addresses and any length); producer_event: hipEvent_t or NULL */
int psdc_zcsd_process_device(psdc_zcsd *h, uint32_t pair, const float *d_x, const float *d_y, size_t len,
                             void *producer_event);
/* Stream frames into zoom cross pairs (mirrors psdc_csd_process_frames).  The three frames calls of a psdc_zcsd object carry the
 * prefix psdc_zoomcsdcascade_, after ZoomCsdCascade, the object's name in the mirrors, as a psdc_zoom object's carry
 * psdc_zoomcascade_ after ZoomCascade: the psdc_zcsd_ set is the sample-fed object's and stays as it was.  The map is
 * psdc_csd_process_frames's, 2 * n_pairs entries: pair p takes a = trace pair_traces[2p] and b = trace pair_traces[2p + 1] of every
 * frame, in Payload::traces order (see "stream frames into a cross object").  Both entries PSDC_TRACE_NONE: the pair is not fed
 * by this call and its stream index does not move.  A trace may feed any number of sides; a == b is allowed (the AM / PM
 * recipe above: one trace, carriers +-ftw).  The map belongs to the call and is not stored.
 * Map errors: PSDC_ERR_ARG without ingesting anything, *n_ok = 0, for a NULL map, a pair with exactly one PSDC_TRACE_NONE, a
 * trace index >= 4 or a map that feeds no pair (the zoom kind's rule, not the pair object's: a call for Loss alone is refused).
 * A run whose format carries fewer traces than the map names is PSDC_ERR_ARG at the run's first frame, with a text that names
 * the trace: the frames before it are ingested and *n_ok counts them.
 * Frames: headers, runs of one format, de::Error codes, *n_ok, header-only frames (Loss only) and Loss are those of
 * psdc_csd_process_frames, from the same scanner; one psdc_loss an object, zeroed by psdc_zcsd_reset.  A call is cut into pieces
 * of whole frames of at most 2^22 samples a trace, in runs of one format, and the cut depends on the headers alone; each piece
 * is ONE decode-and-mix launch per 8 fed pairs (zoom_cross_frames_kernel: a cell is read and converted once, handed to every
 * side of every pair that takes it, mixed in registers with the side's carrier and stored to the side's I and Q streams; the
 * f32 trace never exists in memory) and then one round.  Where both sides of a pair have the same ftw and the same phase0 --
 * two receivers on one carrier -- the oscillator is evaluated once a sample for both, with the bits of two evaluations (I = x c
 * and Q = -(x s) are formed separately from the same (c, s)); equal ftw with different phase0, and the +-ftw recipe, are two
 * oscillators.  The launch stands where the two mixers of psdc_zcsd_process_device stand: on the side stream, behind a grown
 * buffer and round R - 2, in front of round R.
 * Memory: host frames go up through the pinned staging into a 32 MB device buffer made by the first host-frames call -- one
 * staging slot of this object, twice the zoom object's 16 MB --, one decode-and-mix launch (per 8 fed pairs) a slot.
 * Carrier rule: unchanged -- psdc_zcsd_set_carrier is PSDC_ERR_ARG once the pair has taken a sample, by either route; a pair
 * the map left out is still free.  pairs_in of psdc_zcsd_stats_read counts the sample pairs accepted over all fed pairs.
 * Invariants:
 *  (a) a call that is one piece gives the same bits as psdc_zcsd_process fed Payload::traces of the same frames in one call:
 *      all eight rows of every stage, the stats and psdc_zcsd_csd (the decode is bit-identical to Payload::traces, a sample's
 *      phase comes from its 64-bit stream index, and the round is the same);
 *  (b) the same frames in host and in device memory give the same bits (the cut depends on the headers alone);
 *  (c) sample and frame calls may be mixed on one pair: the 64-bit stream index, and so both phases, continues across them;
 *  (d) a steady-state call of one piece that feeds up to 8 pairs is 1 + 3 kernel launches on the side and compute streams
 *      (decode-and-mix; segments, decimators, fold + tails), for host frames that fit one staging slot, where the sample route
 *      needs 2 + 3 for ONE pair.  The device call's header gather on its own stream is one more launch and
 *      psdc_zcsd_stats_read counts it, as the pair object's statistics do: such a device call reads 5. */
int psdc_zoomcsdcascade_process_frames(psdc_zcsd *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size,
                                       size_t n_frames, size_t *n_ok);
/* the same for frames in device memory (mirrors psdc_csd_process_frames_device): the side-stream header gather, the host
 * wait for that launch alone, producer_event, the keep-payload-unchanged rule and "any base address" are that call's; header
 * bytes may be rewritten once the call has returned */
int psdc_zoomcsdcascade_process_frames_device(psdc_zcsd *h, const uint32_t *pair_traces, const uint8_t *d_frames,
                                              size_t frame_size, size_t n_frames, size_t *n_ok, void *producer_event);
/* the Loss counters of the frames the object ingested (mirrors psdc_csd_loss_read); reset != 0 zeroes them after reading */
int psdc_zoomcsdcascade_loss_read(psdc_zcsd *h, psdc_loss *out, int reset);
int psdc_zcsd_sync(psdc_zcsd *h);
int psdc_zcsd_num_stages(psdc_zcsd *h, uint32_t pair);
/* raw accumulators of one stage: rows 8 (n/2 + 1) floats in the row layout above; stat and rows may be NULL */
int psdc_zcsd_stage_spectra(psdc_zcsd *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, float *rows);
/* PsdCascade::psd of every row, with the arguments of psdc_zoom_psd: the auto rows `cap` floats each, sab_upper and sab_lower
 * 2 cap floats (re, im); any may be NULL */
int psdc_zcsd_csd(psdc_zcsd *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band,
                  float *saa_upper, float *saa_lower, float *sbb_upper, float *sbb_lower, float *sab_upper,
                  float *sab_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and sample pairs accepted since creation or the last reset of the statistics */
int psdc_zcsd_stats_read(psdc_zcsd *h, uint64_t *launches, uint64_t *pairs_in, int reset);
const char *psdc_zcsd_last_error(const psdc_zcsd *h);

/* ---- IQ cascade: complex baseband streams, with an optional retune ---------------------------------------------
 * The zoom objects take a REAL stream and mix it to I + i Q themselves.  An IQ object takes streams that are complex already:
 * the demodulated quadratures of an Fls payload (traces BI / BQ), the I/Q of a lock-in or SDR front end, a complex64 array.  It
 * holds `n_channels` independent complex f32 streams z_j = I_j + i Q_j and keeps the two-sided spectrum of each.
 * Carrier: every channel has one, a tuning word `ftw` and a start phase `phase0` (uint64_t, units of 2^-64 turn; default 0, 0),
 * under the zoom object's rules: sample j of the channel's stream, counted from create or reset in 64 bits, has the phase
 * phi_j = phase0 + ftw j mod 2^64, exact in integer arithmetic however the stream is cut into calls; a carrier may be set only
 * while the channel has taken no sample since create or reset (else PSDC_ERR_ARG with a text); a reset puts every carrier back
 * to the default.  With the default the object analyses z as it is; with a carrier it is a second-stage zoom: a coarse
 * down-conversion elsewhere, the fine retune and the log-resolution spectrum here.
 * Mixing: z'_j = z_j exp(-2 pi i phi_j / 2^64).  (c, s) are the f32 cosine and sine of the zoom object's oscillator
 * (csrc/zoom_lo.h, unchanged), and the f32 operations are fixed (csrc/iq_lo.h):
 *     I' = fmaf(Q, s,  I * c)
 *     Q' = fmaf(Q, c, -(I * s))
 * one stand-alone product and one explicit fused multiply-add each, the same bits on host and device.  Two consequences: with
 * Q = 0 these are exactly the zoom mixer's x c and -(x s) -- an IQ channel fed (x, 0) is the zoom channel fed x, bit for bit;
 * with ftw = phase0 = 0 they return (I, Q) unchanged for finite input (up to the sign of a zero).
 * Stages, rows, read-out: everything behind the mixer is the zoom object's, bit for bit (see "zoom cascade" above):
 * segmentation, Window<N>, Detrend applied to I' and Q' separately, /8 half-band decimation of each with the drain of 35
 * outputs, lazy stages, the EWMA factor g and 64-bit counts; each segment is ONE N-point complex transform Z of I' + i Q' and
 * a stage keeps the rows upper[k] = g upper[k] + |Z[k]|^2 and lower[k] = g lower[k] + |Z[(N - k) mod N]|^2, k = 0 ... N/2;
 * the read-out is PsdCascade::psd on each row with the unchanged gain.  A channel has exactly the stages, counts, pendings and
 * Breaks of a PsdCascade fed a real stream of the same length.
 * Scale: under the unchanged gain complex white noise with E|z|^2 = 1 reads 2 in every bin of both rows.  row / 2 is the
 * two-sided density of z: over the offsets (-0.5, 0.5] -- `lower` mirrored, then `upper` -- it integrates to E|z|^2.
 * Sizes and windows are those of the zoom object: n a power of two 64 ... 4096; Window::hann(), Window::rectangular(), or a
 * caller's table with (n - overlap) % 8 == 0.  Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere.  There is no CPU
 * fallback.
 * Sample routes: planar (two f32 streams, each 4-byte aligned) and interleaved ((re, im) pairs, 8-byte aligned: the memory of
 * a complex64 array), each from host or from device memory, any length.  The complex mixer stands where the zoom object's
 * mixer stands: on the side stream, behind a grown buffer and round R - 2, in front of round R; host samples go up through the
 * pinned staging into a 32 MB device landing buffer first (made by the first host call), so host and device calls run the
 * same launches.  A steady-state call is 1 + 3 kernel launches (mixer; segments, decimators, fold + tails) whatever the depth.
 * All four sample routes and the frames route may be mixed on one channel: the stream index, and so the phase, continues
 * across them, and the same calls give the same bits by every route.  Stream ordering, the caller-keeps-memory rule, errors,
 * the device rule and what holds for a bank's channels against single objects are those of the zoom object.
 * Memory: per (channel, stage) two ping-pong buffers for each of I and Q, plus 64 MB of pinned staging. */
typedef struct psdc_iq psdc_iq;
/* n_channels complex channels; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_iq *psdc_iq_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
/* the same with a caller-built Window<N> (src/psd.rs:12-20), as psdc_create_window */
psdc_iq *psdc_iq_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                               int device);
void psdc_iq_destroy(psdc_iq *h);
/* back to the state of a fresh object: stages, buffers, settings, carriers and statistics */
int psdc_iq_reset(psdc_iq *h);
int psdc_iq_set_detrend(psdc_iq *h, int detrend_kind);
int psdc_iq_set_avg(psdc_iq *h, uint32_t limit, uint32_t count);
/* the channel's carrier (see Carrier above); PSDC_ERR_ARG once the channel has taken a sample */
int psdc_iq_set_carrier(psdc_iq *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* len complex samples of a channel from host memory, planar: i[j] + i q[j] */
int psdc_iq_process(psdc_iq *h, uint32_t channel, const float *i, const float *q, size_t len);
/* the same from device memory (any 4-byte aligned addresses and any length); producer_event: hipEvent_t or NULL */
int psdc_iq_process_device(psdc_iq *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event);
/* len complex samples as (re, im) pairs, 2 len floats, 8-byte aligned, from host memory */
int psdc_iq_process_interleaved(psdc_iq *h, uint32_t channel, const float *iq, size_t len);
/* the same from device memory */
int psdc_iq_process_interleaved_device(psdc_iq *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event);
/* Stream frames into IQ channels (mirrors psdc_csd_process_frames).  The map has 2 n_channels entries: channel c takes trace
 * channel_traces[2 c] of every frame as I and trace channel_traces[2 c + 1] as Q, in Payload::traces order (Fls: BI = 2,
 * BQ = 3).  PSDC_TRACE_NONE in both entries: the channel is not fed by this call and its stream index does not move; in only one
 * of them it is PSDC_ERR_ARG.  A trace may feed any number of channels and both sides of one.  The map belongs to the call.
 * Map errors: PSDC_ERR_ARG without ingesting anything for a NULL map, a trace index >= 4, a channel with one PSDC_TRACE_NONE
 * or a map that feeds no channel.  A run whose format carries fewer traces than the map names is PSDC_ERR_ARG at the run's
 * first frame: the frames before it are ingested and *n_ok counts them.
 * Frames: headers, runs of one format, de::Error codes, *n_ok, header-only frames (Loss only), the cut into pieces of whole
 * frames of at most 2^22 samples a trace and Loss committed piece by piece are those of psdc_csd_process_frames, from the same
 * scanner.  Each piece is ONE decode-and-mix launch per 16 fed channels (iq_frames_kernel: a cell is read and converted once,
 * the two samples of every channel it feeds are mixed in registers and stored to the channel's I and Q streams; the f32
 * traces never exist in memory) and then one round.  A one-piece call gives the same bits as the planar sample call fed
 * Payload::traces of the same frames; host and device frames give the same bits; a steady-state one-piece call is 1 + 3
 * launches, and the device call's header gather is a fifth that psdc_iq_stats_read counts. */
int psdc_iq_process_frames(psdc_iq *h, const uint32_t *channel_traces, const uint8_t *frames, size_t frame_size, size_t n_frames,
                           size_t *n_ok);
int psdc_iq_process_frames_device(psdc_iq *h, const uint32_t *channel_traces, const uint8_t *d_frames, size_t frame_size,
                                  size_t n_frames, size_t *n_ok, void *producer_event);
/* the Loss counters of the frames the object ingested; reset != 0 zeroes them after reading */
int psdc_iq_loss_read(psdc_iq *h, psdc_loss *out, int reset);
int psdc_iq_sync(psdc_iq *h);
int psdc_iq_num_stages(psdc_iq *h, uint32_t channel);
/* raw accumulators of one stage: upper, lower n/2 + 1 floats each; any may be NULL */
int psdc_iq_stage_spectra(psdc_iq *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, float *upper, float *lower);
/* PsdCascade::psd (src/psd.rs:479-543) of both rows: upper, lower `cap` floats each (either may be NULL) */
int psdc_iq_psd(psdc_iq *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and complex samples accepted since creation or the last reset of the statistics */
int psdc_iq_stats_read(psdc_iq *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_iq_last_error(const psdc_iq *h);

/* ---- IQ cross cascade: two complex baseband streams, one transform each ------------------------------------------
 * The cross spectrum of two streams that are complex already: two lock-ins or two SDR front ends on one source (their own
 * noise averages out of S_ab, the source's stays), a second-stage zoom on both outputs of a coarse down-conversion done
 * elsewhere, or -- by the zoom cross section's +-ftw recipe with the SAME complex stream on both sides -- the AM / PM
 * separation of a stream that arrives as I/Q.  An IQ cross object holds `n_pairs` independent pairs.  A pair is two complex
 * f32 streams a = I_a + i Q_a and b = I_b + i Q_b, always fed together with equal lengths.
 * Carrier: each side has one, a tuning word and start phase under the zoom cross object's rule (psdc_zcsd_set_carrier): units
 * of 2^-64 turn, default 0, 0; sample j of the pair's stream, counted from create or reset in 64 bits, has the phase
 * phase0 + ftw j mod 2^64 of its side, exact in integers however the stream is cut into calls and by whichever route it came;
 * a carrier may be set only while the pair has taken no sample, by any route, since create or reset (else PSDC_ERR_ARG); a
 * reset puts both back to the default.
 * Mixing: each side is turned by csrc/iq_lo.h's fixed formula, unchanged: I' = fmaf(Q, s, I * c), Q' = fmaf(Q, c, -(I * s))
 * with the (c, s) of csrc/zoom_lo.h at the side's phase.  Where both sides have the same ftw AND the same phase0 the
 * oscillator is evaluated once a sample and used for both, with the bits of two evaluations; equal ftw with different phase0,
 * and the +-ftw recipe, are two oscillators.  With Q_a = Q_b = 0 the four mixed streams are the zoom cross object's of (I_a,
 * I_b), bit for bit (up to the sign of a zero).
 * Everything behind the mixer is the zoom cross object's, bit for bit (see "zoom cross cascade" above): the four streams in
 * lockstep, segmentation, Window<N>, Detrend of each separately, the /8 decimators with the drain of 35 outputs, lazy stages,
 * the EWMA factor g and 64-bit counts; ONE N-point complex transform a side and segment; the eight f64 rows S_aa, S_bb,
 * Re S_ab, Im S_ab, `upper` and `lower` of each, in that section's layout; the sign S_ab = conj(Z_a) Z_b; lower[k] the value AT
 * bin N - k, not conjugated; the read-out PsdCascade::psd on each row with the unchanged gain; the sizes 64 ... 4096
 * (psdc_iqcsd_supported equals psdc_zcsd_supported); the windows; Detrend::Linear PSDC_ERR_UNIMPLEMENTED.  There is no CPU
 * fallback.  Rows 0 ... 3 are the rows of two psdc_iq channels fed the sides with the same carriers (within the chunking bound:
 * the partial sums are ordered differently).
 * Sample routes: planar (four f32 streams I_a, Q_a, I_b, Q_b, each 4-byte aligned) and interleaved (the (re, im) pairs of each
 * side, 8-byte aligned: two complex64 arrays), each from host or from device memory, any length; the contracts are those of the
 * psdc_iq_process calls, per side.  ONE pair mixer launch (iq_pair_mix_kernel) turns both sides, where the zoom cross object
 * runs a mixer a side: on the side stream, behind a grown buffer and round R - 2, in front of round R.  Host samples go up
 * through the pinned staging into a 64 MB device landing buffer first (four streams of 2^22 samples, made by the first host
 * call), so host and device calls run the same launches.  A steady-state call on one pair is 1 + 3 kernel launches whatever
 * the depth (PSDC_IQCSD_STEADY_LAUNCHES: pair mixer; segments, decimators, fold + tails).
 * All four sample routes and the frames route may be mixed on one pair: the stream index, and so both phases, continues across
 * them, and the same calls give the same bits by every route.  Stream ordering, the caller-keeps-memory rule, errors, the
 * device rule, determinism and the bank rule are those of the zoom cross object.
 * Memory: per (pair, stage) two ping-pong buffers for each of the four streams, plus 128 MB of pinned staging. */
#define PSDC_IQCSD_STEADY_LAUNCHES 4
typedef struct psdc_iqcsd psdc_iqcsd;
/* 1 if an object of size n can be created, else 0.  Pure host code. */
int psdc_iqcsd_supported(uint32_t n);
/* n_pairs pairs; window_kind PSDC_WINDOW_HANN / _RECTANGULAR */
psdc_iqcsd *psdc_iqcsd_create(uint32_t n, int window_kind, uint32_t n_pairs, int device);
/* the same with a caller-built Window<N> (src/psd.rs:12-20), as psdc_create_window */
psdc_iqcsd *psdc_iqcsd_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                     int device);
void psdc_iqcsd_destroy(psdc_iqcsd *h);
/* back to the state of a fresh object: stages, buffers, settings, carriers and statistics */
int psdc_iqcsd_reset(psdc_iqcsd *h);
int psdc_iqcsd_set_detrend(psdc_iqcsd *h, int detrend_kind);
int psdc_iqcsd_set_avg(psdc_iqcsd *h, uint32_t limit, uint32_t count);
/* the carrier of one side of a pair (side 0: stream a, 1: stream b); PSDC_ERR_ARG once the pair has taken a sample */
int psdc_iqcsd_set_carrier(psdc_iqcsd *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0);
/* len complex samples of each side from host memory, planar: ia[j] + i qa[j] and ib[j] + i qb[j] */
int psdc_iqcsd_process(psdc_iqcsd *h, uint32_t pair, const float *ia, const float *qa, const float *ib, const float *qb,
                       size_t len);
/* the same from device memory (any 4-byte aligned addresses and any length); producer_event: hipEvent_t or NULL */
int psdc_iqcsd_process_device(psdc_iqcsd *h, uint32_t pair, const float *d_ia, const float *d_qa, const float *d_ib,
                              const float *d_qb, size_t len, void *producer_event);
/* len complex samples of each side as (re, im) pairs, 2 len floats a side, 8-byte aligned, from host memory */
int psdc_iqcsd_process_interleaved(psdc_iqcsd *h, uint32_t pair, const float *za, const float *zb, size_t len);
/* the same from device memory */
int psdc_iqcsd_process_interleaved_device(psdc_iqcsd *h, uint32_t pair, const float *d_za, const float *d_zb, size_t len,
                                          void *producer_event);
/* Stream frames into IQ cross pairs (mirrors psdc_zoomcsdcascade_process_frames).  The map has 4 n_pairs entries: pair p takes
 * the traces pair_traces[4 p ... 4 p + 3] of every frame as I_a, Q_a, I_b, Q_b, in Payload::traces order (Fls: BI = 2, BQ = 3).
 * All four entries PSDC_TRACE_NONE: the pair is not fed by this call and its stream index does not move; one to three of them
 * is PSDC_ERR_ARG.  A trace may feed any number of sides and entries.  The map belongs to the call and is not stored.
 * Every other map, format, cut, Loss and *n_ok rule is that call's: PSDC_ERR_ARG without ingesting anything for a NULL map, a
 * trace index >= 4 or a map that feeds no pair; a run whose format carries fewer traces than the map names is PSDC_ERR_ARG at
 * the run's first frame, the frames before it ingested and counted in *n_ok; pieces of whole frames of at most 2^22 samples a
 * trace, cut by the headers alone; Loss committed piece by piece; one psdc_loss an object, zeroed by a reset.
 * Each piece is ONE decode-and-mix launch per 8 fed pairs (iq_cross_frames_kernel: a cell is read and converted once, handed to
 * every entry of every pair that takes it, each side turned in registers and stored to its I and Q streams; the f32 traces never
 * exist in memory) and then one round.  A one-piece call gives the same bits as the planar sample call fed Payload::traces of
 * the same frames; host and device frames give the same bits; a steady-state one-piece call that feeds up to 8 pairs is 1 + 3
 * launches, and the device call's header gather is a fifth that psdc_iqcsd_stats_read counts.  Host frames go up through the
 * pinned staging into a 64 MB device buffer made by the first host-frames call. */
int psdc_iqcsd_process_frames(psdc_iqcsd *h, const uint32_t *pair_traces, const uint8_t *frames, size_t frame_size,
                              size_t n_frames, size_t *n_ok);
int psdc_iqcsd_process_frames_device(psdc_iqcsd *h, const uint32_t *pair_traces, const uint8_t *d_frames, size_t frame_size,
                                     size_t n_frames, size_t *n_ok, void *producer_event);
/* the Loss counters of the frames the object ingested; reset != 0 zeroes them after reading */
int psdc_iqcsd_loss_read(psdc_iqcsd *h, psdc_loss *out, int reset);
int psdc_iqcsd_sync(psdc_iqcsd *h);
int psdc_iqcsd_num_stages(psdc_iqcsd *h, uint32_t pair);
/* raw accumulators of one stage: rows 8 (n/2 + 1) floats in the zoom cross object's row layout; stat and rows may be NULL */
int psdc_iqcsd_stage_spectra(psdc_iqcsd *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, float *rows);
/* PsdCascade::psd of every row, with the arguments of psdc_zcsd_csd: the auto rows `cap` floats each, sab_upper and sab_lower
 * 2 cap floats (re, im); any may be NULL */
int psdc_iqcsd_csd(psdc_iqcsd *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band,
                   float *saa_upper, float *saa_lower, float *sbb_upper, float *sbb_lower, float *sab_upper,
                   float *sab_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and complex sample pairs accepted since creation or the last reset of the statistics */
int psdc_iqcsd_stats_read(psdc_iqcsd *h, uint64_t *launches, uint64_t *pairs_in, int reset);
const char *psdc_iqcsd_last_error(const psdc_iqcsd *h);

/* ---- integer sample feeds: int16 / int8 samples into the zoom and IQ objects (s16 / s8, sc16 / sc8) -----------------------
 * Hardware does not deliver f32: an SDR delivers interleaved 16-bit or 8-bit integer pairs, a capture card a real int16
 * stream.  The four mixer-fronted objects (zoom, zoom cross, IQ, IQ cross) take such a stream as it is; the mixer in front of
 * stage 0 reads the integers where it reads floats on the f32 routes, so there is no widened copy and no extra launch.
 * Kinds: PSDC_SAMPLE_S16 (int16, native endian) and PSDC_SAMPLE_S8 (int8).  Unit: for the real-input objects (zoom, zoom
 * cross) one integer; for the complex-input objects (IQ, IQ cross) one interleaved (re, im) pair of that type -- sc16 (4
 * bytes) or sc8 (2 bytes).  There is no planar integer route.  `len` counts units.
 * Conversion: every call carries a `float scale`, and the f32 sample the mixer sees is (float)v * scale: the int-to-float
 * conversion is exact, and the product is one stand-alone f32 product rounded to nearest (__fmul_rn on the device; nothing is
 * contracted into the mix formulas of csrc/zoom_lo.h and csrc/iq_lo.h).  scale must be finite, else PSDC_ERR_ARG.  2^-15 for
 * s16 and 2^-7 for s8 map full scale into [-1, 1) (the Python mirror's defaults).
 * The defining property: an integer call gives bit for bit what the object's existing f32 call of the same length -- the
 * interleaved call of the complex objects, the plain call of the real ones -- gives when that call is fed
 * float32(v) * float32(scale), on the same object state and from the same memory side (host or device).  Integer, f32 and
 * frames calls may be mixed on one channel or pair in any order; the stream index, and so the phase, continues across them.
 * Arguments: pointers aligned to the unit (2 bytes for s16, 1 for s8, 4 for sc16, 2 for sc8), else PSDC_ERR_ARG; an unknown
 * kind is PSDC_ERR_ARG; NULL with len > 0 is PSDC_ERR_ARG; len == 0 is PSDC_OK.  A failed call leaves the object as it was.
 * Stream ordering, the producer_event meaning, the caller-keeps-memory rule and lifetimes are exactly those of the object's
 * f32 device call; the error text goes through the object's *_last_error.  Host calls go up through the same pinned staging
 * into the front of the same landing buffer as raw integers, cut into pieces of 2^22 units as the f32 calls are cut into pieces
 * of 2^22 samples, so an integer call makes the launches and rounds of the f32 call of the same length (1 + 3 a steady call for
 * zoom, IQ and IQ cross, 2 + 3 for zoom cross) and *_stats_read counts as before; device calls read the caller's memory in place.
 * Kernels: csrc/sample_int.hip (zoom_mix_int_kernel, iq_mix_int_kernel, iq_pair_mix_int_kernel, each for int16_t and int8_t),
 * siblings of the f32 mixers with their access scheme and, on a pair, their shared oscillator; csrc/sample_int.h holds the
 * index map and the unpack-and-scale, and runs on the host in tests/host/sample_int_emul.cpp.  The ABI stays at version 3. */
#define PSDC_SAMPLE_S16 1 /* int16, native endian */
#define PSDC_SAMPLE_S8 2  /* int8 */
/* len real integers into one zoom channel, from host memory / from device memory */
int psdc_int_zoom_process(psdc_zoom *h, uint32_t channel, const void *x, int kind, float scale, size_t len);
int psdc_int_zoom_process_device(psdc_zoom *h, uint32_t channel, const void *d_x, int kind, float scale, size_t len,
                                 void *producer_event);
/* len real integers of each side into one zoom cross pair (both sides of one kind and scale) */
int psdc_int_zcsd_process(psdc_zcsd *h, uint32_t pair, const void *xa, const void *xb, int kind, float scale, size_t len);
int psdc_int_zcsd_process_device(psdc_zcsd *h, uint32_t pair, const void *d_xa, const void *d_xb, int kind, float scale,
                                 size_t len, void *producer_event);
/* len interleaved (re, im) integer pairs into one IQ channel */
int psdc_int_iq_process(psdc_iq *h, uint32_t channel, const void *z, int kind, float scale, size_t len);
int psdc_int_iq_process_device(psdc_iq *h, uint32_t channel, const void *d_z, int kind, float scale, size_t len,
                               void *producer_event);
/* len interleaved (re, im) integer pairs of each side into one IQ cross pair (both sides of one kind and scale) */
int psdc_int_iqcsd_process(psdc_iqcsd *h, uint32_t pair, const void *za, const void *zb, int kind, float scale, size_t len);
int psdc_int_iqcsd_process_device(psdc_iqcsd *h, uint32_t pair, const void *d_za, const void *d_zb, int kind, float scale,
                                  size_t len, void *producer_event);

/* ---- integer sample feeds of the real-input objects: int16 / int8 samples into the PSD, pair and matrix objects (s16 / s8) --
 * The three objects with no mixer in front of stage 0 (psdc_handle, psdc_cross, psdc_csm) take the same integers under the rule
 * of the section above: kinds PSDC_SAMPLE_S16 / PSDC_SAMPLE_S8, one integer a unit, `len` counts units, the f32 sample the
 * object sees is (float)v * scale as defined there, and the arguments behave as stated there (pointers aligned to the integer,
 * a finite scale, an unknown kind, NULL with len > 0: PSDC_ERR_ARG; len == 0: PSDC_OK; a failed call leaves the object as it
 * was; the error text names the call and goes through psdc_last_error / psdc_cross_last_error / psdc_csm_last_error).
 * With no mixer to read the integers, a converter (csrc/sample_int.hip, sample_cvt_int_kernel for int16_t and int8_t: the
 * mixers' access scheme without the oscillator, one launch for the 1 ... 4 channels of a call) writes the f32 samples into the
 * stage-0 stream buffers exactly where the f32 call's copy writes them.
 * Pair and matrix: an integer call gives bit for bit what the f32 call (psdc_cross_process[_device], psdc_csm_process[_device])
 * of float32(v) * float32(scale) gives, from the same memory side, on the same object state, in every row of every stage;
 * integer, f32 and frames calls mix on one pair or group in any order.  Host calls carry the raw integers through the pinned
 * staging into a landing buffer (m 2^22 floats, made by the first such call) in the f32 call's pieces of 2^22 units: per piece
 * the m copies and ONE converter launch, so a steady host call makes the f32 call's launches (3 a round) + 1 a piece, 4 for a
 * call of at most 2^22 units.  A device call has ONE converter launch on the copy stream where the f32 call has its m copies,
 * under the same event rules (3 + 1 launches a steady call); the caller's memory is read by that launch alone, so stream ordering,
 * producer_event and lifetimes are those of the f32 device call.  psdc_cross_stats_read / psdc_csm_stats_read count the converter.
 * PSD object, host: psdc_sint_process follows psdc_process step for step -- the same pinned staging holding the raw integers,
 * the same quantum counted in samples, the same fast path (a bounds check and a memcpy while the staged samples stay below the
 * quantum).  A staged fill of integers is uploaded into a landing buffer of the handle (2 quantum bytes, made by the first such
 * upload) and converted on the copy stream into the place the f32 upload writes.  A call whose (kind, scale) differs from what
 * the channel's staging holds -- f32 against integers, s16 against s8, another scale -- submits the staged samples first.  So
 * a stream fed with ONE (kind, scale) gives the BITS of psdc_process fed float32(v) * float32(scale) in the same call sizes;
 * where kinds change inside a quantum the chunk-invariance statement of psdc_process holds: counters exact, spectra to rounding.
 * PSD object, device: psdc_sint_process_device takes the route of a SHORT f32 span: producer_event is waited for on the handle's
 * stream, earlier spans and staged host samples of the channel go out first, and the converter writes the stage-0 stream buffer
 * (calls longer than 2^26 units in pieces of that many).  The integers are NOT read in place by the fused kernels: the route
 * costs one extra pass over the stream compared with an in-place f32 span.  The caller's buffer is read by the converter
 * launches only and must stay valid and unmodified until psdc_sync, a read-out or a psdc_record_consumed event, as an f32 span.
 * The thread function runs on the host in tests/host/sample_cvt_emul.cpp.  The ABI stays at version 3. */
int psdc_sint_process(psdc_handle *h, uint32_t channel, const void *x, int kind, float scale, size_t len);
int psdc_sint_process_device(psdc_handle *h, uint32_t channel, const void *d_x, int kind, float scale, size_t len,
                             void *producer_event);
/* len integers of each side into one pair (both sides of one kind and scale) */
int psdc_sint_cross_process(psdc_cross *h, uint32_t pair, const void *x, const void *y, int kind, float scale, size_t len);
int psdc_sint_cross_process_device(psdc_cross *h, uint32_t pair, const void *d_x, const void *d_y, int kind, float scale,
                                   size_t len, void *producer_event);
/* len integers of each of the m channels of one group (x: m pointers, the array itself in host memory) */
int psdc_sint_csm_process(psdc_csm *h, uint32_t group, const void *const *x, int kind, float scale, size_t len);
int psdc_sint_csm_process_device(psdc_csm *h, uint32_t group, const void *const *d_x, int kind, float scale, size_t len,
                                 void *producer_event);

/* ---- spectral kurtosis cascade: per-bin Gaussianity beside the PSD ------------------------------------------------
 * Every other object keeps first moments of the periodogram P_j[k] = |X_j[k]|^2: how much power a bin holds.  This one keeps
 * the second moment beside it, which tells stationary Gaussian noise from a coherent line, a burst, or a source that is on
 * part of the time -- all of which read the same in the PSD.
 * Unit and stages: a unit is one real f32 stream; `n_channels` independent ones.  Per stage the segmentation, Window<N>,
 * Detrend, /8 half-band decimation with the drain of 35 outputs, lazy stages and the averaging schedule (set_avg) are those of
 * PsdCascade<N> fed the same stream -- what a pair object does per channel.  A channel has exactly the stages, counts,
 * pendings and Breaks of a PsdCascade fed x.
 * Rows: each (channel, stage) holds two f64 rows of n/2 + 1 bins,
 *     row 0:  S1[k] = sum_j w_j P_j[k],        row 1:  S2[k] = sum_j w_j P_j[k]^2,
 * with w_j the weights a pair object gives S_xx: 1 while the stage averages as a boxcar, then the EWMA weights of
 * src/psd.rs:218-233; both rows are folded with the same factor.  Row 0 is therefore the pair object's S_xx row and
 * PsdCascade's spectrum (to 1e-5 relative: the rounding order differs).
 * Weights: the segment kernel transforms with amplitude 1 and weights both products afterwards, (w P) and (w P) P; the weight
 * is never squared and never divided by (csrc/sk_fft.h).
 * Estimator: with M = count, the stage's reported count (psdc_stage_stat.count),
 *     SK[k] = (M + 1) / (M - 1) * (M S2[k] / S1[k]^2 - 1),
 * computed on the host in f64 from the f64 rows.  It is defined for count >= 2; below that, and where S1[k] == 0, a bin reads
 * NaN.  Readings: 1 for Gaussian noise of any colour (a linear filter keeps Gaussian noise Gaussian, so at every stage);
 * 0 for a line of constant amplitude; about 2/d - 1 for noise present a fraction d of the time.  The real-valued bins 0 and N/2
 * read 2 for Gaussian noise (their P is chi-squared with one degree of freedom, not two).  For Gaussian noise the standard
 * deviation of a bin is about 2 / sqrt(M).
 * EWMA regime: once count sits at the averaging limit the weights decay geometrically and M = count is an approximation: the
 * effective number of averages is about 2 count - 1, so SK carries a bias of order 1 / count.
 * Range: a workgroup's partial rows are f32, so P^2 summed over the segments a workgroup takes in one round must stay below
 * f32 max (3.4e38); the accumulators themselves are f64.
 * Merged read-out: psdc_sk_psd is PsdCascade::psd (src/psd.rs:479-543) of row 0, with the same MergeOpts, bins, Breaks and gain
 * as psdc_psd.  psdc_sk_sk returns the same Breaks and bin selection: bin i of the merged array is the SK of the stage and bin
 * that psdc_sk_psd took bin i from (no gain applies: SK is a ratio).  It is written in f64.
 * Sizes and windows are those of pairs: n a power of two 64 ... 4096; Window::hann(), Window::rectangular(), or a caller's
 * table with (n - overlap) % 8 == 0.  Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere.  There is no CPU fallback.
 * Stream ordering, the caller-keeps-memory rule, errors and the device rule are those of the pair object: host samples go up
 * through the pinned staging, device samples are copied on the side stream behind producer_event, a grown buffer and round
 * R - 2.  A steady round is 3 kernel launches whatever the depth (segments, decimators, fold + tails).  Host and device
 * calls of the same samples, and the same calls twice, give the same bits; a bank's channel equals a single object under the
 * rule stated for the zoom object.  Stream frames and integer samples do not feed this object yet. */
typedef struct psdc_sk psdc_sk;
/* 1 where n is a size the object takes, else 0 */
int psdc_sk_supported(uint32_t n);
psdc_sk *psdc_sk_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
psdc_sk *psdc_sk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                               int device);
void psdc_sk_destroy(psdc_sk *h);
int psdc_sk_reset(psdc_sk *h);
int psdc_sk_set_detrend(psdc_sk *h, int detrend_kind);
int psdc_sk_set_avg(psdc_sk *h, uint32_t limit, uint32_t count);
/* len real samples of a channel from host memory */
int psdc_sk_process(psdc_sk *h, uint32_t channel, const float *x, size_t len);
/* the same from device memory; producer_event: hipEvent_t or NULL */
int psdc_sk_process_device(psdc_sk *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
int psdc_sk_sync(psdc_sk *h);
int psdc_sk_num_stages(psdc_sk *h, uint32_t channel);
/* raw f64 accumulators of one stage: s1, s2 n/2 + 1 doubles each; any may be NULL */
int psdc_sk_stage_moments(psdc_sk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1, double *s2);
/* the merged PSD (row 0): psd `cap` floats, may be NULL to query sizes */
int psdc_sk_psd(psdc_sk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *psd,
                size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* the merged SK: sk `cap` doubles, may be NULL to query sizes; the Breaks and the length are those of psdc_sk_psd */
int psdc_sk_sk(psdc_sk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk,
               size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* kernel launches issued and samples accepted since creation or the last reset of the statistics */
int psdc_sk_stats_read(psdc_sk *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_sk_last_error(const psdc_sk *h);

/* ---- zoom and IQ spectral kurtosis cascades: SK around a carrier ---------------------------------------------------
 * The spectral kurtosis object takes real streams from DC upwards.  The streams SK is used on most are complex: I/Q from an
 * SDR front end or a lock-in, the Fls BI / BQ traces, or a narrow band around a carrier of a real stream.  These two objects
 * keep the second moment of the periodogram beside the first on the two-sided cascade: psdc_zsk_* is the zoom object (a real
 * stream plus a carrier, fed as psdc_zoom_* is) and psdc_iqsk_* the IQ object (a complex stream plus an optional retune, fed
 * as psdc_iq_* is).  Both share one segment kernel (csrc/zoom_sk.hip).
 * Unit, carrier and stages: those of the zoom / IQ object fed the same stream and carrier -- segmentation, Window<N>, Detrend,
 * /8 decimation of I and Q with the drain of 35 outputs, lazy stages, the averaging schedule (set_avg), counts, pendings and
 * Breaks.
 * Rows: each (channel, stage) holds four f64 rows of n/2 + 1 bins, in this order, Z the transform of the segment's I + i Q:
 *     row 0:  s1_upper[k] = sum_j w_j |Z_j[k]|^2              row 1:  s1_lower[k] = sum_j w_j |Z_j[(N - k) mod N]|^2
 *     row 2:  s2_upper[k] = sum_j w_j |Z_j[k]|^4              row 3:  s2_lower[k] = sum_j w_j |Z_j[(N - k) mod N]|^4
 * with w_j the weights of the spectral kurtosis object: 1 while the stage averages as a boxcar, then the EWMA weights; all four
 * rows are folded with the same factor.  Rows 0 and 1 are therefore the zoom / IQ object's `upper` and `lower` (to 1e-5
 * relative: the weight goes on the products here, on the samples there).  The transform runs with amplitude 1 and the weight is
 * applied as (w P) and (w P) P, never squared and never divided by (csrc/zoom_sk_fft.h, csrc/sk_fft.h).
 * Estimator: SK = (M + 1) / (M - 1) * (M S2 / S1^2 - 1) with M = count, per side, in f64 on the host, in the operation order
 * of the spectral kurtosis object; NaN below two averages and where S1 == 0.
 * What SK reads on complex bins: every bin of a complex stream is complex, so circular Gaussian noise reads 1 at every bin,
 * offset 0 and Nyquist included: the real object's "2 at the real-valued bins" does not occur.  A line of constant amplitude
 * reads 0; power that is on a fraction d of the time reads about 2/d - 1.  A real stream mixed from f0 is not circular where
 * its own DC and Nyquist fall: near offset f0 in `lower` and offset 0.5 - f0 in `upper` (for 0 < f0 < 0.5) SK rises towards 2.
 * A numpy model (N = 512, f0 = 0.2, 2^21 samples, Hann) read 1.29 and 1.56 at upper bins 153 and 154 and 1.31 and 1.60 at
 * lower bins 103 and 102, every other bin inside 16 / sqrt(count); circular complex Gaussian noise in the same model read
 * 5.8 / sqrt(count) at its worst bin, 1.013 at bin 0 and 1.000 at bin N/2.  The EWMA regime and the f32 range of a workgroup's
 * partial rows are as stated for the spectral kurtosis object.
 * Merged read-out: psdc_zsk_psd / psdc_iqsk_psd are psdc_zoom_psd of rows 0 and 1.  psdc_zsk_sk / psdc_iqsk_sk return the same
 * Breaks and bin selection: bin i of each merged array is the SK of the stage and bin the psd took bin i from (no gain: SK is
 * a ratio; no new stitch).  Offsets are read as the zoom object's are.
 * Sizes and windows are those of psdc_sk_supported and of the zoom object; Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as
 * everywhere.  There is no CPU fallback.  Sample routes, stream ordering, the caller-keeps-memory rule, errors, the device
 * rule and the bank rule are those of psdc_zoom_* / psdc_iq_*: a steady-state call is 1 + 3 kernel launches (mixer; segments,
 * decimators, fold + tails); host and device calls of the same samples, and the same calls twice, give the same bits.  Only
 * the f32 sample routes feed these objects yet. */
typedef struct psdc_zsk psdc_zsk;
/* 1 where n is a size the object takes, else 0 (psdc_sk_supported) */
int psdc_zsk_supported(uint32_t n);
/* mirrors psdc_zoom_create / psdc_zoom_create_window */
psdc_zsk *psdc_zsk_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
psdc_zsk *psdc_zsk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                 int device);
void psdc_zsk_destroy(psdc_zsk *h);
/* as psdc_zoom_reset: stages, buffers, settings, carriers and statistics */
int psdc_zsk_reset(psdc_zsk *h);
int psdc_zsk_set_detrend(psdc_zsk *h, int detrend_kind);
int psdc_zsk_set_avg(psdc_zsk *h, uint32_t limit, uint32_t count);
/* as psdc_zoom_set_carrier; PSDC_ERR_ARG once the channel has taken a sample */
int psdc_zsk_set_carrier(psdc_zsk *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* as psdc_zoom_process / psdc_zoom_process_device */
int psdc_zsk_process(psdc_zsk *h, uint32_t channel, const float *x, size_t len);
int psdc_zsk_process_device(psdc_zsk *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
int psdc_zsk_sync(psdc_zsk *h);
int psdc_zsk_num_stages(psdc_zsk *h, uint32_t channel);
/* raw f64 accumulators of one stage (as psdc_sk_stage_moments, per side): n/2 + 1 doubles each; any may be NULL */
int psdc_zsk_stage_moments(psdc_zsk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1_upper,
                           double *s1_lower, double *s2_upper, double *s2_lower);
/* psdc_zoom_psd of rows 0 and 1 */
int psdc_zsk_psd(psdc_zsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                 float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* the merged SK of both sides (as psdc_sk_sk): sk_upper, sk_lower `cap` doubles each, either may be NULL; the Breaks and the
 * length are those of psdc_zsk_psd */
int psdc_zsk_sk(psdc_zsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk_upper,
                double *sk_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* as psdc_zoom_stats_read */
int psdc_zsk_stats_read(psdc_zsk *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_zsk_last_error(const psdc_zsk *h);

typedef struct psdc_iqsk psdc_iqsk;
int psdc_iqsk_supported(uint32_t n);
/* mirrors psdc_iq_create / psdc_iq_create_window */
psdc_iqsk *psdc_iqsk_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
psdc_iqsk *psdc_iqsk_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                   int device);
void psdc_iqsk_destroy(psdc_iqsk *h);
int psdc_iqsk_reset(psdc_iqsk *h);
int psdc_iqsk_set_detrend(psdc_iqsk *h, int detrend_kind);
int psdc_iqsk_set_avg(psdc_iqsk *h, uint32_t limit, uint32_t count);
/* as psdc_iq_set_carrier: the retune, default 0, 0 */
int psdc_iqsk_set_carrier(psdc_iqsk *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* the four f32 sample routes of psdc_iq_*: planar and interleaved, host and device */
int psdc_iqsk_process(psdc_iqsk *h, uint32_t channel, const float *i, const float *q, size_t len);
int psdc_iqsk_process_device(psdc_iqsk *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event);
int psdc_iqsk_process_interleaved(psdc_iqsk *h, uint32_t channel, const float *iq, size_t len);
int psdc_iqsk_process_interleaved_device(psdc_iqsk *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event);
int psdc_iqsk_sync(psdc_iqsk *h);
int psdc_iqsk_num_stages(psdc_iqsk *h, uint32_t channel);
/* as psdc_zsk_stage_moments, psdc_zsk_psd (psdc_iq_psd of rows 0 and 1) and psdc_zsk_sk */
int psdc_iqsk_stage_moments(psdc_iqsk *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *s1_upper,
                            double *s1_lower, double *s2_upper, double *s2_lower);
int psdc_iqsk_psd(psdc_iqsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                  float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
int psdc_iqsk_sk(psdc_iqsk *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, double *sk_upper,
                 double *sk_lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* as psdc_iq_stats_read: complex samples accepted */
int psdc_iqsk_stats_read(psdc_iqsk *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_iqsk_last_error(const psdc_iqsk *h);

/* ---- AM/PM cascades: amplitude and phase noise spectra of a carrier ------------------------------------------------
 * The two-sided objects keep |Z_k|^2 of each sideband of a carrier.  Their sum is S_am + S_pm and their difference
 * Im S_am,pm: how much of the sideband power is amplitude noise and how much phase noise they cannot say.  These two objects
 * keep one more complex accumulator a bin on the same transform, the complementary spectrum comp[k] = sum_j w_j Z_j[k]
 * Z_j[(N - k) mod N] -- a product WITHOUT a conjugate.  For z = A (1 + a(t) + i phi(t)), a and phi real and small,
 *     (upper + lower) / 2 = |A|^2 (S_a + S_phi)                          upper - lower = -4 |A|^2 Im S_a,phi
 *     comp conj(u)        = |A|^2 (S_a - S_phi + 2 i Re S_a,phi),        u = A^2 / |A|^2
 * with S_a,phi = conj(a_k) phi_k: one transform a segment gives S_am, S_pm and the AM-PM cross spectrum at every stage.  The
 * relation is a frequency-domain one: no unwrap, no per-sample transcendental, no state beyond the zoom object's.  psdc_zampm_* is
 * the zoom object (a real stream plus a carrier, fed as psdc_zoom_* is) and psdc_iqampm_* the IQ object (a complex stream plus
 * an optional retune, fed as psdc_iq_* is).  Both share one segment kernel (csrc/zoom_ampm.hip).
 * Unit, carrier and stages: those of the zoom / IQ object fed the same stream and carrier -- segmentation, Window<N>, Detrend,
 * /8 decimation of I and Q with the drain of 35 outputs, lazy stages, the averaging schedule (set_avg) with its EWMA weights,
 * counts, pendings and Breaks.
 * Rows: each (channel, stage) holds four f64 rows of n/2 + 1 bins, in this order, Z the transform of the segment's I + i Q:
 *     row 0:  upper[k]   = sum_j w_j |Z_j[k]|^2                 row 1:  lower[k]   = sum_j w_j |Z_j[(N - k) mod N]|^2
 *     row 2:  comp_re[k] = sum_j w_j Re(Z_j[k] Z_j[(N - k) mod N])   row 3:  comp_im[k] = the imaginary part of the same
 * At k = 0 and k = N/2 the product is Z[k]^2.  All four rows are bilinear in Z: the weight goes on the samples as sqrt(w_j), as in
 * the zoom object, and all four are folded with the same factor.  Rows 0 and 1 are the zoom / IQ object's `upper` and `lower`
 * (to rounding: 2e-6).
 * Carrier: bin 0 of comp at stage 0 is sum Z[0]^2 = A^2 (sum win)^2 per segment, so the carrier's phasor u = comp[0] / |comp[0]|,
 * its power and the lock figure |comp[0]| / sqrt(upper[0] lower[0]) (1 for a carrier at the tuning word, towards 0 for one
 * that turns during the average) come from the same rows; the Python module reads them (carrier(), am_pm()).
 * Limits: the separation is a linear, small-modulation one -- phi^2 reads as AM at second order; the carrier must sit at the
 * tuning word to within the reciprocal of the averaging time; bins 0 and 1 of every stage hold the carrier itself under Hann; a
 * real stream's image at -2 f0 is where the zoom object has it.
 * Merged read-out: psdc_zampm_psd / psdc_iqampm_psd are psdc_zoom_psd of rows 0 and 1.  psdc_zampm_sidebands /
 * psdc_iqampm_sidebands stitch all four rows with that read-out's Breaks and its per-stage factor, in f64: the AM/PM split is
 * a difference of nearly equal numbers when one modulation dominates.  Offsets are read as the zoom object's are.
 * Sizes and windows are those of the zoom object (64 ... 4096); Detrend::Linear is PSDC_ERR_UNIMPLEMENTED as everywhere.  There
 * is no CPU fallback.  Sample routes, stream ordering, the caller-keeps-memory rule, errors, the device rule and the bank rule
 * are those of psdc_zoom_* / psdc_iq_*: a steady-state call is 1 + 3 kernel launches (mixer; segments, decimators, fold +
 * tails); host and device calls of the same samples, and the same calls twice, give the same bits.  Only the f32 sample routes
 * feed these objects: stream frames, the loss record and the integer feeds are not offered yet. */
typedef struct psdc_zampm psdc_zampm;
/* 1 where n is a size the object takes, else 0 */
int psdc_zampm_supported(uint32_t n);
/* mirrors psdc_zoom_create / psdc_zoom_create_window */
psdc_zampm *psdc_zampm_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
psdc_zampm *psdc_zampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                     int device);
void psdc_zampm_destroy(psdc_zampm *h);
/* as psdc_zoom_reset: stages, buffers, settings, carriers and statistics */
int psdc_zampm_reset(psdc_zampm *h);
int psdc_zampm_set_detrend(psdc_zampm *h, int detrend_kind);
int psdc_zampm_set_avg(psdc_zampm *h, uint32_t limit, uint32_t count);
/* as psdc_zoom_set_carrier; PSDC_ERR_ARG once the channel has taken a sample */
int psdc_zampm_set_carrier(psdc_zampm *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* as psdc_zoom_process / psdc_zoom_process_device */
int psdc_zampm_process(psdc_zampm *h, uint32_t channel, const float *x, size_t len);
int psdc_zampm_process_device(psdc_zampm *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
int psdc_zampm_sync(psdc_zampm *h);
int psdc_zampm_num_stages(psdc_zampm *h, uint32_t channel);
/* raw f64 accumulators of one stage: n/2 + 1 doubles each; any may be NULL */
int psdc_zampm_stage_rows(psdc_zampm *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *upper, double *lower,
                          double *comp_re, double *comp_im);
/* psdc_zoom_psd of rows 0 and 1 */
int psdc_zampm_psd(psdc_zampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                   float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* all four rows merged in f64: `cap` doubles each, any may be NULL; the Breaks and the length are those of psdc_zampm_psd */
int psdc_zampm_sidebands(psdc_zampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                         double *upper, double *lower, double *comp_re, double *comp_im, size_t cap, size_t *len,
                         psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* as psdc_zoom_stats_read */
int psdc_zampm_stats_read(psdc_zampm *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_zampm_last_error(const psdc_zampm *h);

typedef struct psdc_iqampm psdc_iqampm;
int psdc_iqampm_supported(uint32_t n);
/* mirrors psdc_iq_create / psdc_iq_create_window */
psdc_iqampm *psdc_iqampm_create(uint32_t n, int window_kind, uint32_t n_channels, int device);
psdc_iqampm *psdc_iqampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                       int device);
void psdc_iqampm_destroy(psdc_iqampm *h);
int psdc_iqampm_reset(psdc_iqampm *h);
int psdc_iqampm_set_detrend(psdc_iqampm *h, int detrend_kind);
int psdc_iqampm_set_avg(psdc_iqampm *h, uint32_t limit, uint32_t count);
/* as psdc_iq_set_carrier: the retune, default 0, 0 */
int psdc_iqampm_set_carrier(psdc_iqampm *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* the four f32 sample routes of psdc_iq_*: planar and interleaved, host and device */
int psdc_iqampm_process(psdc_iqampm *h, uint32_t channel, const float *i, const float *q, size_t len);
int psdc_iqampm_process_device(psdc_iqampm *h, uint32_t channel, const float *d_i, const float *d_q, size_t len, void *producer_event);
int psdc_iqampm_process_interleaved(psdc_iqampm *h, uint32_t channel, const float *iq, size_t len);
int psdc_iqampm_process_interleaved_device(psdc_iqampm *h, uint32_t channel, const float *d_iq, size_t len, void *producer_event);
int psdc_iqampm_sync(psdc_iqampm *h);
int psdc_iqampm_num_stages(psdc_iqampm *h, uint32_t channel);
/* as psdc_zampm_stage_rows, psdc_zampm_psd (psdc_iq_psd of rows 0 and 1) and psdc_zampm_sidebands */
int psdc_iqampm_stage_rows(psdc_iqampm *h, uint32_t channel, uint32_t stage, psdc_stage_stat *stat, double *upper, double *lower,
                           double *comp_re, double *comp_im);
int psdc_iqampm_psd(psdc_iqampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band, float *upper,
                    float *lower, size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
int psdc_iqampm_sidebands(psdc_iqampm *h, uint32_t channel, int keep_overlap, uint32_t min_count, int keep_transition_band,
                          double *upper, double *lower, double *comp_re, double *comp_im, size_t cap, size_t *len,
                          psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* as psdc_iq_stats_read: complex samples accepted */
int psdc_iqampm_stats_read(psdc_iqampm *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_iqampm_last_error(const psdc_iqampm *h);

/* ---- AM/PM cross cascades: cross-correlated amplitude and phase noise of two channels --------------------------------
 * Two channels a and b on one carrier (two ADCs on one oscillator, two lock-ins, the two arms of a cross-correlation phase-noise
 * set-up): what the channels share survives the average of the cross spectra of their modulations, each channel's own noise
 * goes down as 1 / sqrt(count).  psdc_zxampm_* is the zoom cross object (two real streams, a carrier a side, fed as psdc_zcsd_*
 * is) and psdc_iqxampm_* the IQ cross object (two complex streams, an optional retune a side, fed as psdc_iqcsd_* is), both
 * on one segment kernel (csrc/zoom_ampm_cross.hip) that transforms each channel once a segment.
 * Unit, carriers and stages: those of the zoom cross / IQ cross object fed the same streams and carriers -- segmentation,
 * Window<N>, Detrend, /8 decimation of I and Q, lazy stages, the averaging schedule with its EWMA weights, counts, pendings and
 * Breaks.
 * Rows: each (pair, stage) holds twelve f64 rows of n/2 + 1 bins; kn = (N - k) mod N.
 *     rows 0 ... 7:  the zoom cross object's eight rows, in its order and with its signs (S_aa, S_bb, Re S_ab, Im S_ab, each upper
 *                    then lower; S_ab = conj(Z_a) Z_b; lower is the value at bin kn, not conjugated)
 *     rows 8, 9:     Re, Im of cab[k] = sum_j w_j Z_a,j[k] Z_b,j[kn]      a product WITHOUT a conjugate
 *     rows 10, 11:   Re, Im of cba[k] = sum_j w_j Z_a,j[kn] Z_b,j[k]
 * At k = 0 and k = N/2, cab == cba.  All twelve are bilinear in Z: the weight goes on the samples as sqrt(w_j).
 * Model: z_x = A_x (1 + a_x + i phi_x), v_x = A_x / |A_x|.  The carriers enter through w = conj(v_a) v_b, q = v_a v_b and
 * P = |A_a| |A_b| only, read from bin 0 of stage 0 under Detrend::None: sab_up[0] = P w count n^2 window_power and
 * cab[0] = P q count n^2 window_power; the locks are |sab_up[0]| / sqrt(saa_up[0] sbb_up[0]) and
 * |cab[0]| / sqrt(saa_up[0] sbb_lo[0]).  With U = sab_up, L = sab_lo, T1 = U conj(w), T2 = conj(cab) q, T3 = cba conj(q),
 * T4 = conj(L) w:
 *     s_am    = conj(a_a) a_b     = ( T1 + T2 + T3 + T4) / (4 P)        s_pm    = conj(phi_a) phi_b = (T1 - T2 - T3 + T4) / (4 P)
 *     s_am_pm = conj(a_a) phi_b   = ( T1 - T2 + T3 - T4) / (4 i P)      s_pm_am = conj(phi_a) a_b   = i (T1 + T2 - T3 - T4) / (4 P)
 * The Python module reads them (carriers(), am_pm_cross()).
 * Limits: those of the AM/PM cascades -- a linear, small-modulation split (phi^2 reads as AM at second order); both carriers at
 * their tuning words to within the reciprocal of the averaging time (the locks say whether they are); bins 0 and 1 of every
 * stage hold the carriers themselves under Hann.
 * Merged read-out: psdc_zxampm_sidebands / psdc_iqxampm_sidebands stitch all twelve rows in f64 with ONE set of Breaks, taken from
 * rows 0 and 1 as psdc_zampm_sidebands takes them, and the per-stage factor of that read-out.
 * Sizes and windows are those of the zoom cross object; the twelve-row kernel uses no scratch memory at any of them.  There is no
 * CPU fallback.  Sample routes, stream ordering, the caller-keeps-memory rule, errors, the device rule and the bank rule are those
 * of psdc_zcsd_* / psdc_iqcsd_*, and so are the kernel launches of a steady-state call (PSDC_ZCSD_STEADY_LAUNCHES,
 * PSDC_IQCSD_STEADY_LAUNCHES); host and device calls of the same samples, and the same calls twice, give the same bits.  Only the
 * f32 sample routes feed these objects: stream frames, the loss record and the integer feeds are not offered. */
typedef struct psdc_zxampm psdc_zxampm;
/* 1 where n is a size the object takes, else 0 */
int psdc_zxampm_supported(uint32_t n);
/* mirrors psdc_zcsd_create / psdc_zcsd_create_window */
psdc_zxampm *psdc_zxampm_create(uint32_t n, int window_kind, uint32_t n_pairs, int device);
psdc_zxampm *psdc_zxampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                       int device);
void psdc_zxampm_destroy(psdc_zxampm *h);
int psdc_zxampm_reset(psdc_zxampm *h);
int psdc_zxampm_set_detrend(psdc_zxampm *h, int detrend_kind);
int psdc_zxampm_set_avg(psdc_zxampm *h, uint32_t limit, uint32_t count);
/* as psdc_zcsd_set_carrier: side 0 is channel a, 1 channel b */
int psdc_zxampm_set_carrier(psdc_zxampm *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0);
/* as psdc_zcsd_process / psdc_zcsd_process_device */
int psdc_zxampm_process(psdc_zxampm *h, uint32_t pair, const float *x, const float *y, size_t len);
int psdc_zxampm_process_device(psdc_zxampm *h, uint32_t pair, const float *d_x, const float *d_y, size_t len, void *producer_event);
int psdc_zxampm_sync(psdc_zxampm *h);
int psdc_zxampm_num_stages(psdc_zxampm *h, uint32_t pair);
/* raw f64 accumulators of one stage: rows[12][n/2 + 1], or NULL for the statistics alone */
int psdc_zxampm_stage_rows(psdc_zxampm *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, double *rows);
/* all twelve rows merged in f64: rows[12][cap] (row r starts at rows + r * cap), or NULL for the length and the Breaks alone */
int psdc_zxampm_sidebands(psdc_zxampm *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, double *rows,
                          size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
/* as psdc_zcsd_stats_read */
int psdc_zxampm_stats_read(psdc_zxampm *h, uint64_t *launches, uint64_t *pairs_in, int reset);
const char *psdc_zxampm_last_error(const psdc_zxampm *h);

typedef struct psdc_iqxampm psdc_iqxampm;
int psdc_iqxampm_supported(uint32_t n);
/* mirrors psdc_iqcsd_create / psdc_iqcsd_create_window */
psdc_iqxampm *psdc_iqxampm_create(uint32_t n, int window_kind, uint32_t n_pairs, int device);
psdc_iqxampm *psdc_iqxampm_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_pairs,
                                         int device);
void psdc_iqxampm_destroy(psdc_iqxampm *h);
int psdc_iqxampm_reset(psdc_iqxampm *h);
int psdc_iqxampm_set_detrend(psdc_iqxampm *h, int detrend_kind);
int psdc_iqxampm_set_avg(psdc_iqxampm *h, uint32_t limit, uint32_t count);
/* as psdc_iqcsd_set_carrier: the retune of one side, default 0, 0 */
int psdc_iqxampm_set_carrier(psdc_iqxampm *h, uint32_t pair, uint32_t side, uint64_t ftw, uint64_t phase0);
/* the four f32 sample routes of psdc_iqcsd_*: planar and interleaved, host and device */
int psdc_iqxampm_process(psdc_iqxampm *h, uint32_t pair, const float *ia, const float *qa, const float *ib, const float *qb, size_t len);
int psdc_iqxampm_process_device(psdc_iqxampm *h, uint32_t pair, const float *d_ia, const float *d_qa, const float *d_ib,
                                const float *d_qb, size_t len, void *producer_event);
int psdc_iqxampm_process_interleaved(psdc_iqxampm *h, uint32_t pair, const float *za, const float *zb, size_t len);
int psdc_iqxampm_process_interleaved_device(psdc_iqxampm *h, uint32_t pair, const float *d_za, const float *d_zb, size_t len,
                                            void *producer_event);
int psdc_iqxampm_sync(psdc_iqxampm *h);
int psdc_iqxampm_num_stages(psdc_iqxampm *h, uint32_t pair);
/* as psdc_zxampm_stage_rows and psdc_zxampm_sidebands */
int psdc_iqxampm_stage_rows(psdc_iqxampm *h, uint32_t pair, uint32_t stage, psdc_stage_stat *stat, double *rows);
int psdc_iqxampm_sidebands(psdc_iqxampm *h, uint32_t pair, int keep_overlap, uint32_t min_count, int keep_transition_band, double *rows,
                           size_t cap, size_t *len, psdc_break *breaks, size_t breaks_cap, size_t *n_breaks);
int psdc_iqxampm_stats_read(psdc_iqxampm *h, uint64_t *launches, uint64_t *pairs_in, int reset);
const char *psdc_iqxampm_last_error(const psdc_iqxampm *h);

/* ---- waterfall cascades: time-resolved PSD and SK per stage ---------------------------------------------------------
 * Every other object averages over the whole stream: one set of accumulator rows a stage, read as the average since the last
 * reset.  These two keep, per stage, a ring of the most recent BLOCKS of segments, so that a spectrum that moves in time (a
 * drifting carrier, a mode hop, a spur that comes and goes, a servo ringing after a step) can be seen moving.  psdc_wf_* is the
 * spectral kurtosis object (real streams, fed as psdc_sk_* is) and psdc_zwf_* the zoom spectral kurtosis object (a real stream
 * mixed down from a carrier, fed as psdc_zsk_* is); the segment kernels, mixers, decimators and feeds are theirs, unchanged.
 * Construction: creation takes the sibling's arguments and
 *     block  B: segments a ring row, 2 ... 2^24 (SK needs M >= 2),
 *     depth  K: ring rows a stage, K >= 1.
 * A (channel, stage) ring is K * rows * (n/2 + 1) * 8 bytes (rows: 2 for psdc_wf, 4 for psdc_zwf); creation fails with
 * PSDC_ERR_ARG and a text naming the numbers when that exceeds 2^27 bytes.  Rings are allocated with their stages, lazily.
 * Sizes and windows are those of psdc_sk_supported / psdc_zsk_supported.  set_detrend and (psdc_zwf) set_carrier are the
 * siblings'.  There is no set_avg: every segment has weight 1.
 * Blocks and ring slots: block b of stage k is the segments [b B, (b + 1) B) of that stage, counted from the stream's start or
 * the last reset.  Block b lives in ring slot b mod K; the ring holds the newest min(K, blocks started) blocks.  The newest
 * block may be partial: its count is the number of its segments folded so far; every other block's count is B.  A slot holds
 * the sibling's rows of its block: S1 = sum P and S2 = sum P^2 (psdc_wf), or s1_upper, s1_lower, s2_upper, s2_lower (psdc_zwf).
 * A block that takes a slot over OVERWRITES it: what the slot held, a NaN included, does not decay into the new block.
 * Stage k's blocks are 8^k times longer in input time than stage 0's: the cascade's constant relative resolution, in time too.
 * Nominal time: block b of stage k nominally covers the input samples
 *     [b B hop 8^k,  ((b + 1) B - 1) hop 8^k + n 8^k),      hop = n - overlap.
 * The decimators' delay (their filter length and the 35 drained outputs a stage) is NOT included: a deeper stage's blocks lie
 * later in input time than this by that delay.
 * Feeding and draining: process, process_device, sync, reset, num_stages and stats_read behave as on the siblings; read-outs
 * drain.  A steady round whose pieces fit one job table costs the sibling's launches (3, and 1 + 3 for psdc_zwf); a round that
 * crosses many blocks is cut into one segment-kernel job a block and may take further launches, and a round longer than a ring
 * folds into a slot once a launch, in block order.  Host and device calls of the same samples, and the same calls twice, give
 * the same bits.
 * Read-outs: psdc_*_stage_blocks reports a stage's ring; psdc_*_stage_rows returns the raw f64 moment rows of the newest
 * `max_rows` blocks, oldest first, with each row's absolute block index and count; psdc_*_image turns them into f32 images on the
 * device (csrc/waterfall.hip), oldest block first:
 *     psd[r][k] = float32(S1[r][k] * (double)gsc_r),   gsc_r = 1.0f / (gain(n, count_r) * (float)8^stage),
 * the f32 factor the merged read-out applies to an included stage of that count and decimation (src/psd.rs:515-517), and
 *     sk[r][k]  = float32((M + 1) / (M - 1) * (M S2 / S1^2 - 1)),   M = count_r, evaluated in f64,
 * NaN where count_r < 2 or S1 == 0, as the spectral kurtosis object defines it.  psdc_wf images are [rows][n/2 + 1];
 * psdc_zwf images are [rows][2][n/2 + 1], side 0 upper and side 1 lower.
 * Out of scope: IQ feeds, stream frames, `loss` and integer feeds; averaging schedules and EWMA; cross, matrix and AM/PM
 * waterfalls; skipping pieces of blocks that the same round overwrites; compensating the decimators' delay in the nominal
 * time; more than one GPU an object.  There is no CPU fallback. */
typedef struct psdc_wf psdc_wf;
typedef struct psdc_zwf psdc_zwf;
/* what a stage's ring holds */
typedef struct psdc_wf_blocks {
    uint32_t block;        /* B: segments a block */
    uint32_t depth;        /* K: ring rows */
    uint64_t started;      /* blocks started since the stream's start or the last reset */
    uint32_t rows_valid;   /* min(K, started) */
    uint32_t newest_count; /* segments folded into the newest block, 1 ... B (0 before the first segment) */
    uint64_t pending;      /* as psdc_stage_stat.pending */
} psdc_wf_blocks;
/* 1 where n is a size the object takes, else 0 (psdc_sk_supported) */
int psdc_wf_supported(uint32_t n);
psdc_wf *psdc_wf_create(uint32_t n, int window_kind, uint32_t n_channels, uint32_t block, uint32_t depth, int device);
psdc_wf *psdc_wf_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                               uint32_t block, uint32_t depth, int device);
void psdc_wf_destroy(psdc_wf *h);
/* stages, rings, buffers, the detrend setting and statistics; block and depth stay */
int psdc_wf_reset(psdc_wf *h);
int psdc_wf_set_detrend(psdc_wf *h, int detrend_kind);
/* as psdc_sk_process / psdc_sk_process_device */
int psdc_wf_process(psdc_wf *h, uint32_t channel, const float *x, size_t len);
int psdc_wf_process_device(psdc_wf *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
int psdc_wf_sync(psdc_wf *h);
int psdc_wf_num_stages(psdc_wf *h, uint32_t channel);
int psdc_wf_stage_blocks(psdc_wf *h, uint32_t channel, uint32_t stage, psdc_wf_blocks *out);
/* the newest min(max_rows, rows_valid) blocks, oldest first: *n_rows of them; block_index, counts: max_rows entries, always
 * written; s1, s2: [max_rows][n/2 + 1] doubles, either may be NULL */
int psdc_wf_stage_rows(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, uint64_t *block_index, uint32_t *counts,
                       double *s1, double *s2, uint32_t *n_rows);
/* the same rows as images: psd, sk [max_rows][n/2 + 1] floats in host memory, either (not both) may be NULL */
int psdc_wf_image(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *psd, float *sk, uint64_t *block_index,
                  uint32_t *counts, uint32_t *n_rows);
/* the same with d_psd, d_sk in device memory (min(max_rows, depth) rows each at most; the caller's own work on that memory must
 * have completed); returns when the kernel has completed; block_index and counts are host arrays */
int psdc_wf_image_device(psdc_wf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *d_psd, float *d_sk,
                         uint64_t *block_index, uint32_t *counts, uint32_t *n_rows);
int psdc_wf_stats_read(psdc_wf *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_wf_last_error(const psdc_wf *h);

/* 1 where n is a size the object takes, else 0 (psdc_zsk_supported) */
int psdc_zwf_supported(uint32_t n);
psdc_zwf *psdc_zwf_create(uint32_t n, int window_kind, uint32_t n_channels, uint32_t block, uint32_t depth, int device);
psdc_zwf *psdc_zwf_create_window(uint32_t n, const float *win, float power, float nenbw, size_t overlap, uint32_t n_channels,
                                 uint32_t block, uint32_t depth, int device);
void psdc_zwf_destroy(psdc_zwf *h);
/* as psdc_wf_reset, and the carriers */
int psdc_zwf_reset(psdc_zwf *h);
int psdc_zwf_set_detrend(psdc_zwf *h, int detrend_kind);
/* as psdc_zsk_set_carrier */
int psdc_zwf_set_carrier(psdc_zwf *h, uint32_t channel, uint64_t ftw, uint64_t phase0);
/* as psdc_zsk_process / psdc_zsk_process_device */
int psdc_zwf_process(psdc_zwf *h, uint32_t channel, const float *x, size_t len);
int psdc_zwf_process_device(psdc_zwf *h, uint32_t channel, const float *d_x, size_t len, void *producer_event);
int psdc_zwf_sync(psdc_zwf *h);
int psdc_zwf_num_stages(psdc_zwf *h, uint32_t channel);
int psdc_zwf_stage_blocks(psdc_zwf *h, uint32_t channel, uint32_t stage, psdc_wf_blocks *out);
/* as psdc_wf_stage_rows, the four rows of a slot: [max_rows][n/2 + 1] doubles each, any may be NULL */
int psdc_zwf_stage_rows(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, uint64_t *block_index, uint32_t *counts,
                        double *s1_upper, double *s1_lower, double *s2_upper, double *s2_lower, uint32_t *n_rows);
/* as psdc_wf_image / psdc_wf_image_device; psd, sk: [max_rows][2][n/2 + 1] floats, side 0 upper, side 1 lower */
int psdc_zwf_image(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *psd, float *sk, uint64_t *block_index,
                   uint32_t *counts, uint32_t *n_rows);
int psdc_zwf_image_device(psdc_zwf *h, uint32_t channel, uint32_t stage, uint32_t max_rows, float *d_psd, float *d_sk,
                          uint64_t *block_index, uint32_t *counts, uint32_t *n_rows);
int psdc_zwf_stats_read(psdc_zwf *h, uint64_t *launches, uint64_t *samples_in, int reset);
const char *psdc_zwf_last_error(const psdc_zwf *h);

/* Last error text of a handle; with h == NULL, of the calling thread's last
 * failed psdc_create / handle-less call. */
const char *psdc_last_error(const psdc_handle *h);

int psdc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PSDCASCADE_H */
