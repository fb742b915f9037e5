// frame_scan.h -- which frames of a call are taken and what Loss becomes: the ONE host-side restatement of Frame::from_bytes
// (src/de/frame.rs:25-60), the payloads' size checks (src/de/data.rs:22-25, 91-93, 149-150, 173-174) and Loss::update
// (src/loss.rs:11-26) behind every frames call (frames_ingest.cpp, cross_runtime.cpp).  Host only, no HIP, no handle: where the
// samples go is the callers' business.  tests/host/frame_scan_check.cpp drives it on the CPU.
#ifndef PSDC_FRAME_SCAN_H
#define PSDC_FRAME_SCAN_H

#include "../../include/psdcascade.h"

#include <cstddef>
#include <cstdint>

#include "wire_format.h"

namespace psdrt {

using psdk::WireFmt;

// Where a call's headers are: the 8 header bytes of frame f at hdr + f * stride (host memory).  (frames, frame_size) for frames in
// host memory, (the gathered headers, 8) for frames on the device.
struct HdrView {
    const uint8_t *hdr;
    size_t stride;
    const uint8_t *at(size_t f) const { return hdr + f * stride; }
};

inline bool frame_magic_ok(const uint8_t *p) { return p[0] == 0x7b && p[1] == 0x05; } // Header::parse, src/de/frame.rs:27-29

// The checks every frames call begins with.  PSDC_OK with *go = false: no frames, nothing to do; PSDC_ERR_ARG: null frames;
// PSDC_ERR_FRAME_SIZE: a frame shorter than its header.
constexpr const char *FRAME_SHORT_TEXT = "frame shorter than its header";
inline int check_frames_call(const void *frames, size_t frame_size, size_t n_frames, bool *go)
{
    *go = false;
    if (n_frames == 0)
        return PSDC_OK;
    if (!frames)
        return PSDC_ERR_ARG;
    if (frame_size < 8) // &input[..HEADER_SIZE] panics (src/de/frame.rs:50)
        return PSDC_ERR_FRAME_SIZE;
    *go = true;
    return PSDC_OK;
}

// The format of the run that frame f0 starts: its first frame's (Header::parse, src/de/frame.rs:25-37).  PSDC_ERR_FRAME_HEADER /
// PSDC_ERR_FRAME_FORMAT for a frame that starts none.  adcdac_only: Fls / ThermostatEem / Mpll are PSDC_ERR_FRAME_FORMAT too
// (psdc_process_adcdac_frames).
inline int run_start(const HdrView &v, size_t f0, bool adcdac_only, const WireFmt **wf)
{
    const uint8_t *first = v.at(f0);
    *wf = nullptr;
    if (!frame_magic_ok(first))
        return PSDC_ERR_FRAME_HEADER;
    const WireFmt *w = psdk::wire_fmt(first[2]);
    if (!w || (adcdac_only && w->id != 1))
        return PSDC_ERR_FRAME_FORMAT;
    *wf = w;
    return PSDC_OK;
}

// why scan_piece stopped: one of these or a PSDC_ERR_FRAME_* code (< 0)
constexpr int SCAN_LIMIT = 0;   // every frame of the range was accepted
constexpr int SCAN_RUN_END = 1; // a frame of another (valid) format: the next run starts there

// Frames [f0, f0 + lim) of a run of format wf, `payload` = frame_size - 8 bytes each: the number accepted (from f0 on, up to the
// first that is not) and *stop.  *loss takes Loss::update of the accepted ones.  The checks are the reference's, in its order:
// magic, format id, payload size / batches, then Loss.  adcdac_only: another valid format is PSDC_ERR_FRAME_FORMAT, no run end.
inline size_t scan_piece(const HdrView &v, const WireFmt &wf, size_t payload, size_t f0, size_t lim, bool adcdac_only,
                         psdc_loss *loss, int *stop)
{
    const size_t batch_bytes = (size_t)wf.batch_bytes;
    const bool size_ok = payload % batch_bytes == 0;
    const size_t batches = payload / batch_bytes;
    for (size_t i = 0; i < lim; ++i) {
        const uint8_t *f = v.at(f0 + i);
        if (!frame_magic_ok(f)) {
            *stop = PSDC_ERR_FRAME_HEADER;
            return i;
        }
        if (f[2] != wf.id) { // unknown id (or, adcdac_only, not AdcDac) -- or the next run
            *stop = !adcdac_only && psdk::wire_fmt(f[2]) ? SCAN_RUN_END : PSDC_ERR_FRAME_FORMAT;
            return i;
        }
        if (!size_ok || f[3] != batches) {
            *stop = PSDC_ERR_FRAME_SIZE;
            return i;
        }
        const uint32_t seq = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
        loss->received += f[3];
        if (loss->have_seq)
            loss->dropped += (uint32_t)(seq - loss->next_seq); // wrapping_sub
        loss->next_seq = seq + f[3];                            // wrapping_add
        loss->have_seq = 1;
    }
    *stop = SCAN_LIMIT;
    return lim;
}

// frames from f0 on (a run start: AdcDac) that carry the magic and AdcDac's id, whatever else they say:
// psdc_process_adcdac_frames_device checks such a run, and counts its Loss, on the device
inline size_t adcdac_run_length(const HdrView &v, size_t f0, size_t n_frames)
{
    size_t run = 1;
    while (f0 + run < n_frames && frame_magic_ok(v.at(f0 + run)) && v.at(f0 + run)[2] == 1)
        ++run;
    return run;
}

// de::Error's Display for a PSDC_ERR_FRAME_* code (src/de/mod.rs); callers add their own prefix and suffix
inline const char *frame_error_text(int code, bool adcdac_only = false)
{
    return code == PSDC_ERR_FRAME_HEADER   ? "Invalid frame header"
           : code == PSDC_ERR_FRAME_FORMAT ? (adcdac_only ? "Unknown or non-AdcDac format ID" : "Unknown format ID")
                                           : "Payload size";
}

// *n_ok = the frames ingested, at EVERY exit of a frames call, device errors in mid-call included
struct StoreOk {
    size_t *p;
    const size_t &v;
    ~StoreOk()
    {
        if (p)
            *p = v;
    }
};

} // namespace psdrt

#endif
