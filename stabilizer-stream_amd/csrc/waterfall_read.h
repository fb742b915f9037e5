// waterfall_read.h -- what wf_image_kernel (waterfall.hip) computes for one element, and the map from an oldest-first row of a
// read-out to its ring slot.  Host and device: tests/host/waterfall_emul.cpp runs these on the CPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSDK_WF_HD __host__ __device__
#else
#define PSDK_WF_HD
#endif

namespace psdk {

// rows the ring holds: the newest min(K, blocks started) blocks
PSDK_WF_HD inline uint32_t wf_valid_rows(uint64_t started, uint32_t K) { return started < K ? (uint32_t)started : K; }

// Row r of a read-out of nr <= wf_valid_rows rows, oldest first, is block started - nr + r, which lives in slot block mod K:
// before the ring wraps (started <= K) that is the block index itself, afterwards the slots are taken from the oldest on.
PSDK_WF_HD inline uint64_t wf_row_block(uint64_t started, uint32_t nr, uint32_t r) { return started - nr + r; }
PSDK_WF_HD inline uint32_t wf_row_slot(uint64_t started, uint32_t K, uint32_t nr, uint32_t r)
{
    return (uint32_t)(wf_row_block(started, nr, r) % K);
}

// psd = float32(S1 * (double)gsc): one f64 multiply, one rounding; gsc is the f32 factor the stitch applies to a stage of that
// count and decimation
PSDK_WF_HD inline float wf_psd(double s1, float gsc) { return (float)(s1 * (double)gsc); }

// the estimator of include/psdcascade.h ("spectral kurtosis cascade") in f64: NaN below two segments and without power
PSDK_WF_HD inline double wf_sk_f64(uint32_t count, double s1, double s2)
{
    if (count < 2 || s1 == 0.0)
        return __builtin_nan("");
    const double m = (double)count;
    return (m + 1.0) / (m - 1.0) * (m * s2 / (s1 * s1) - 1.0);
}
// ... rounded once (the image's element; the robust read-out of waterfall_robust.h compares the f64 value)
PSDK_WF_HD inline float wf_sk(uint32_t count, double s1, double s2) { return (float)wf_sk_f64(count, s1, s2); }

} // namespace psdk
