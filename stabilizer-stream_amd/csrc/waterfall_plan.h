// waterfall_plan.h -- the piece cut of the waterfall cascades (psdc_wf_*, psdc_zwf_*; include/psdcascade.h, "waterfall cascades").
// A stage's segments are grouped into blocks of B: block b is the segments [b B, (b + 1) B) and lives in slot b mod K of the
// stage's ring of K row sets.  A round's span of new segments [s0, s1) is cut at the block boundaries into pieces; each piece is
// one job of the segment kernel and one fold into its slot, and the piece that holds a block's first segment overwrites the
// slot (`fresh`) where the others add to it.  Pure host code, no HIP: tests/host/waterfall_plan_check.cpp checks it exhaustively.
#pragma once
#include <algorithm>
#include <cstdint>

namespace psdk {

struct WfPiece {
    uint64_t seg0; // absolute index of the piece's first segment
    uint32_t nseg; // 1 ... B segments, all of one block
    uint32_t slot; // (seg0 / B) mod K
    bool fresh;    // the piece holds its block's first segment: the fold overwrites the slot
};

// the pieces of [s0, s1) in segment order; emit(const WfPiece &); B >= 1, K >= 1
template <class Emit>
inline void wf_cut(uint64_t s0, uint64_t s1, uint32_t B, uint32_t K, Emit &&emit)
{
    while (s0 < s1) {
        const uint64_t b = s0 / B;
        const uint64_t end = std::min<uint64_t>(s1, (b + 1) * (uint64_t)B);
        emit(WfPiece{s0, (uint32_t)(end - s0), (uint32_t)(b % K), s0 == b * (uint64_t)B});
        s0 = end;
    }
}

// blocks started once `segs` segments are folded, and how many of them the newest holds (0 before the first segment)
inline uint64_t wf_blocks_started(uint64_t segs, uint32_t B) { return (segs + B - 1) / B; }
inline uint32_t wf_newest_count(uint64_t segs, uint32_t B) { return segs ? (uint32_t)(segs - (wf_blocks_started(segs, B) - 1) * B) : 0; }

} // namespace psdk
