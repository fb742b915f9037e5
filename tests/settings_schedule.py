"""Mid-stream set_detrend / set_avg for the restatements of the cross-runtime objects (a plain helper module, no tests of its own).

The reference's semantics (src/psd.rs:431-443; include/psdcascade.h, cross section): samples fed before a call are analysed with
the old setting.  Settings change only between process calls, so which setting a segment sees is decided by one number, the
samples its unit had taken when the change was made: segment j of stage k belongs to the epoch in which the unit's count of
completed stage-k segments first exceeded j.  segments_after is that count in closed form, Schedule the map (k, j) -> settings,
and make_walk the list of operations one GPU walk of tests/test_gpu_settings_midstream.py performs.  All three are anchored in
tests/test_settings_schedule_host.py: segments_after and the scheduled restatements to the C oracle, which implements mid-stream
changes itself, and the walks to the conditions that make them worth running."""
import numpy as np

U32_MAX = 0xFFFFFFFF
DRAIN = 35
DETRENDS = ("none", "midpoint", "span", "mean")

# kind: (has set_avg, streams are complex already); one entry per kind of csrc/cross_runtime.cpp's table
KINDS = {
    "cross": (True, False), "csm": (True, False), "zoom": (True, False), "zcsd": (True, False), "iq": (True, True),
    "iqcsd": (True, True), "sk": (True, False), "zsk": (True, False), "iqsk": (True, True), "zampm": (True, False),
    "iqampm": (True, True), "zxampm": (True, False), "iqxampm": (True, True), "wf": (False, False), "zwf": (False, False),
}
UNITS = 2
WF_BLOCK, WF_DEPTH = 4, 8  # small, so that blocks straddle the changes and the ring wraps

# (kind, n, seed, window) of every GPU walk: every kind at N = 64 and at N = 2048, Hann but for one rectangular walk a size.
# A seed is only ever changed to meet the conditions of test_walk_properties, never to make a comparison pass.
WALKS = [(kind, n, 100 * i + (1 if n == 64 else 2), "rect" if (kind, n) in (("zcsd", 64), ("sk", 2048)) else "hann")
         for i, kind in enumerate(KINDS) for n in (64, 2048)]


def _stages(n, overlap, length):
    """[(completed segments, pending samples)] per stage of a unit that has taken `length` samples: what the restatements embody.
    A stage hands the decimator the samples its completed segments cover; the next stage gets an eighth of them less the
    one-time drain."""
    hop = n - overlap
    out = []
    size = length
    while size > 0:
        nseg = 0 if size < n else 1 + (size - n) // hop
        out.append((nseg, size if nseg == 0 else size - nseg * hop))
        p = nseg * hop + overlap if nseg else 0
        size = max(0, p // 8 - DRAIN)
    return out


def segments_after(n, overlap, length):
    """the number of completed segments of every stage, stage 0 first, once a unit has taken `length` samples"""
    return [s for s, _ in _stages(n, overlap, length)]


def pending_after(n, overlap, length):
    """the pending samples of every stage at that moment"""
    return [p for _, p in _stages(n, overlap, length)]


def stage_avg(avg, k):
    """PsdCascade's averaging limit of stage k: min(count >> 3k, limit) of avg = (limit, count)"""
    sh = 3 * k
    return min((avg[1] >> sh) if sh < 32 else 0, avg[0])


class Schedule:
    """events: [(samples the unit had taken when the change was made, detrend or None, avg (limit, count) or None)] in call order;
    detrend, avg: the settings before the first event.  schedule(k, j) -> (detrend, avg) of segment j of stage k."""

    def __init__(self, n, overlap, events, detrend="none", avg=(U32_MAX, U32_MAX)):
        self.epochs = [(detrend, tuple(avg))]
        self.done = []  # per event: the segments every stage had completed
        for taken, d, a in events:
            pd, pa = self.epochs[-1]
            self.epochs.append((pd if d is None else d, pa if a is None else tuple(a)))
            self.done.append(segments_after(n, overlap, taken))
        assert all(u[0] <= v[0] for u, v in zip(self.done, self.done[1:]) if u and v)

    def epoch(self, k, j):
        e = 0
        for i, segs in enumerate(self.done):  # (monotonic: a later event never has fewer segments)
            if (segs[k] if k < len(segs) else 0) > j:
                break
            e = i + 1
        return e

    def __call__(self, k, j):
        return self.epochs[self.epoch(k, j)]

    def stage(self, k, j):
        """(detrend, averaging limit of stage k) of segment j of stage k"""
        d, a = self(k, j)
        return d, stage_avg(a, k)

    def final_avg(self, k):
        return stage_avg(self.epochs[-1][1], k)

    def detrends_of_stage(self, k, nseg):
        """the detrend kinds segments 0 ... nseg - 1 of stage k ran under"""
        return {self(k, j)[0] for j in range(nseg)}


# ---- the walks ----

def _cut(rng, n):
    """a cut as test_randomized_feed_stress draws it: a few samples, up to 6 N, or 6 N to 40 N"""
    c = int(rng.integers(3))
    if c == 0:
        return int(rng.integers(1, 8))
    if c == 1:
        return int(rng.integers(8, 6 * n + 1))
    return int(rng.integers(6 * n, 40 * n + 1))


def make_walk(kind, n, seed, window="hann"):
    """The operations of one walk over a bank of UNITS units, a pure function of its arguments:
      ("host", unit, length, layout) / ("device", unit, length, layout, offset): a process call; layout "planar" / "interleaved"
          for the kinds whose streams are complex (they alternate), None otherwise; offset: the odd number of elements the
          device pointer lies behind an allocation's start;
      ("detrend", name); ("avg", limit, count); ("read", unit): a mid-stream read-out of one unit.
    The units are fed unevenly; every walk ends with a stretch without changes long enough for four stage-2 segments."""
    has_avg, is_iq = KINDS[kind]
    rng = np.random.default_rng([seed, n, list(KINDS).index(kind)])
    hop = n // 2 if window == "hann" else n
    ops = []
    nfeed = [0]

    def feed(unit, length, device=None):
        layout = ("planar", "interleaved")[nfeed[0] % 2] if is_iq else None
        nfeed[0] += 1
        if device is None:
            device = bool(rng.integers(2))
        ops.append(("device", unit, length, layout, int(rng.choice([1, 3, 5, 7]))) if device else ("host", unit, length, layout))

    def stretch(unit, least, last_device=None):
        """random cuts to `unit` until it has taken `least` more samples, one of them 20 N or more (a stage-1 segment at least)"""
        cuts = [int(rng.integers(20 * n, 40 * n + 1))] if least >= 20 * n else []
        got = sum(cuts)
        while got < least:
            cuts.append(_cut(rng, n))
            got += cuts[-1]
        for i in rng.permutation(len(cuts)):
            feed(unit, cuts[int(i)])
        if last_device is not None:  # a last small cut by the route asked for: it leaves a partial segment behind
            feed(unit, int(rng.integers(1, hop)), device=last_device)

    # warm-up: short, so that the deeper stages are created after the first change
    stretch(0, 12 * n)
    stretch(1, 7 * n)
    changes = ["detrend", "avg"] * 3 if has_avg else ["detrend"] * 4
    # the detrend kinds in turn: the stream starts under none, mean is always among them, no kind follows itself
    picks = [str(d) for d in rng.permutation(["mean", "midpoint", "span"])]
    spot = int(rng.integers(1, 4))
    if not has_avg:
        picks.insert(spot, "none")
    elif spot < 3 and picks[spot] != "mean":
        picks[spot] = "none"
    navg = 0
    for r, what in enumerate(changes):
        if r:
            stretch(int(r % 2), 22 * n)
            if r == 3:
                ops.append(("read", int(rng.integers(UNITS))))
            # (the route of the last call alternates in pairs, so that either kind of change follows either route)
            stretch(int(1 - r % 2), 22 * n + int(rng.integers(0, 9 * n)), last_device=bool((r // 2 + r) % 2))
        else:
            feed(0, int(rng.integers(1, hop)), device=True)  # the first change follows a device call directly
        if what == "detrend":
            ops.append(("detrend", picks.pop(0)))
        else:
            if navg == 0:    # below the count stage 0 has by now
                avg = (int(rng.integers(3, 11)), int(rng.integers(1, 401)))
            elif navg == 1:  # and up again
                avg = (int(rng.integers(30, 51)), int(rng.integers(200, 401)))
            else:
                avg = (int(rng.integers(1, 51)), int(rng.integers(1, 401)))
            navg += 1
            ops.append(("avg",) + avg)
        if r == 0:  # a read-out directly behind the first change
            ops.append(("read", int(rng.integers(UNITS))))
    # the tail: four stage-2 segments (64 hops of stage 0 each) and more for both units, a read-out in between
    stretch(0, 2 * 64 * hop)
    stretch(1, 3 * 64 * hop)
    ops.append(("read", 1))
    stretch(0, 3 * 64 * hop + int(rng.integers(0, 5 * n)))
    stretch(1, 2 * 64 * hop + int(rng.integers(0, 5 * n)))
    return ops


def unit_events(walk, unit):
    """(events for Schedule, samples taken in all) of one unit of a walk"""
    taken = 0
    events = []
    for op in walk:
        if op[0] in ("host", "device") and op[1] == unit:
            taken += op[2]
        elif op[0] == "detrend":
            events.append((taken, op[1], None))
        elif op[0] == "avg":
            events.append((taken, None, (op[1], op[2])))
    return events, taken
