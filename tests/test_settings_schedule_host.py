"""What makes the scheduled restatements (the schedule= argument of the nine restate functions) and the walks of
tests/test_gpu_settings_midstream.py trustworthy, without a GPU: the closed form of the segment counts and the schedule logic are
held to the C oracle's PsdCascade, which implements mid-stream set_detrend / set_avg itself (src/psd.rs:431-443); a one-epoch
schedule gives the bytes of the unscheduled call; and every walk the GPU file runs meets the conditions that make it a test."""
import numpy as np
import pytest

from settings_schedule import (DETRENDS, KINDS, UNITS, WALKS, WF_BLOCK, WF_DEPTH, Schedule, make_walk, pending_after, segments_after,
                               stage_avg, unit_events)
from test_cross_host import U32_MAX, restate
from test_gpu_cross import window_of
from test_sk_host import restate_sk
from test_waterfall_host import restate_waterfall, restate_zoom_waterfall
from test_zoom_ampm_cross_host import restate_zoom_ampm_cross
from test_zoom_ampm_host import restate_zoom_ampm
from test_zoom_cross_host import restate_zoom_cross
from test_zoom_host import noise, restate_zoom, stitch_zoom
from test_zoom_sk_host import restate_zoom_sk

FTW = int(0.2345678901234567 * 2.0 ** 64)  # cycles a sample in 2^-64 turn: off every bin grid


def overlap_of(n, wkind):
    return {"hann": n // 2, "rect": 0, "custom": n // 4}[wkind]


def random_cuts(rng, n, total):
    cuts = []
    while sum(cuts) < total:
        cuts.append(int(rng.choice([rng.integers(1, 50), rng.integers(1, 6 * n), rng.integers(6 * n, 40 * n)])))
    return cuts


@pytest.mark.parametrize("wkind", ["hann", "rect", "custom"])
@pytest.mark.parametrize("n", [64, 256, 1024])
def test_segments_after_is_the_oracle(pkg, ora, n, wkind):
    """segments_after / pending_after against ora.PsdCascade fed the same calls, after every call: stages, counts (unlimited
    averaging, so that a count is the number of segments) and pendings equal; the stream reaches stage 3."""
    rng = np.random.default_rng(n + len(wkind))
    _, owin = window_of(pkg, n, wkind)
    ref = ora.PsdCascade(n, "f64", window=owin)
    x = noise((600 if n == 64 else 300) * n, n)  # (a stage of N = 64 takes eight segments to fill the next one's drain, of 256 two)
    taken = 0
    for c in random_cuts(rng, n, x.size - 40 * n):
        ref.process(x[taken:taken + c])
        taken += c
        segs, pend = segments_after(n, overlap_of(n, wkind), taken), pending_after(n, overlap_of(n, wkind), taken)
        assert ref.num_stages == len(segs), taken
        for k in range(len(segs)):
            info = ref.stage_info(k)
            assert (info["count"], info["pending"]) == (segs[k], pend[k]), (taken, k)
    assert len(segs) >= 4


def same_bytes(a, b, what=""):
    """two restatement results (lists of dicts of scalars, arrays and lists of such dicts): equal, arrays by their bytes"""
    assert type(a) is type(b), what
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (u, v) in enumerate(zip(a, b)):
            same_bytes(u, v, f"{what}[{i}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for key in a:
            same_bytes(a[key], b[key], f"{what}.{key}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert a == b, what


def nine(ora, n, x, y, window, prec, **kw):
    """the nine restatements on one input, with the keyword arguments given to each that takes them"""
    nw = {k: v for k, v in kw.items() if k != "avg"}  # the waterfalls have no set_avg
    return {
        "restate": restate(ora, x, y, n, window, prec=prec, **kw),
        "restate_zoom": restate_zoom(ora, x, n, FTW, 0, window, prec=prec, **kw),
        "restate_zoom_cross": restate_zoom_cross(ora, x, y, n, (FTW, FTW // 3), (0, 0), window, prec=prec, **kw),
        "restate_sk": restate_sk(ora, x, n, window, prec=prec, **kw),
        "restate_zoom_sk": restate_zoom_sk(ora, x, n, FTW, 0, window, prec=prec, **kw),
        "restate_zoom_ampm": restate_zoom_ampm(ora, x, n, FTW, 0, window, prec=prec, **kw),
        "restate_zoom_ampm_cross": restate_zoom_ampm_cross(ora, x, y, n, (FTW, FTW // 3), (0, 0), window, prec=prec, **kw),
        "restate_waterfall": restate_waterfall(ora, x, n, 3, window, prec=prec, **nw),
        "restate_zoom_waterfall": restate_zoom_waterfall(ora, x, n, FTW, 3, window, prec=prec, **nw),
    }


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("wkind,detrend,avg", [("hann", "span", (7, 100)), ("custom", "mean", (U32_MAX, U32_MAX))])
def test_one_epoch_schedule_gives_the_unscheduled_bytes(pkg, ora, wkind, detrend, avg, prec):
    """Each of the nine restatements under a schedule of one epoch -- without events, and with one event before the first sample --
    against the unscheduled call with that epoch's settings: every array of every stage bit for bit."""
    n = 64
    _, owin = window_of(pkg, n, wkind)
    x, y = noise(90 * n, 5), noise(90 * n, 6)
    plain = nine(ora, n, x, y, owin, prec, detrend=detrend, avg=avg)
    assert len(plain) == 9 and all(len(st) >= 3 for st in plain.values())
    ov = overlap_of(n, wkind)
    for sched in (Schedule(n, ov, [], detrend, avg), Schedule(n, ov, [(0, detrend, None), (0, None, avg)])):
        for name, got in nine(ora, n, x, y, owin, prec, schedule=sched).items():
            same_bytes(got, plain[name], name)


def random_schedule(rng, n, total):
    """[("feed", length) | ("detrend", name) | ("avg", limit, count)]: random set_detrend / set_avg between random calls"""
    taken = int(rng.integers(n, 6 * n))  # a first change while only the first stages exist
    ops = [("feed", taken), ("detrend", DETRENDS[int(rng.integers(1, 4))])]
    while taken < total:
        r = rng.random()
        if r < 0.15:
            ops.append(("detrend", DETRENDS[int(rng.integers(4))]))
        elif r < 0.3:
            ops.append(("avg", int(rng.integers(1, 50)), int(rng.integers(1, 400))))
        else:
            c = int(rng.choice([rng.integers(1, 50), rng.integers(1, 6 * n), rng.integers(6 * n, 40 * n)]))
            ops.append(("feed", c))
            taken += c
    return ops, taken


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n,wkind", [(64, "hann"), (64, "rect"), (256, "custom"), (128, "hann")])
def test_random_schedule_is_the_oracle_cascade(pkg, ora, n, wkind, seed):
    """Random set_detrend / set_avg between random calls, given to ora.PsdCascade f64 as calls and to the restatements as a
    Schedule: stages, counts and pendings equal, and the rows that are the auto-PSD of one real stream the oracle's -- sxx / syy
    of restate and S1 of restate_sk to 1e-12 (the bound of test_restatement_sxx_is_the_oracle), upper / lower of restate_zoom with
    ftw = 0 to 1e-9 and its stitched rows to 2e-7 (the bounds of test_restatement_ftw0_is_the_oracle_cascade).  The deeper stages
    are created after the first changes, so the settings a lazily created stage starts with are part of this."""
    rng = np.random.default_rng(1000 * n + seed)
    pwin, owin = window_of(pkg, n, wkind)
    ops, total = random_schedule(rng, n, 200 * n)
    x, y = noise(total, 7 * n + seed), noise(total, 9 * n + seed)
    refs = [ora.PsdCascade(n, "f64", window=owin) for _ in range(2)]
    events, taken = [], 0
    for op in ops:
        if op[0] == "feed":
            for r, v in zip(refs, (x, y)):
                r.process(v[taken:taken + op[1]])
            taken += op[1]
        elif op[0] == "detrend":
            events.append((taken, op[1], None))
            for r in refs:
                r.set_detrend(op[1])
        else:
            events.append((taken, None, op[1:]))
            for r in refs:
                r.set_avg(*op[1:])
    assert len(events) >= 3 and len(segments_after(n, overlap_of(n, wkind), events[0][0])) < refs[0].num_stages
    sched = Schedule(n, overlap_of(n, wkind), events)
    detrended = any(d != "none" for d, _ in sched.epochs)
    cross = restate(ora, x, y, n, owin, schedule=sched)
    sk = restate_sk(ora, x, n, owin, schedule=sched)
    zoom = restate_zoom(ora, x, n, 0, 0, owin, schedule=sched)
    for name, st in (("restate", cross), ("restate_sk", sk), ("restate_zoom", zoom)):
        assert refs[0].num_stages == len(st), name
        for k, s in enumerate(st):
            info = refs[0].stage_info(k)
            assert (info["count"], info["avg"], info["pending"]) == (s["count"], s["avg"], s["pending"]), (name, k)
    for k in range(refs[0].num_stages):
        rx, ry = refs[0].stage_spectrum(k), refs[1].stage_spectrum(k)
        for name, got, r in (("sxx", cross[k]["sxx"], rx), ("syy", cross[k]["syy"], ry), ("s1", sk[k]["s1"], rx)):
            assert np.max(np.abs(got - r) / np.maximum(r, 1e-300)) <= 1e-12, (name, k)
        floor = 1e-9 * np.mean(rx) if detrended else 0.0
        for row in ("upper", "lower"):
            assert np.all(np.abs(zoom[k][row] - rx) <= 1e-9 * rx + floor), (row, k)
    p, rbr, _ = refs[0].psd()
    up, lo, br = stitch_zoom(pkg, n, pwin, zoom)
    assert len(br) == len(rbr) and up.shape == p.shape
    for b, r in zip(br, rbr):
        assert (b.count, b.avg, b.pending, b.bins.start, b.bins.stop, b.start) == (
            r["count"], r["avg"], r["pending"], r["bins_start"], r["bins_end"], r["start"]), (b, r)
    floor = 1e-6 * np.mean(p) if detrended else 0.0
    for row in (up, lo):
        assert np.all(np.abs(row - p) <= 2e-7 * p + floor)


def counts_of(sched, k, nseg):
    """the count of stage k after each of its first nseg segments under the schedule (the reference's rule, src/psd.rs:218-224)"""
    out, count = [], 0
    for j in range(nseg):
        a = sched.stage(k, j)[1]
        if count > a:
            count = a
        count += 1
        out.append(count)
    return out


@pytest.mark.parametrize("kind,n,seed,wkind", WALKS)
def test_walk_properties(kind, n, seed, wkind):
    """The conditions a walk has to meet, from make_walk alone.  A seed that misses one is replaced; no condition is loosened."""
    walk = make_walk(kind, n, seed, wkind)
    assert walk == make_walk(kind, n, seed, wkind)  # a pure function of its arguments
    has_avg, is_iq = KINDS[kind]
    ov = overlap_of(n, wkind)
    changes = [i for i, op in enumerate(walk) if op[0] in ("detrend", "avg")]
    # at least three detrend changes, none and mean among the kinds segments ran under; at least three avg changes
    assert sum(op[0] == "detrend" for op in walk) >= 3
    assert sum(op[0] == "avg" for op in walk) >= (3 if has_avg else 0) and (has_avg or not any(op[0] == "avg" for op in walk))
    assert all(op[1] in DETRENDS for op in walk if op[0] == "detrend")
    assert all(1 <= op[1] <= 50 and 1 <= op[2] <= 400 for op in walk if op[0] == "avg")
    # changes directly behind a device call and behind a host call, nothing in between
    assert {walk[i - 1][0] for i in changes if walk[i][0] == "detrend"} == {"host", "device"}
    assert not has_avg or {walk[i - 1][0] for i in changes if walk[i][0] == "avg"} == {"host", "device"}
    # both routes, odd device offsets, mid-stream read-outs between and behind the changes; the complex kinds alternate their layouts
    feeds = [op for op in walk if op[0] in ("host", "device")]
    assert {op[0] for op in feeds} == {"host", "device"} and all(op[4] % 2 == 1 for op in feeds if op[0] == "device")
    reads = [i for i, op in enumerate(walk) if op[0] == "read"]
    assert len(reads) >= 3 and reads[0] < changes[1] and changes[1] < reads[1] < changes[-1] < reads[-1] < len(walk) - 1
    if is_iq:
        assert all(a[3] != b[3] for a, b in zip(feeds, feeds[1:])) and {op[3] for op in feeds} == {"planar", "interleaved"}
        assert {(op[0], op[3]) for op in feeds} == {(r, lay) for r in ("host", "device") for lay in ("planar", "interleaved")}
    else:
        assert all(op[3] is None for op in feeds)
    per_unit = [unit_events(walk, u) for u in range(UNITS)]
    assert per_unit[0][1] != per_unit[1][1] and [e[0] for e in per_unit[0][0]] != [e[0] for e in per_unit[1][0]]  # fed unevenly
    for events, total in per_unit:
        sched = Schedule(n, ov, events)
        at = [segments_after(n, ov, e[0]) + [0] * 8 for e in events]
        end = segments_after(n, ov, total)
        assert {"none", "mean"} <= sched.detrends_of_stage(0, end[0])
        # at least two changes with a stage-0 and a stage-1 segment completing before the next change
        assert sum(b[0] > a[0] and b[1] > a[1] for a, b in zip(at, at[1:])) >= 2
        # a change while the unit holds a partial segment
        assert any(pending_after(n, ov, e[0])[0] > ov for e in events if e[0] >= n)  # (beyond the overlap a full stage keeps)
        # four stage-2 segments after the last change
        assert end[2] - at[-1][2] >= 4
        # a stage created after a change
        assert len(end) > len(segments_after(n, ov, events[0][0]))
        if has_avg:  # a limit that drops below the count stage 0 has at that moment, and one that rises
            c0 = counts_of(sched, 0, end[0])
            lowered = raised = False
            prev = U32_MAX
            for e, a in zip(events, at):
                if e[2] is None:
                    continue
                new = stage_avg(e[2], 0)
                lowered |= a[0] > 0 and new < c0[a[0] - 1]
                raised |= new > prev
                prev = new
            assert lowered and raised
        else:  # the waterfalls: a block that straddles a detrend change, and rings that wrap at stages 0 and 1
            assert any(a[0] % WF_BLOCK for a in at) and any(a[1] % WF_BLOCK for a in at)
            assert end[0] > WF_BLOCK * WF_DEPTH and end[1] > WF_BLOCK * WF_DEPTH
