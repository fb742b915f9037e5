"""Waterfall cascades on the GPU (psdc_wf_*, psdc_zwf_*; csrc/waterfall_plan.h, csrc/waterfall.hip) against the f64 restatements of
tests/test_waterfall_host.py and their f32 siblings, block by block and stage by stage; against the spectral kurtosis objects,
whose rows a stage's blocks sum to; and the read-out kernel's images against the raw rows.  Semantics: include/psdcascade.h,
"waterfall cascades"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS
from test_sk_host import gaussian
from test_waterfall_host import (TONE_B, TONE_BLOCKS, TONE_N, WF_ROWS, ZWF_ROWS, check_tone_switch, restate_waterfall,
                                 restate_zoom_waterfall, ring_of, tone_input)
from test_zoom_host import emul, mix_f32, windows_of  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, window, detrend, block, depth, the lengths of the calls the stream is fed in).  Hann hops n/2, the rectangular window n.
PARITY_CASES = [
    (64, "hann", "none", 4, 8, (200 * 64,)),             # the ring wraps at stages 0 and 1; a partial newest block at stage 2
    (256, "rect", "mean", 3, 64, (256, 5 * 128, 40_017 - 256 - 5 * 128)),  # B odd: blocks start on odd segments of sk_kernel's pairs
    (1024, "hann", "midpoint", 16, 4, (100 * 1024,)),
    (4096, "hann", "none", 2, 16, (24 * 4096,)),
]
ZOOM_PARITY_CASES = [PARITY_CASES[0], PARITY_CASES[2]]
ZOOM_F0 = 0.23


def feed(g, x, calls, dx=None):
    """x in calls of the given lengths: from host memory, or with dx (a device tensor of x) from device memory"""
    assert sum(calls) == x.size
    for s, e in zip(np.cumsum((0,) + tuple(calls[:-1])), np.cumsum(calls)):
        if dx is None:
            g.process(x[int(s):int(e)])
        else:
            g.process_device(dx.data_ptr() + 4 * int(s), int(e - s))


def all_rows(g):
    return [g.stage_rows(k) for k in range(g.num_stages())]


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.max(np.abs(ref)) + 1e-300)))


def assert_parity(g, st64, st32, block, depth, names, what):
    """stage_rows and stage_blocks of every stage against the restatement's ring: block indices, counts, blocks started and pending
    exact; the S1 rows within 1e-5 and the S2 rows within 2e-5, as the spectral kurtosis objects hold theirs (assert_psd_close with
    the f32 restatement as the yardstick of the widening)"""
    assert g.num_stages() == len(st64)
    nh = len(names) // 2
    for k, (s, s32) in enumerate(zip(st64, st32)):
        info = g.stage_blocks(k)
        ring, ring32 = ring_of(s, depth), ring_of(s32, depth)
        assert info == dict(block=block, depth=depth, started=len(s["blocks"]), rows_valid=len(ring),
                            newest_count=ring[-1]["count"] if ring else 0, pending=s["pending"]), (what, k, info)
        got = g.stage_rows(k)
        assert got[0].tolist() == [b["index"] for b in ring] and got[1].tolist() == [b["count"] for b in ring], (what, k)
        worst = [0.0] * len(names)
        for r, (b, b32) in enumerate(zip(ring, ring32)):
            for i, name in enumerate(names):
                row = got[2 + i][r]
                worst[i] = max(worst[i], rel_err(row, b[name]))
                assert_psd_close(row, b[name], f"{what} stage {k} block {b['index']} {name}", rtol=1e-5 if i < nh else 2e-5,
                                 ref_f32=b32[name])
        print(f"{what} stage {k}: {len(ring)} rows of {len(s['blocks'])} blocks started, newest count {info['newest_count']}; "
              "worst relative error " + " ".join(f"{n_} {w:.3g}" for n_, w in zip(names, worst)))


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_waterfall_parity(pkg, ora, gpu_required, case):
    n, wkind, detrend, block, depth, calls = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    x = gaussian(sum(calls), 3000 + case)
    g = pkg.WaterfallCascade(n, block=block, depth=depth, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    feed(g, x, calls)
    st64 = restate_waterfall(ora, x, n, block, owin, detrend)
    st32 = restate_waterfall(ora, x, n, block, owin, detrend, "f32")
    if case == 0:  # what the case is there for
        assert len(st64[0]["blocks"]) > depth and len(st64[1]["blocks"]) > depth and 0 < st64[2]["blocks"][-1]["count"] < block
    assert_parity(g, st64, st32, block, depth, WF_ROWS, f"waterfall case {case}")


@pytest.mark.parametrize("case", range(len(ZOOM_PARITY_CASES)))
def test_zoom_waterfall_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, block, depth, calls = ZOOM_PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    x = gaussian(sum(calls), 3100 + case)
    ftw = pkg.zoom_ftw(ZOOM_F0)[0]
    g = pkg.ZoomWaterfallCascade(n, ftw=ftw, block=block, depth=depth, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    feed(g, x, calls)
    st64 = restate_zoom_waterfall(ora, x, n, ftw, block, owin, detrend)
    st32 = restate_zoom_waterfall(ora, x, n, ftw, block, owin, detrend, "f32", iq=mix_f32(emul, x, ftw))
    assert_parity(g, st64, st32, block, depth, ZWF_ROWS, f"zoom waterfall case {case}")


def test_more_than_one_job_table_in_a_round(pkg, ora, gpu_required):
    """N = 64, B = 2, K = 512, one call of 64 + 32 * 799 samples: 800 segments and 400 blocks at stage 0, more pieces than a job
    table holds (128), so the round's segment and fold launches are cut in several.  Parity as above; more launches than a steady
    spectral kurtosis round's 3."""
    n, block, depth = 64, 2, 512
    x = gaussian(64 + 32 * 799, 3200)
    g = pkg.WaterfallCascade(n, block=block, depth=depth)
    g.process(x)
    la = g.stats_read()["launches"]
    st64 = restate_waterfall(ora, x, n, block)
    st32 = restate_waterfall(ora, x, n, block, prec="f32")
    assert st64[0]["segs"] == 800 and len(st64[0]["blocks"]) == 400
    assert_parity(g, st64, st32, block, depth, WF_ROWS, "job tables")
    print(f"launches of the one call: {la}")
    assert la > 3
    assert la >= 4 + 4 + 1  # 400 pieces at stage 0 alone: four job tables of segments, four of folds, the decimators


def summed(rows):
    """per stage (sum of the counts, the summed moment rows)"""
    return [(int(r[1].sum()), [m.sum(axis=0) for m in r[2:]]) for r in rows]


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_rows_sum_to_the_sk_object(pkg, gpu_required, zoom):
    """With K larger than the number of blocks a stage's rows sum to SkCascade.stage_moments / ZoomSkCascade.stage_moments on the
    same calls within the siblings' chunking bound (2e-6); the counts sum exactly; as many stages"""
    n, block, depth = 512, 5, 4096
    calls = (1000, 77_777, (1 << 19) + 3)
    x = gaussian(sum(calls), 3300)
    if zoom:
        w = pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth)
        s = pkg.ZoomSkCascade(n, f0=ZOOM_F0)
    else:
        w = pkg.WaterfallCascade(n, block=block, depth=depth)
        s = pkg.SkCascade(n)
    feed(w, x, calls)
    feed(s, x, calls)
    assert w.num_stages() == s.num_stages() >= 4
    worst = 0.0
    for k, (count, rows) in enumerate(summed(all_rows(w))):
        m = s.stage_moments(k)
        assert count == m[0]["count"] and w.stage_blocks(k)["pending"] == m[0]["pending"], k
        assert w.stage_blocks(k)["started"] == -(-count // block) <= depth
        for got, ref in zip(rows, m[1:]):
            if count:
                worst = max(worst, float(np.max(np.abs(got - ref) / ref)))
            assert np.all(np.abs(got - ref) <= 2e-6 * ref), (k, float(np.max(np.abs(got - ref) / np.maximum(ref, 1e-300))))
    print(f"sum of the rows against the {'zoom ' if zoom else ''}SK object: worst relative difference {worst:.3g}")


def same_rows(a, b, tol, what):
    """block indices and counts identical; tol 0: equal bits, else every row within tol"""
    assert len(a) == len(b), what
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra[0].tolist() == rb[0].tolist() and ra[1].tolist() == rb[1].tolist(), (what, k)
        for u, v in zip(ra[2:], rb[2:]):
            if tol == 0:
                assert u.tobytes() == v.tobytes(), (what, k)
            else:
                assert np.all(np.abs(u - v) <= tol * v), (what, k, float(np.max(np.abs(u - v) / np.maximum(v, 1e-300))))


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_cuts_and_routes(pkg, gpu_required, zoom):
    """One call against odd-sized calls, among them calls shorter than a segment and calls ending inside a block: rows within 2e-6,
    block indices and counts identical.  The same calls twice: equal bits.  Host against device: within 2e-6 (the same calls:
    equal bits).  reset and replay: equal bits."""
    import torch
    n, block, depth = 256, 6, 32
    calls = (100, 27, 1000, 129, 33_333, 5, 77_777, 4 * 128 * 6 + 31)  # 100 and 27 and 5 are shorter than a segment
    x = gaussian(sum(calls), 3400)
    make = (lambda: pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth)) if zoom else \
        (lambda: pkg.WaterfallCascade(n, block=block, depth=depth))
    one = make()
    one.process(x)
    ref = all_rows(one)
    assert len(ref) >= 3 and ref[0][0].size == depth and ref[0][0][0] > 0  # the ring has wrapped at stage 0
    a = make()
    feed(a, x, calls)
    got_a = all_rows(a)
    same_rows(got_a, ref, 2e-6, "host chunks")
    a2 = make()
    feed(a2, x, calls)
    same_rows(all_rows(a2), got_a, 0, "the same calls twice")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    d = make()
    feed(d, x, calls, dx)
    got_d = all_rows(d)
    same_rows(got_d, ref, 2e-6, "device chunks")
    same_rows(got_d, got_a, 0, "host against device, the same calls")
    info = [d.stage_blocks(k) for k in range(d.num_stages())]
    d.set_detrend(3)
    d.reset()
    assert d.num_stages() == 0
    feed(d, x, calls, dx)
    same_rows(all_rows(d), got_d, 0, "reset + replay")
    assert [d.stage_blocks(k) for k in range(d.num_stages())] == info
    assert d.stats()["samples_in"] == x.size


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_steady_launches(pkg, gpu_required, zoom):
    """With B larger than the segments of a call a round's pieces fit one job table: a steady device call is exactly 3 kernel launches
    (segments, decimators, fold + tails), and 1 + 3 with the zoom object's mixer -- what the spectral kurtosis objects take."""
    import torch
    n, m = 512, 1 << 20
    dx = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=8192, depth=4) if zoom else pkg.WaterfallCascade(n, block=8192, depth=4)
    s = pkg.ZoomSkCascade(n, f0=ZOOM_F0) if zoom else pkg.SkCascade(n)
    for obj in (g, s):
        for _ in range(12):
            obj.process_device(dx.data_ptr(), m)
        obj.stats(reset=True)
        for _ in range(8):
            obj.process_device(dx.data_ptr(), m)
    la, ls = g.stats()["launches"], s.stats()["launches"]
    g.sync()
    s.sync()
    assert g.num_stages() == s.num_stages() >= 4
    assert la == ls == (4 if zoom else 3) * 8, (la, ls)


def test_a_new_block_overwrites_its_slot(pkg, gpu_required):
    """N = 64, B = 4, K = 4: 4 blocks' worth of NaN samples, then 12 blocks' worth of noise.  Every slot held NaN rows once; a block
    that takes a slot over overwrites it, so every row of stage 0 is finite afterwards (a fold by g_total = 0 would keep the NaN)."""
    n, block, depth = 64, 4, 4
    nan = np.full(4 * block * 32 + 32, np.nan, np.float32)   # segments 0 ... 15: blocks 0 ... 3
    x = gaussian(12 * block * 32, 3500)                      # segments 16 ... 63: blocks 4 ... 15 (block 4 still reads NaN samples)
    g = pkg.WaterfallCascade(n, block=block, depth=depth)
    g.process(nan)
    idx, cnt, s1, s2 = g.stage_rows(0)
    assert idx.tolist() == [0, 1, 2, 3] and cnt.tolist() == [4] * 4 and np.all(np.isnan(s1)) and np.all(np.isnan(s2))
    for s in range(0, x.size, 700):
        g.process(x[s:s + 700])
    idx, cnt, s1, s2 = g.stage_rows(0)
    assert idx.tolist() == [12, 13, 14, 15] and cnt.tolist() == [4] * 4
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2)) and np.all(s1 > 0)
    psd, sk, _, _ = g.image(0)
    assert np.all(np.isfinite(psd)) and np.all(np.isfinite(sk))


def stage_gsc(pkg, n, window, count, stage):
    """the f32 factor the stitch applies to an included stage of that count and decimation: read from pkg.stitch of a row of ones
    (one stage: decimation 1), times 8^-stage (a power of two: exact)"""
    ones = np.ones((1, n // 2 + 1), np.float32)
    out, br = pkg.stitch(n, [count], [0xFFFFFFFF], [0], ones, pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True),
                         window=window)
    assert out.size == n // 2 + 1 and np.all(out == out[0])
    return np.float32(out[0]) * np.float32(8.0 ** -stage)


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_image(pkg, gpu_required, zoom):
    """image() against stage_rows(): psd is np.float32(s1 * float64(gsc)) bit for bit, sk within 1e-6 relative + 1e-6 absolute of
    sk_from_moments with NaNs in the same places (the newest block of stage 1 holds one segment); rows oldest first with the indices
    of stage_rows; image_device into a torch tensor gives the same bits; max_rows below the valid rows returns the newest rows."""
    import torch
    n, block, depth = 256, 3, 16
    # stage 1 of a Hann cascade gets its (3 m + 1)-th segment: its newest block holds exactly one
    length = next(L for L in range(60_000, 70_000, 8) if stage_segments(n, L)[1] % block == 1)
    x = gaussian(length, 3600)
    g = pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth) if zoom else pkg.WaterfallCascade(n, block=block, depth=depth)
    g.process(x)
    sides = 2 if zoom else 1
    assert g.num_stages() >= 3 and g.stage_blocks(1)["newest_count"] == 1 and g.stage_blocks(0)["started"] > depth
    for k in range(g.num_stages()):
        got = g.stage_rows(k)
        idx, cnt = got[0], got[1]
        psd, sk, iidx, icnt = g.image(k)
        assert iidx.tolist() == idx.tolist() and icnt.tolist() == cnt.tolist()
        assert psd.dtype == sk.dtype == np.float32 and psd.shape == sk.shape == ((idx.size, 2, n // 2 + 1) if zoom else (idx.size, n // 2 + 1))
        if idx.size == 0:  # (a stage that holds samples but no segment yet)
            continue
        psd, sk = psd.reshape(idx.size, sides, -1), sk.reshape(idx.size, sides, -1)
        for r in range(idx.size):
            gsc = stage_gsc(pkg, n, pkg.Window.HANN, int(cnt[r]), k)
            for side in range(sides):
                s1, s2 = got[2 + side][r], got[2 + sides + side][r]
                want = (s1 * np.float64(gsc)).astype(np.float32)
                assert psd[r, side].tobytes() == want.tobytes(), (k, r, side)
                ref = pkg.sk_from_moments(int(cnt[r]), s1, s2)
                assert np.array_equal(np.isnan(sk[r, side]), np.isnan(ref)), (k, r, side)
                assert (cnt[r] < 2) == bool(np.all(np.isnan(ref)))
                ok = ~np.isnan(ref)
                assert np.all(np.abs(sk[r, side][ok] - ref[ok]) <= 1e-6 * np.abs(ref[ok]) + 1e-6), (k, r, side)
        # the same images written into a tensor; either output alone; fewer rows: the newest
        shape = (depth, sides, n // 2 + 1)
        tp, ts = torch.full(shape, -1.0, device="cuda"), torch.full(shape, -1.0, device="cuda")
        torch.cuda.synchronize()
        didx, dcnt = g.image_device(k, tp.data_ptr(), ts.data_ptr())
        assert didx.tolist() == idx.tolist() and dcnt.tolist() == cnt.tolist()
        assert tp.cpu().numpy()[:idx.size].tobytes() == psd.tobytes() and ts.cpu().numpy()[:idx.size].tobytes() == sk.tobytes()
        assert np.all(tp.cpu().numpy()[idx.size:] == -1.0)  # nothing behind the rows written
        tp.fill_(-1.0)
        torch.cuda.synchronize()
        g.image_device(k, tp.data_ptr(), None)
        assert tp.cpu().numpy()[:idx.size].tobytes() == psd.tobytes()
        ts.fill_(-1.0)
        torch.cuda.synchronize()
        few = max(1, idx.size // 2)
        fidx, fcnt = g.image_device(k, None, ts.data_ptr(), max_rows=few)
        assert fidx.tolist() == idx[-few:].tolist() and fcnt.tolist() == cnt[-few:].tolist()
        assert ts.cpu().numpy()[:few].tobytes() == sk[-few:].tobytes() and np.all(ts.cpu().numpy()[few:] == -1.0)
        p2, s2_, i2, c2 = g.image(k, max_rows=few)
        assert i2.tolist() == idx[-few:].tolist() and p2.reshape(few, sides, -1).tobytes() == psd[-few:].tobytes()
        r2 = g.stage_rows(k, max_rows=few)
        assert r2[0].tolist() == idx[-few:].tolist() and r2[2].tobytes() == got[2][-few:].tobytes()


def stage_segments(n, length, stages=2, hop=None):
    """segments of the first stages of a Hann cascade fed `length` samples (csrc/plan.h)"""
    hop = hop or n // 2
    out = []
    for _ in range(stages):
        j = 0 if length < n else 1 + (length - n) // hop
        out.append(j)
        p = j * hop + (n - hop) if j else 0
        length = max(0, (p >> 3) - 35)
    return out


def test_recent_psd_of_every_block_is_the_sk_objects_psd(pkg, gpu_required):
    """recent_psd(blocks=None) -- every row of every stage, K larger than the blocks -- against SkCascade.psd() on the same stream:
    equal Breaks, pure 1e-5.  recent_psd(blocks=1) is stitched from the newest block of each stage alone."""
    n, block, depth = 1024, 7, 512
    x = gaussian(1 << 20, 3700)
    w = pkg.WaterfallCascade(n, block=block, depth=depth)
    w.process(x)
    s = pkg.SkCascade(n)
    s.process(x)
    psd, br = w.recent_psd(blocks=None)
    ref, rbr = s.psd()
    assert br == rbr and w.num_stages() == s.num_stages() >= 4
    rel = assert_psd_close(psd, ref, "recent_psd of every block against SkCascade.psd()", pure=True)
    print(f"recent_psd(all) against SkCascade.psd(): worst relative error {rel:.3g}")
    one, obr = w.recent_psd(blocks=1)
    assert [b.count for b in obr] == [w.stage_blocks(k)["newest_count"] for k in reversed(range(w.num_stages()))]
    z = pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth)
    z.process(x)
    zs = pkg.ZoomSkCascade(n, f0=ZOOM_F0)
    zs.process(x)
    up, lo, zbr = z.recent_psd(blocks=None)
    rup, rlo, rzbr = zs.psd()
    assert zbr == rzbr
    assert_psd_close(up, rup, "zoom recent_psd upper", pure=True)
    assert_psd_close(lo, rlo, "zoom recent_psd lower", pure=True)


def test_tone_switch(pkg, ora, gpu_required):
    """the property tests/test_waterfall_host.py shows on the f64 restatement, on the GPU's rows: a tone that moves from bin 10 to
    bin 20 half-way is at its half's bin in every block wholly inside one half; at most 2 blocks touch the switch"""
    x, half = tone_input()
    g = pkg.WaterfallCascade(TONE_N, block=TONE_B, depth=64)
    for s in range(0, x.size, 5000):
        g.process(x[s:s + 5000])
    idx, cnt, s1, _ = g.stage_rows(0)
    assert idx.tolist() == list(range(TONE_BLOCKS)) and cnt.tolist() == [TONE_B] * TONE_BLOCKS
    check_tone_switch(pkg, idx, s1, half, x.size)
    psd, _, _, _ = g.image(0)
    assert np.argmax(psd, axis=1).tolist() == np.argmax(s1, axis=1).tolist()  # the image shows the same
    for b in (0, 7):
        assert g.block_span(0, b) == pkg.waterfall_block_span(TONE_N, TONE_N // 2, TONE_B, 0, b)


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_argument_errors_on_an_object(pkg, gpu_required, zoom):
    """a stage and a channel out of range, null outputs, Detrend::Linear, a carrier after the first sample"""
    import ctypes as C
    L = pkg.lib()
    tag = "psdc_zwf_" if zoom else "psdc_wf_"
    f = lambda name: getattr(L, tag + name)  # noqa: E731
    b = (pkg.ZoomWaterfallCascadeBank if zoom else pkg.WaterfallCascadeBank)(256, 2, block=4, depth=4)
    with pytest.raises(pkg.PsdError) as e:
        b.stage_blocks(0, 0)  # no sample yet: no stage
    assert e.value.code == pkg.ERR_ARG and tag + "stage_blocks: stage 0 out of range" in str(e.value)
    b.process(0, gaussian(5000, 1))
    ns = b.num_stages(0)
    for call in (lambda: b.stage_blocks(0, ns), lambda: b.stage_rows(0, ns), lambda: b.image(0, ns), lambda: b.image_device(0, ns, 8, 8)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and f"stage {ns} out of range" in str(e.value)
    for call in (lambda: b.process(2, np.zeros(9, np.float32)), lambda: b.num_stages(2), lambda: b.stage_blocks(2, 0),
                 lambda: b.stage_rows(5, 0), lambda: b.image(2, 0)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "out of range (n_channels 2)" in str(e.value)
    idx, cnt, nr = (C.c_uint64 * 4)(), (C.c_uint32 * 4)(), C.c_uint32()
    img = np.zeros((4, 2, 129), np.float32)
    assert f("image")(b._h, 0, 0, 4, None, None, idx, cnt, C.byref(nr)) == pkg.ERR_ARG
    assert tag + "image: null output" in f("last_error")(b._h).decode()
    assert f("image_device")(b._h, 0, 0, 4, None, None, idx, cnt, C.byref(nr)) == pkg.ERR_ARG
    assert f("image")(b._h, 0, 0, 4, pkg._fptr(img), None, None, cnt, C.byref(nr)) == pkg.ERR_ARG
    assert f("image")(b._h, 0, 0, 4, pkg._fptr(img), None, idx, cnt, None) == pkg.ERR_ARG
    assert f("stage_blocks")(b._h, 0, 0, None) == pkg.ERR_ARG
    assert tag + "stage_blocks: null output" in f("last_error")(b._h).decode()
    assert f("process")(b._h, 0, None, 4) == pkg.ERR_ARG and "null sample pointer" in f("last_error")(b._h).decode()
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED
    if zoom:
        with pytest.raises(pkg.PsdError) as e:
            b.set_carrier(0, f0=0.1)
        assert e.value.code == pkg.ERR_ARG and "has taken" in str(e.value)
        b.set_carrier(1, f0=0.1)
    # a read-out of no rows writes nothing
    p, s, i, c = b.image(0, 0, max_rows=0)
    assert p.shape[0] == s.shape[0] == i.size == c.size == 0
    b.close()


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_waterfall_cli(pkg, gpu_required, tmp_path, zoom):
    """tools/psd_cli.py --raw FILE --waterfall B:K / --zoom-waterfall F0:B:K with --csv DIR: one file a stage, rows = blocks, columns
    = bins, a header line with the block indices and counts; the values are image()'s (one call here: the file is shorter than the
    tool's 2^20 samples a call)"""
    n, block, depth = 512, 8, 16
    length = (1 << 17) + 777
    x = (gaussian(length, 41) + 30.0 * np.cos(2 * np.pi * 0.2001 * np.arange(length))).astype(np.float32)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    opt = ["--zoom-waterfall", f"{ZOOM_F0}:{block}:{depth}"] if zoom else ["--waterfall", f"{block}:{depth}"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--raw", str(raw), *opt, "--csv", str(tmp_path / "csv")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    g = pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth) if zoom else pkg.WaterfallCascade(n, block=block, depth=depth)
    g.set_detrend(pkg.Detrend.MEAN)  # the tool's default AcqOpts
    g.process(x)
    label = f"zoom_waterfall raw @ {g.f0:.12g}" if zoom else "waterfall raw"
    stem = "".join(ch if ch.isalnum() else "_" for ch in (f"zoom_waterfall_raw_{g.f0:.9g}" if zoom else "waterfall_raw"))
    assert f"{label}: {g.num_stages()} stages, block {block} depth {depth}" in r.stdout, r.stdout
    assert g.num_stages() >= 3 and g.stage_blocks(0)["started"] > depth
    for k in range(g.num_stages()):
        psd, sk, idx, cnt = g.image(k)
        path = tmp_path / "csv" / f"{stem}_stage{k}.csv"
        head = open(path).readline()
        assert head.startswith(f"# stage {k}: blocks {' '.join(map(str, idx.tolist()))}; counts {' '.join(map(str, cnt.tolist()))};"), head
        if idx.size == 0:
            assert len(open(path).readlines()) == 1
            continue
        d = np.loadtxt(path, delimiter=",", ndmin=2)
        want = np.concatenate([psd.reshape(idx.size, -1), sk.reshape(idx.size, -1)], axis=1)  # one line a block: psd then sk
        assert d.shape == want.shape
        assert np.array_equal(np.isnan(d), np.isnan(want)) and np.allclose(d, want, rtol=2e-6, atol=0, equal_nan=True), k
