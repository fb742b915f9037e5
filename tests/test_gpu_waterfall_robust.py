"""Robust waterfall read-outs on the GPU (include/psdcascade_robust.h, psdcx_*; csrc/waterfall_robust.hip;
stabilizer-stream_amd/robust.py): every output against numpy on stage_rows(), byte for byte.  The numpy statement of the
semantics is numpy_robust of tests/test_waterfall_robust_host.py, which that file holds against the host emulation."""
import numpy as np
import pytest

from test_gpu_waterfall import ZOOM_F0, stage_gsc
from test_sk_host import gaussian
from test_waterfall_robust_host import numpy_robust, same_f32

pytestmark = pytest.mark.gpu

INF = float("inf")
KINDS = ("median", "min", "max")


@pytest.fixture(scope="module")
def robust(pkg):
    from stabilizer_stream_amd import robust as mod
    return mod


def make(pkg, zoom, n, block, depth):
    return pkg.ZoomWaterfallCascade(n, f0=ZOOM_F0, block=block, depth=depth) if zoom else pkg.WaterfallCascade(n, block=block, depth=depth)


def complete_rows(g, stage, sides):
    """(block indices, V [R][sides][bins], W) of the complete blocks a stage's ring holds, oldest first, from stage_rows()"""
    got = g.stage_rows(stage)
    idx, cnt = got[0], got[1]
    ok = cnt == g.block
    assert np.all(ok[:-1]) if ok.size else True  # only the newest block may be partial
    V = np.stack([got[2 + s][ok] for s in range(sides)], axis=1) if ok.any() else np.zeros((0, sides, g.n // 2 + 1))
    W = np.stack([got[2 + sides + s][ok] for s in range(sides)], axis=1) if ok.any() else np.zeros((0, sides, g.n // 2 + 1))
    return idx[ok], V, W


def gap_limits(pkg, block, V, W):
    """(sk_lo, sk_hi) placed in gaps of the data: of the f64 SK of every (row, side, bin), sorted, around the 15 % and the 85 %
    quantile the midpoint of the widest of the 16 nearest gaps, which must exceed 1e-9 (the device's f64 may contract a
    multiply-add: 1e-9 is six orders above that), so that no row is near a limit and kept / excised can be compared at every bin"""
    sk = np.sort(pkg.sk_from_moments(block, V, W).ravel())
    sk = sk[~np.isnan(sk)]
    assert sk.size > 64
    out = []
    for q in (0.15, 0.85):
        c = int(q * sk.size)
        lo = max(0, min(c - 8, sk.size - 17))
        gaps = np.diff(sk[lo:lo + 17])
        i = int(np.argmax(gaps))
        assert gaps[i] > 1e-9, (q, gaps[i])
        out.append(0.5 * (sk[lo + i] + sk[lo + i + 1]))
    assert out[0] < out[1]
    return tuple(out)


def parity_input(n, block, segs):
    """Gaussian noise for `segs` Hann segments of stage 0 (and 17 samples more), a tone gated on for about a third of the blocks, one
    block's worth of samples at 100 x amplitude"""
    hop = n // 2
    length = n + (segs - 1) * hop + 17
    x = gaussian(length, 4000 + n + segs).astype(np.float64)
    t = np.arange(length)
    per = block * hop
    gate = (t // per) % 3 == 1
    x += gate * 5.0 * np.cos(2 * np.pi * (0.2 + 1.0 / (3 * n)) * t)
    x[20 * per + 7:21 * per + 7] *= 100.0
    return x.astype(np.float32)


def check_stage(pkg, robust, g, stage, sides, zoom, max_rows, limits_cache):
    """one stage and max_rows against numpy; returns the rows considered"""
    n, block = g.n, g.block
    idx, V, W = complete_rows(g, stage, sides)
    cap = robust.MAX_ROWS if max_rows is None else max_rows
    R = min(cap, idx.size)
    plain = robust.stage_robust(g, stage, max_rows=max_rows)
    assert set(plain) == {"median", "min", "max", "rows", "first_block", "last_block"}
    shape = (2, n // 2 + 1) if zoom else (n // 2 + 1,)
    assert plain["rows"] == R
    for k in KINDS:
        assert plain[k].dtype == np.float32 and plain[k].shape == shape
    if R == 0:
        assert all(np.all(np.isnan(plain[k])) for k in KINDS)
        r = robust.stage_robust(g, stage, max_rows=max_rows, sk_limits=(-INF, INF))
        assert r["rows"] == 0 and np.all(np.isnan(r["excised"])) and r["kept"].dtype == np.uint32 and not r["kept"].any()
        return 0
    assert (plain["first_block"], plain["last_block"]) == (int(idx[-R]), int(idx[-1]))
    gsc = stage_gsc(pkg, n, pkg.Window.HANN, block, stage)
    if stage not in limits_cache:  # from every considered row of the stage (max_rows None); fewer rows are a subset
        limits_cache[stage] = gap_limits(pkg, block, V[-min(robust.MAX_ROWS, idx.size):], W[-min(robust.MAX_ROWS, idx.size):])
    lo, hi = limits_cache[stage]
    med, mn, mx, exc, kept = numpy_robust(pkg, V[-R:], W[-R:], block, gsc, lo, hi)
    for k, want in zip(KINDS, (med, mn, mx)):
        assert plain[k].reshape(sides, -1).tobytes() == want.tobytes(), (stage, max_rows, k)
    r = robust.stage_robust(g, stage, max_rows=max_rows, sk_limits=(lo, hi))
    assert (r["rows"], r["first_block"], r["last_block"]) == (R, int(idx[-R]), int(idx[-1]))
    for k in KINDS:
        assert r[k].tobytes() == plain[k].tobytes()
    assert r["kept"].dtype == np.uint32 and np.array_equal(r["kept"].reshape(sides, -1), kept), (stage, max_rows)
    assert same_f32(r["excised"].reshape(sides, -1), exc), (stage, max_rows)
    if R >= 5:
        assert 0 < kept.sum() < kept.size * R  # the limits cut on both sides
    return R


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("partial", [True, False], ids=["newest-partial", "newest-complete"])
def test_parity_with_numpy(pkg, robust, gpu_required, zoom, n, partial):
    """B = 8, K = 12, 41 blocks at stage 0 (the ring has wrapped more than twice) and a few at stage 1; the newest block of stage 0
    holds 3 of 8 segments (left out) or all 8 (in).  For every stage and max_rows in {None, 1, 2, 5, 6}: median, min, max byte for
    byte np.float32(stat(V) * np.float64(gsc)); rows, first_block, last_block from stage_rows' indices and counts; kept and excised
    byte for byte at every bin with the limits placed in gaps of the data; a stage without a complete block gives rows == 0."""
    block, depth = 8, 12
    sides = 2 if zoom else 1
    segs = 40 * block + (3 if partial else block)
    g = make(pkg, zoom, n, block, depth)
    x = parity_input(n, block, segs)
    for s in range(0, x.size, 50_000):
        g.process(x[s:s + 50_000])
    info = g.stage_blocks(0)
    assert info["started"] == 41 > 2 * depth and info["newest_count"] == (3 if partial else block)
    assert g.num_stages() >= 3 and g.stage_blocks(1)["started"] >= 4
    limits = {}
    seen = []
    for stage in range(g.num_stages()):
        for max_rows in (None, 1, 2, 5, 6):
            seen.append(check_stage(pkg, robust, g, stage, sides, zoom, max_rows, limits))
    assert robust.stage_robust(g, 0)["rows"] == (depth - 1 if partial else depth)
    assert robust.stage_robust(g, 0)["last_block"] == (39 if partial else 40)
    assert 0 in seen and 6 in seen and 5 in seen  # a stage without a complete block; an even and an odd R above 2
    r = robust.stage_robust(g, 0, max_rows=0)
    assert r["rows"] == 0 and np.all(np.isnan(r["median"]))


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_device_outputs(pkg, robust, gpu_required, zoom):
    """the same calls into torch tensors prefilled with -1: the bytes of the host call, nothing written behind [sides][n/2 + 1];
    each output alone gives the same bytes; every call is exactly one launch, whatever was asked"""
    import torch
    n, block, depth = 64, 8, 12
    sides = 2 if zoom else 1
    g = make(pkg, zoom, n, block, depth)
    g.process(parity_input(n, block, 40 * block + 3))
    _, V, W = complete_rows(g, 0, sides)
    lim = gap_limits(pkg, block, V, W)
    ne, pad = sides * (n // 2 + 1), 64
    names = ("median", "min", "max", "excised", "kept")
    for stage, max_rows in ((0, None), (0, 5), (1, None)):
        host = robust.stage_robust(g, stage, max_rows=max_rows, sk_limits=lim)
        assert host["rows"] > 0
        t = {k: torch.full((ne + pad,), -1, device="cuda", dtype=torch.int32 if k == "kept" else torch.float32) for k in names}
        torch.cuda.synchronize()
        la = g.stats_read()["launches"]
        info = robust.stage_robust_device(g, stage, {k: v.data_ptr() for k, v in t.items()}, max_rows=max_rows, sk_limits=lim)
        assert g.stats_read()["launches"] == la + 1
        assert info == {k: host[k] for k in ("rows", "first_block", "last_block")}
        for k in names:
            got = t[k].cpu().numpy()
            assert got[:ne].tobytes() == host[k].tobytes(), (stage, max_rows, k)
            assert np.all(got[ne:] == -1), (stage, max_rows, k)
        for k in names:  # each output alone
            one = torch.full((ne + pad,), -1, device="cuda", dtype=t[k].dtype)
            torch.cuda.synchronize()
            la = g.stats_read()["launches"]
            robust.stage_robust_device(g, stage, {k: one.data_ptr()}, max_rows=max_rows,
                                       sk_limits=lim if k in ("excised", "kept") else None)
            assert g.stats_read()["launches"] == la + 1, k
            got = one.cpu().numpy()
            assert got[:ne].tobytes() == host[k].tobytes() and np.all(got[ne:] == -1), (stage, max_rows, k)
        la = g.stats_read()["launches"]
        robust.stage_robust(g, stage, max_rows=max_rows)
        robust.stage_robust(g, stage, max_rows=max_rows, sk_limits=lim)
        assert g.stats_read()["launches"] == la + 2
    # no complete block: nothing written, nothing launched
    ns = g.num_stages()
    assert g.stage_blocks(ns - 1)["started"] <= 1 and g.stage_blocks(ns - 1)["newest_count"] < block
    one = torch.full((ne,), -1.0, device="cuda")
    torch.cuda.synchronize()
    la = g.stats_read()["launches"]
    assert robust.stage_robust_device(g, ns - 1, {"median": one.data_ptr()})["rows"] == 0
    assert g.stats_read()["launches"] == la and np.all(one.cpu().numpy() == -1)


def test_ties(pkg, robust, gpu_required):
    """n = 64, B = 4, K = 4, a stream periodic in the hop: every segment of stage 0 is the same, so every block's row is, and
    median == min == max at every bin, bit for bit (R = 4: the even median is 0.5 (v + v))"""
    n, block, depth = 64, 4, 4
    period = gaussian(n // 2, 4100)
    g = pkg.WaterfallCascade(n, block=block, depth=depth)
    g.process(np.tile(period, 2 * 7 * block + 1))
    idx, cnt, s1, _ = g.stage_rows(0)
    assert idx.size == depth and cnt.tolist() == [block] * depth
    for max_rows in (None, 3):
        r = robust.stage_robust(g, 0, max_rows=max_rows, sk_limits=(-INF, INF))
        assert r["rows"] == (depth if max_rows is None else 3)
        assert r["median"].tobytes() == r["min"].tobytes() == r["max"].tobytes()
        assert np.all(r["median"] > 0) and np.all(np.isfinite(r["median"]))
        assert np.all(r["kept"] == r["rows"]) and r["excised"].tobytes() == r["median"].tobytes()


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_zeros(pkg, robust, gpu_required, zoom):
    """an all-zero stream: median, min and max 0, kept 0 and excised NaN (SK is NaN without power), at every stage with a row"""
    n, block, depth = 64, 4, 4
    g = make(pkg, zoom, n, block, depth)
    g.process(np.zeros(32 * 4 * 70, np.float32))
    seen = 0
    for k in range(g.num_stages()):
        r = robust.stage_robust(g, k, sk_limits=(-INF, INF))
        if not r["rows"]:
            continue
        seen += 1
        for name in KINDS:
            assert r[name].tobytes() == np.zeros_like(r[name]).tobytes(), (k, name)
        assert not r["kept"].any() and np.all(np.isnan(r["excised"]))
    assert seen >= 2


def test_nan_block(pkg, robust, gpu_required):
    """n = 64, B = 4, K = 6: noise, one block's worth of NaN samples, noise.  While a block the NaN touched is among the considered
    rows median, min and max are NaN at every bin; excised stays finite with kept = R - (rows touched by NaN); max_rows that
    reaches only clean rows is finite; once the touched blocks have left the ring everything is finite."""
    n, block, depth = 64, 4, 6
    per = block * 32
    g = pkg.WaterfallCascade(n, block=block, depth=depth)
    g.process(gaussian(3 * per + 32, 4200))
    g.process(np.full(per, np.nan, np.float32))
    g.process(gaussian(2 * per, 4201))
    idx, cnt, s1, _ = g.stage_rows(0)
    assert cnt.tolist() == [block] * idx.size and idx.size == depth
    touched = np.isnan(s1).any(axis=1)
    assert np.array_equal(touched, np.isnan(s1).all(axis=1)) and 1 <= touched.sum() <= 2 and not touched[-1]
    r = robust.stage_robust(g, 0, sk_limits=(-INF, INF))
    assert r["rows"] == depth
    for name in KINDS:
        assert np.all(np.isnan(r[name])), name
    assert np.all(np.isfinite(r["excised"])) and np.all(r["kept"] == depth - int(touched.sum()))
    clean = int(np.argmax(touched[::-1]))  # rows behind the newest touched one
    assert clean >= 1
    r = robust.stage_robust(g, 0, max_rows=clean, sk_limits=(-INF, INF))
    assert r["rows"] == clean and all(np.all(np.isfinite(r[name])) for name in KINDS + ("excised",)) and np.all(r["kept"] == clean)
    g.process(gaussian(depth * per, 4202))
    idx, cnt, s1, _ = g.stage_rows(0)
    assert np.all(np.isfinite(s1))
    r = robust.stage_robust(g, 0, sk_limits=(-INF, INF))
    assert all(np.all(np.isfinite(r[name])) for name in KINDS + ("excised",)) and np.all(r["kept"] == r["rows"])


def test_a_burst_moves_the_median_by_at_most_c_order_statistics(pkg, robust, gpu_required):
    """Stage 0, n = 256, B = 8, K = 32, 30 blocks: the same noise in the same calls twice, the second time with a 100 x burst inside
    the nominal span of three blocks.  The burst touches c blocks (block_span; consecutive blocks share `overlap` samples), c <= 4.
    The rows of every untouched block are bit-identical between the runs.  Changing c of R values moves the j-th order statistic
    by at most c places, so with m = (R - 1) // 2 the contaminated median lies between the clean rows' order statistics
    max(0, m - c) and min(R - 1, R - 1 - m + c), scaled by g: no tolerance enters.  The mean of the contaminated rows exceeds the
    clean rows' maximum at more than half of the bins -- the thing the median is for: the burst is a factor 10^4 in power, while a
    block's row (a chi-square of at most 16 degrees of freedom a bin) spreads by a factor of about 10 between its 0.1 % and
    99.9 % quantiles."""
    n, block, depth = 256, 8, 32
    hop = n // 2
    blocks = 30
    length = n + (blocks * block - 1) * hop + 5
    x = gaussian(length, 4300)
    runs = []
    span = lambda b: pkg.waterfall_block_span(n, hop, block, 0, b)  # noqa: E731
    b0, b1 = span(10).start + 50, span(12).stop - hop
    assert span(10).start <= b0 < b1 <= span(12).stop
    for burst in (False, True):
        y = x.copy()
        if burst:
            y[b0:b1] *= 100.0
        g = pkg.WaterfallCascade(n, block=block, depth=depth)
        for s in range(0, length, 5000):
            g.process(y[s:s + 5000])
        idx, cnt, s1, _ = g.stage_rows(0)
        assert idx.tolist() == list(range(blocks)) and cnt.tolist() == [block] * blocks
        assert g.block_span(0, 3) == span(3)
        runs.append((s1, robust.stage_robust(g, 0)))
    touched = [b for b in range(blocks) if span(b).start < b1 and span(b).stop > b0]
    c = len(touched)
    assert 3 <= c <= 4 and set(touched) >= {10, 11, 12}, touched
    (clean, rc), (cont, rb) = runs
    untouched = [b for b in range(blocks) if b not in touched]
    assert clean[untouched].tobytes() == cont[untouched].tobytes()
    assert not np.array_equal(clean[touched], cont[touched])
    R = rb["rows"]
    assert R == rc["rows"] == blocks
    gsc = np.float64(stage_gsc(pkg, n, pkg.Window.HANN, block, 0))
    cs = np.sort(clean, axis=0)
    m = (R - 1) // 2
    lo = (cs[max(0, m - c)] * gsc).astype(np.float32)
    hi = (cs[min(R - 1, R - 1 - m + c)] * gsc).astype(np.float32)
    assert np.all(lo <= rb["median"]) and np.all(rb["median"] <= hi)
    assert np.all((cs[m] * gsc).astype(np.float32) <= rc["median"]) and np.all(rc["median"] <= (cs[R - 1 - m] * gsc).astype(np.float32))
    above = np.mean(cont, axis=0) > cs[-1]
    print(f"burst: {c} blocks touched; the mean of the rows exceeds the clean maximum at {int(above.sum())} of {above.size} bins; "
          f"median moved by at most {float(np.max(rb['median'] / rc['median'])):.3g} x")
    assert above.sum() > above.size // 2


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_robust_psd(pkg, robust, gpu_required, zoom):
    """robust_psd of every kind: breaks equal pkg.stitch's for the counts (B where a stage has a complete block, else 0), field by
    field; inside every included break's bins every value within 2^-22 relative of the stage's robust row at the source bin (three
    f32 roundings of 2^-24: the division by gsc, the stitch's product, the row's own).  kind "excised" with limits (-inf, inf) is the
    mean of the complete blocks: within 2^-22 of the stitch of the summed rows of exactly those blocks, which at stage 0 (its
    newest block complete) is recent_psd(blocks=rows)."""
    n, block, depth = 256, 8, 8
    sides = 2 if zoom else 1
    g = make(pkg, zoom, n, block, depth)
    g.process(parity_input(n, block, 41 * block))
    ns = g.num_stages()
    b = g._b
    assert g.stage_blocks(0)["newest_count"] == block and ns >= 3
    tol = 2.0 ** -22
    opts = pkg.MergeOpts()
    avgs = [0xFFFFFFFF >> (3 * k) for k in range(ns)]
    pend = [g.stage_blocks(k)["pending"] for k in range(ns)]
    for kind in ("median", "min", "max", "excised"):
        lim = (-INF, INF) if kind == "excised" else None
        rows = [robust.stage_robust(g, k, sk_limits=lim) for k in range(ns)]
        counts = [block if r["rows"] else 0 for r in rows]
        assert counts[0] == block and counts[-1] == 0
        out = robust.robust_psd(g, kind=kind, sk_limits=lim, opts=opts)
        assert len(out) == sides + 1
        _, ref_br = pkg.stitch(n, counts, avgs, pend, np.ones((ns, n // 2 + 1), np.float32), opts, window=pkg.Window.HANN)
        br = out[-1]
        assert len(br) == len(ref_br) == ns
        for a, r in zip(br, ref_br):
            assert a == r and (a.start, a.include, a.count, a.avg, a.bins, a.fft_size, a.decimation, a.pending, a.processed) == \
                (r.start, r.include, r.count, r.avg, r.bins, r.fft_size, r.decimation, r.pending, r.processed)
        included = 0
        for i, a in enumerate(br):
            k = ns - 1 - i
            if not a.include:
                assert counts[k] == 0
                continue
            included += 1
            for s in range(sides):
                got = out[s][a.start:a.start + len(a.bins)].astype(np.float64)
                want = rows[k][kind].reshape(sides, -1)[s][a.bins.start:a.bins.stop].astype(np.float64)
                rel = np.abs(got - want) / want
                print(f"robust_psd {kind} stage {k} side {s}: worst relative distance to the row {rel.max() * 2 ** 24:.3g} x 2^-24")
                assert np.all(rel <= tol), (kind, k, s)
        assert included >= 2 and sum(len(a.bins) for a in br if a.include) == out[0].size
        if kind != "excised":
            continue
        # the mean of the complete blocks against the stitch of their summed rows
        sums = np.zeros((sides, ns, n // 2 + 1), np.float32)
        tot = []
        for k in range(ns):
            _, V, _ = complete_rows(g, k, sides)
            V = V[-rows[k]["rows"]:] if rows[k]["rows"] else V[:0]
            tot.append(block * V.shape[0])
            sums[:, k] = V.sum(axis=0)
        for s in range(sides):
            ref, rbr = pkg.stitch(n, tot, avgs, pend, sums[s], opts, window=pkg.Window.HANN)
            assert [a.bins for a in rbr] == [a.bins for a in br] and [a.include for a in rbr] == [a.include for a in br]
            rel = np.abs(out[s].astype(np.float64) - ref) / ref
            print(f"robust_psd excised side {s}: worst relative distance to the stitched mean {rel.max() * 2 ** 24:.3g} x 2^-24")
            assert np.all(rel <= tol), s
        recent = g.recent_psd(blocks=rows[0]["rows"])
        a = br[-1]  # stage 0
        for s in range(sides):
            got, ref = out[s][a.start:], recent[s][recent[-1][-1].start:]
            assert got.size == ref.size == len(a.bins)
            assert np.all(np.abs(got.astype(np.float64) - ref) <= tol * ref), s


@pytest.mark.parametrize("zoom", [False, True], ids=["real", "zoom"])
def test_argument_errors_on_a_live_object(pkg, robust, gpu_required, zoom):
    """no output requested; excised with NaN limits or lo > hi; a stage out of range: ERR_ARG with a text naming the argument, and
    the object is usable afterwards"""
    tag = "psdcx_zwf_robust" if zoom else "psdcx_wf_robust"
    g = (pkg.ZoomWaterfallCascadeBank if zoom else pkg.WaterfallCascadeBank)(64, 2, block=4, depth=4)
    g.process(0, gaussian(5000, 4400))
    ns = g.num_stages(0)
    before = robust.stage_robust(g, 0, sk_limits=(0.0, 2.0))
    assert before["rows"] == 3  # 155 segments: three complete blocks behind the partial newest one
    cases = [(lambda: robust.stage_robust_device(g, 0, {}), tag + "_device: null output"),
             (lambda: robust.stage_robust_device(g, 0, {"median": None}), "null output"),
             (lambda: robust.stage_robust(g, 0, sk_limits=(float("nan"), 2.0)), tag + ": sk_lo"),
             (lambda: robust.stage_robust(g, 0, sk_limits=(0.0, float("nan"))), "sk_hi"),
             (lambda: robust.stage_robust(g, 0, sk_limits=(2.0, 1.0)), "sk_lo <= sk_hi"),
             (lambda: robust.stage_robust_device(g, 0, {"kept": 8}, sk_limits=None), "sk_lo"),
             (lambda: robust.stage_robust(g, ns), f"{tag}: stage {ns} out of range"),
             (lambda: robust.stage_robust(g, 0, channel=2), "out of range (n_channels 2)")]
    for call, text in cases:
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))
    with pytest.raises(pkg.PsdError) as e:
        robust.robust_psd(g, kind="mean")
    assert e.value.code == pkg.ERR_ARG and "kind" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        robust.robust_psd(g, kind="excised")
    assert e.value.code == pkg.ERR_ARG and "sk_limits" in str(e.value)
    after = robust.stage_robust(g, 0, sk_limits=(0.0, 2.0))
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True) if isinstance(before[k], np.ndarray) else before[k] == after[k]
    assert robust.stage_robust(g, 0, sk_limits=(-INF, INF))["rows"] == 3  # infinite limits are allowed
    g.process(1, gaussian(5000, 4401))
    assert robust.stage_robust(g, 0, channel=1)["rows"] == 3
    g.close()


def test_cli_robust(pkg, robust, gpu_required, tmp_path):
    """tools/psd_cli.py --waterfall B:K --robust median --robust excised:3 --csv DIR: beside the unchanged files of a stage, one
    <stage>_robust.csv with a header line (rows and blocks considered) and one line a KIND, excised followed by its kept counts; the
    values are stage_robust()'s"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, block, depth = 512, 8, 16
    x = gaussian((1 << 16) + 777, 4500)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--raw", str(raw), "--waterfall", f"{block}:{depth}",
                        "--robust", "median", "--robust", "excised:3", "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    g = pkg.WaterfallCascade(n, block=block, depth=depth)
    g.set_detrend(pkg.Detrend.MEAN)  # the tool's default
    g.process(x)
    assert g.num_stages() >= 3
    for k in range(g.num_stages()):
        want = robust.stage_robust(g, k, sk_limits=robust.sk_limits(block, 3.0))
        assert (tmp_path / "csv" / f"waterfall_raw_stage{k}.csv").exists()
        lines = open(tmp_path / "csv" / f"waterfall_raw_stage{k}_robust.csv").read().splitlines()
        blocks = f"blocks {want['first_block']} ... {want['last_block']}" if want["rows"] else "no complete block"
        assert lines[0] == f"# stage {k} robust: {want['rows']} rows, {blocks}; lines: median excised:3 kept"
        assert len(lines) == 4
        for line, name in zip(lines[1:], ("median", "excised", "kept")):
            got = np.array([float(v) for v in line.split(",")])
            assert np.allclose(got, want[name], rtol=2e-6, atol=0, equal_nan=True), (k, name)
    bad = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--raw", str(raw), "--waterfall", f"{block}:{depth}",
                          "--robust", "mean"], capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "--robust takes" in bad.stderr
