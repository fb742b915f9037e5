"""Spectral kurtosis cascade on the GPU (psdc_sk_*, csrc/sk.hip) against the f64 restatement of tests/test_sk_host.py and its f32
sibling, against the auto-PSD and the pair object where row 0 makes them comparable, and the statistical properties the
restatement was shown to have there.  Semantics: include/psdcascade.h, "spectral kurtosis cascade"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS, window_of
from test_sk_host import (PROP_N, U32_MAX, check_gated, check_gauss, check_tone, gaussian, object_argument_errors, prop_input,
                          prop_restatement, restate_sk)

pytestmark = pytest.mark.gpu

# (n, window, detrend, avg (limit, count) or None, length -- or the lengths of the calls the stream is fed in).
# Hann hops n/2, the rectangular window n, the custom table 3n/4.
# Teams a tile: 32 at n = 64, 8 at 256, 2 at 1024, 1 at 4096 (a team takes two segments).
PARITY_CASES = [
    (64, "hann", "none", None, 200 * 64),                    # three live stages and more; default averaging
    (256, "rect", "mean", None, 200 * 256 + 17),
    (1024, "custom", "span", (3, U32_MAX), 200 * 1024),      # EWMA from the fifth segment of every stage
    (4096, "hann", "midpoint", (7, 64), 200 * 4096),         # limit 7 at stages 0 and 1, then 1, then 0
    (64, "hann", "none", (3, U32_MAX), 64),                  # exactly one segment
    (64, "rect", "span", (7, 64), 5 * 64),                   # 5 segments (odd), fewer than the 32 teams of a tile
    (256, "hann", "midpoint", (7, 64), 256 + 5 * 128),       # 6 segments (even), fewer than the 8 teams of a tile
    (1024, "hann", "mean", (7, 64), 200 * 1024 + 511),       # 399 segments at stage 0 (odd): EWMA change inside the call
    (4096, "rect", "none", None, 200 * 4096),                # 200 segments (even)
    (256, "custom", "none", (3, U32_MAX), 60_000),
    (4096, "hann", "mean", (3, U32_MAX), 3 * 4096),          # 5 segments, one team a tile
    (1024, "rect", "none", (7, 64), (1024, 8 * 1024)),       # segment 1 alone, then the pairs (2, 3) ... (8, 9): boxcar -> EWMA inside the last
    (256, "hann", "none", (3, U32_MAX), (256, 4 * 128, 40_000)),  # the pair (4, 5) of the second call is (boxcar, first EWMA segment)
]


def stitched(pkg, n, pwin, stages, key):
    wt = pwin if isinstance(pwin, pkg.WindowTable) else pkg.WindowTable._kind(n, pwin)
    rows = np.stack([s[key] for s in stages]).astype(np.float32)
    return pkg.stitch(n, [s["count"] for s in stages], [s["avg"] for s in stages], [s["pending"] for s in stages], rows,
                      pkg.MergeOpts(), window=wt)


def sk_by_breaks(pkg, g, breaks):
    """the merged SK row written out from the stage moments and the Breaks: Break i is stage ns - 1 - i"""
    ns = g.num_stages()
    out = []
    for i, b in enumerate(breaks):
        if not b.include:
            continue
        info, s1, s2 = g.stage_moments(ns - 1 - i)
        assert info["count"] == b.count
        out.append(pkg.sk_from_moments(info["count"], s1, s2)[b.bins.start:b.bins.stop])
    return np.concatenate(out) if out else np.zeros(0)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_sk_parity(pkg, ora, gpu_required, case):
    n, wkind, detrend, avg, length = PARITY_CASES[case]
    pwin, owin = window_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    calls = length if isinstance(length, tuple) else (length,)
    length = sum(calls)
    x = gaussian(length, 1000 + case)
    g = pkg.SkCascade(n, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    for s, e in zip(np.cumsum((0,) + calls[:-1]), np.cumsum(calls)):
        g.process(x[s:e])
    st64 = restate_sk(ora, x, n, owin, detrend, avg, "f64")
    st32 = restate_sk(ora, x, n, owin, detrend, avg, "f32")
    # 1. Breaks, counts, pendings: exact
    psd, br = g.psd()
    ref0, rbr = stitched(pkg, n, pwin, st64, "s1")
    assert br == rbr and g.num_stages() == len(st64)
    got = [g.stage_moments(k) for k in range(len(st64))]
    for k, ((info, _, _), s) in enumerate(zip(got, st64)):
        assert (info["count"], info["avg"], info["pending"]) == (s["count"], s["avg"], s["pending"]), k
    if length >= 200 * n:
        assert sum(1 for s in st64 if s["count"] > 0) >= 3
    # 2. row 0, merged, as test_zoom_parity holds a row
    print(f"case {case} row 0: worst relative error {np.max(np.abs(psd - ref0) / np.maximum(ref0, 1e-300)):.3g}")
    if detrend == "none":
        assert_psd_close(psd, ref0, f"sk row 0 case {case}", pure=True)
    else:
        assert_psd_close(psd, ref0, f"sk row 0 case {case} {detrend}", ref_f32=stitched(pkg, n, pwin, st32, "s1")[0])
    # 3. row 1, stage by stage, rtol 2e-5 (squaring doubles the relative error), held to the f32 restatement's own arithmetic
    for k, ((info, s1, s2), s, s32) in enumerate(zip(got, st64, st32)):
        if s["count"]:
            print(f"case {case} stage {k} count {s['count']}: worst relative error S1 {np.max(np.abs(s1 - s['s1']) / np.maximum(s['s1'], 1e-300)):.3g} "
                  f"S2 {np.max(np.abs(s2 - s['s2']) / np.maximum(s['s2'], 1e-300)):.3g}")
        assert_psd_close(s2, s["s2"], f"sk row 1 case {case} stage {k}", rtol=2e-5, ref_f32=s32["s2"])
    # 4. SK wherever both rows met their pure bounds: dR / R <= e2 + 2 e1 = 4e-5 with R = M S2 / S1^2
    worst = 0.0
    for k, ((info, s1, s2), s) in enumerate(zip(got, st64)):
        m = s["count"]
        if m < 2:
            assert np.all(np.isnan(pkg.sk_from_moments(m, s1, s2)))
            continue
        ok = (np.abs(s1 - s["s1"]) <= 1e-5 * s["s1"]) & (np.abs(s2 - s["s2"]) <= 2e-5 * s["s2"]) & (s["s1"] > 0)
        sk_g, sk_r = pkg.sk_from_moments(m, s1, s2)[ok], pkg.sk_from_moments(m, s["s1"], s["s2"])[ok]
        bound = 4e-5 * (sk_r + (m + 1.0) / (m - 1.0))
        if ok.any():
            worst = max(worst, float(np.max(np.abs(sk_g - sk_r) / bound)))
        assert np.all(np.abs(sk_g - sk_r) <= bound), (k, float(np.max(np.abs(sk_g - sk_r) / bound)))
    print(f"case {case} SK: worst |SK_gpu - SK_f64| / bound {worst:.3g}")
    # the merged SK is the stages' SK, selected by the Breaks of psd()
    sk, sbr = g.sk()
    assert sbr == br and sk.dtype == np.float64 and sk.size == psd.size
    assert np.array_equal(sk, sk_by_breaks(pkg, g, br), equal_nan=True)


def test_sk_row0_is_the_psd(pkg, gpu_required):
    """SkCascade.psd() against PsdCascade.psd() on the same stream: equal Breaks, pure 1e-5.  Stage rows against CsdCascade fed
    (x, x): S1 within 1e-5 of its sxx."""
    n = 1024
    x = gaussian(1 << 20, 77)
    g = pkg.SkCascade(n)
    g.process(x)
    psd, br = g.psd()
    p = pkg.PsdCascade(n)
    p.process(x)
    pp, pbr = p.psd()
    assert br == pbr
    rel = assert_psd_close(psd, pp, "sk psd vs PsdCascade", pure=True)
    c = pkg.CsdCascade(n)
    c.process(x, x)
    assert c.num_stages() == g.num_stages() >= 4
    worst = 0.0
    for k in range(g.num_stages()):
        info, s1, _ = g.stage_moments(k)
        cinfo, sxx, _, _ = c.stage_spectra(k)
        assert info["count"] == cinfo["count"] and info["pending"] == cinfo["pending"]
        if info["count"]:
            worst = max(worst, float(np.max(np.abs(s1 - sxx) / sxx)))
    print(f"psd vs PsdCascade {rel:.3g}; S1 vs the pair object's sxx {worst:.3g}")
    assert worst <= 1e-5


def moments(g):
    return [g.stage_moments(k) for k in range(g.num_stages())]


def same_moments(a, b, tol, what=""):
    """tol 0: equal bits; else both rows within tol (the pair object's chunking bound), statistics equal"""
    assert len(a) == len(b), what
    for k, ((ia, a1, a2), (ib, b1, b2)) in enumerate(zip(a, b)):
        assert ia == ib, (what, k)
        for u, v in ((a1, b1), (a2, b2)):
            if tol == 0:
                assert u.tobytes() == v.tobytes(), (what, k)
            else:
                assert np.all(np.abs(u - v) <= tol * v), (what, k, float(np.max(np.abs(u - v) / np.maximum(v, 1e-300))))


def test_sk_chunking_and_routes(pkg, gpu_required):
    """One call against calls of 1000, 77 777 and 2^20 + 3 samples, host and device: both rows within the pair object's chunking
    bound (2e-6).  The same calls twice, host against device, reset and replay: equal bits."""
    import torch
    n = 512
    cuts = np.cumsum([0, 1000, 77_777, (1 << 20) + 3])
    length = int(cuts[-1])
    x = gaussian(length, 31)
    one = pkg.SkCascade(n)
    one.process(x)
    ref = moments(one)
    a = pkg.SkCascade(n)
    for s, e in zip(cuts[:-1], cuts[1:]):
        a.process(x[s:e])
    got_a = moments(a)
    same_moments(got_a, ref, 2e-6, "host chunks")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    d = pkg.SkCascade(n)
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    got_d = moments(d)
    same_moments(got_d, ref, 2e-6, "device chunks")
    same_moments(got_d, got_a, 0, "host against device, same calls")
    one_d = pkg.SkCascade(n)
    one_d.process_device(dx.data_ptr(), length)
    same_moments(moments(one_d), ref, 0, "host against device, one call")
    a2 = pkg.SkCascade(n)
    for s, e in zip(cuts[:-1], cuts[1:]):
        a2.process(x[s:e])
    same_moments(moments(a2), got_a, 0, "same calls twice")
    psd_d, sk_d = d.psd(), d.sk()
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()  # settings too
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    same_moments(moments(d), got_d, 0, "reset + replay")
    assert d.psd()[1] == psd_d[1] and d.psd()[0].tobytes() == psd_d[0].tobytes() and d.sk()[0].tobytes() == sk_d[0].tobytes()
    assert d.stats()["samples_in"] == length


def test_sk_bank(pkg, gpu_required):
    """Two channels of a bank fed different streams equal two single objects bit for bit, each channel fed and read out in turn (so
    that its rounds are its single object's)."""
    n = 256
    xs = [gaussian(300_000, 400), gaussian(123_457, 401)]
    step = [65_536, 33_333]
    bank = pkg.SkCascadeBank(n, 2)
    for c, x in enumerate(xs):
        single = pkg.SkCascade(n)
        for s in range(0, x.size, step[c]):
            bank.process(c, x[s:s + step[c]])
            single.process(x[s:s + step[c]])
        got = [bank.stage_moments(c, k) for k in range(bank.num_stages(c))]
        same_moments(got, moments(single), 0, f"channel {c}")
        (p, br), (q, qbr) = bank.psd(c), single.psd()
        assert br == qbr and p.tobytes() == q.tobytes()
        assert bank.sk(c)[0].tobytes() == single.sk()[0].tobytes()
    # channel 0 is what it was before channel 1 was fed
    single = pkg.SkCascade(n)
    for s in range(0, xs[0].size, step[0]):
        single.process(xs[0][s:s + step[0]])
    same_moments([bank.stage_moments(0, k) for k in range(bank.num_stages(0))], moments(single), 0, "channel 0 afterwards")


def gpu_stages(pkg, case):
    g = pkg.SkCascade(PROP_N)
    g.process(prop_input(case))
    return moments(g)


def test_sk_gaussian_noise_reads_one(pkg, ora, gpu_required):
    """(a) of tests/test_sk_host.py on the GPU: the same input, the same assertions"""
    st = gpu_stages(pkg, "gauss")
    ref = prop_restatement(ora, "gauss")
    assert [i["count"] for i, _, _ in st] == [s["count"] for s in ref]
    check_gauss(lambda k: pkg.sk_from_moments(st[k][0]["count"], st[k][1], st[k][2]), [i["count"] for i, _, _ in st])
    sk0 = pkg.sk_from_moments(st[0][0]["count"], st[0][1], st[0][2])
    assert abs(sk0[0] - 2.0) < 0.5 and abs(sk0[-1] - 2.0) < 0.5  # the real-valued bins


def test_sk_tone_reads_zero(pkg, ora, gpu_required):
    """(b): a line of constant amplitude reads 0 at its bin, the noise beside it 1"""
    info, s1, s2 = gpu_stages(pkg, "tone")[0]
    assert info["count"] == prop_restatement(ora, "tone")[0]["count"]
    check_tone(pkg.sk_from_moments(info["count"], s1, s2))


def test_sk_gated_noise_reads_above_two(pkg, ora, gpu_required):
    """(c): noise that is on half of the time; the median within 0.01 of the restatement's"""
    info, s1, s2 = gpu_stages(pkg, "gated")[0]
    r = prop_restatement(ora, "gated")[0]
    assert info["count"] == r["count"]
    med = check_gated(pkg.sk_from_moments(info["count"], s1, s2))
    med_r = check_gated(pkg.sk_from_moments(r["count"], r["s1"], r["s2"]))
    assert abs(med - med_r) < 0.01, (med, med_r)


def test_sk_launches(pkg, gpu_required):
    """After warm-up a device call at ten live stages is one round of exactly 3 kernel launches (segments, decimators, fold + tails):
    what the pair object's device call adds, whose two input copies -- here one -- are no launches."""
    import torch
    n = 512
    m = 1 << 24
    dx = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.SkCascade(n)
    for _ in range(760):  # 1.3e10 samples: stage 9 takes its first ones after 1.0e10 (35 outputs drained and up to n samples held a stage)
        g.process_device(dx.data_ptr(), m)
    g.stats(reset=True)
    for _ in range(8):
        g.process_device(dx.data_ptr(), m)
    la = g.stats()["launches"]
    g.sync()
    assert g.num_stages() >= 10
    assert la == 3 * 8, la
    c = pkg.CsdCascade(n)
    for _ in range(4):
        c.process_device(dx.data_ptr(), dx.data_ptr(), m)
    c.stats_read(reset=True)
    c.process_device(dx.data_ptr(), dx.data_ptr(), m)
    assert c.stats_read()["launches"] == 3
    c.sync()


def test_sk_argument_errors_on_an_object(pkg, gpu_required):
    """Detrend::Linear, a channel out of range, a null sample pointer, a stage out of range"""
    object_argument_errors(pkg)


def test_sk_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --sk: the lines frequency,psd,sk against the object's read-out (one call here: the file is
    shorter than the tool's 2^20 samples a call), and the tone's bin counted among the bins away from 1"""
    fs = 1000.0
    length = (1 << 17) + 777
    x = (gaussian(length, 41) + 30.0 * np.cos(2 * np.pi * 0.2001 * np.arange(length))).astype(np.float32)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--raw", str(raw), "--sk", "--fs", str(fs), "--csv",
                        str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("sk raw:")]
    assert len(line) == 1 and "bins beyond 8 sigma of 1: " in line[0], r.stdout
    assert int(line[0].rsplit(": ", 1)[1]) >= 1
    bank = pkg.SkCascadeBank(512, 1)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.process(0, x)
    psd, br = bank.psd(0, pkg.MergeOpts(min_count=1))
    sk, _ = bank.sk(0, pkg.MergeOpts(min_count=1))
    d = np.loadtxt(tmp_path / "csv" / "sk_raw.csv", delimiter=",")
    assert d.shape == (psd.size, 3)
    assert np.allclose(d[:, 0], pkg.Break.frequencies(br) * fs, rtol=1e-6, atol=0)
    assert np.all(np.abs(d[:, 1] - psd) <= 2e-6 * psd + 1e-6 * np.mean(psd))
    assert np.array_equal(np.isnan(d[:, 2]), np.isnan(sk)) and np.allclose(d[:, 2], sk, rtol=1e-5, atol=1e-6, equal_nan=True)
    k = int(np.argmin(np.where(np.isnan(d[:, 2]), np.inf, d[:, 2])))
    assert abs(d[k, 0] - 0.2001 * fs) <= fs / 512 and d[k, 2] < 0.05  # the line reads 0 where everything else reads about 1
