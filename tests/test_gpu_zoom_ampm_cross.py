"""AM/PM cross cascades on the GPU (psdc_zxampm_*, psdc_iqxampm_*, csrc/zoom_ampm_cross.hip) against the f64 restatement of
tests/test_zoom_ampm_cross_host.py and its f32 sibling, against the zoom cross, AM/PM and zoom objects where the rows make them
comparable, and the readings of am_pm_cross() and carriers() the restatement was shown to give there.  Semantics:
include/psdcascade.h, "AM/PM cross cascades"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS, assert_sxy_close
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_sk_host import gaussian
from test_zoom_ampm_cross_host import (PROP_F0, PROP_N, check_common, check_const, check_delay, restate_zoom_ampm_cross,
                                       stage_am_pm_cross, twelve, xprop_input, xprop_restatement)
from test_zoom_cross_host import stitch_zoom_cross
from test_zoom_host import M64, U32_MAX, carrier_ftw, emul, mix_f32, windows_of  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the two auto rows a complex row is judged against: its pairing scale is the square root of their product
PAIRING = {4: (0, 2), 5: (1, 3), 8: (0, 3), 10: (1, 2)}  # sab_up, sab_lo, cab, cba (the row of the real part)
NAMES = {4: "sab_up", 5: "sab_lo", 8: "cab", 10: "cba"}

# (n, window, detrend, avg (limit, count) or None, carriers (a, b), length).  Hann hops n/2.
# Teams a workgroup (a tile is one segment a team): 32 at n = 64 (sixteen teams a wavefront; the last tile has idle teams), 2 at
# 1024 (a team is one wavefront); at 2048 one team of two wavefronts and at 4096 one of four (__syncthreads, the largest LDS).
# Lengths: three stages must be live and the deepest hold five averages, since the pure 1e-5 rule needs averaged bins (one
# periodogram has bins at 1e-4 of its level, where the error of ANY f32 transform, relative to the stage's level, is beyond 1e-5 of
# the bin: tests/test_gpu_zoom_ampm.py has the account; n (8^2 + 8) + 37 samples leave ONE segment there and were measured to miss the
# pure rule by 1.7e-5 and 2.6e-5 at one bin each at n = 1024 and 2048).  200 n + 37 samples give 399, 48 and 5 segments, an odd
# stage-0 count, at n >= 1024.
PARITY_CASES = [
    (64, "hann", "none", None, (("bin", 5), ("bin", 5)), 64 * 401 + 5),  # 801, 98 and 10 segments
    (1024, "hann", "none", (3, U32_MAX), (0.2345678901234567, 0.2345678901234567), 1024 * 200 + 37),  # EWMA from the fifth segment
    (2048, "hann", "midpoint", None, (3 ** 0.5 / 7, 0.3141592653589793), 2048 * 200 + 37),
    (4096, "hann", "mean", (7, 64), (0.6180339887498949, 0.6180339887498949), 4096 * 200 + 37),
    (4096, "hann", "none", None, (0.7131313131313131, 0.2718281828459045), 4096 * 200 + 37),
    (1024, "hann", "mean", None, (0.1 * 2 ** 0.5, 0.1 * 2 ** 0.5), 1024 * 200 + 37),
    (64, "hann", "none", (3, U32_MAX), (0.2345678901234567, 0.2345678901234567), 64 * 3 + 5),  # 5 segments, fewer than the 32 teams
]

# (n, route, carrier, avg, detrend); Hann
IQ_PARITY_CASES = [
    (64, "interleaved", ("bin", 0), None, "none"),
    (1024, "planar", 0.2345678901234567, (7, 64), "mean"),
]


def make(pkg, n, ftw, window=None, phase0=(0, 0), detrend=None, avg=None, cls=None):
    g = (cls or pkg.ZoomAmPmCsdCascade)(n, window=window if window is not None else pkg.Window.HANN)
    for side in (0, 1):
        g.set_carrier(ftw=ftw[side], phase0=phase0[side], side=side)
    if detrend is not None:
        g.set_detrend(detrend)
    if avg is not None:
        g.set_avg(pkg.AvgOpts(*avg))
    return g


def stage_rows(g):
    return [g.stage_rows(k) for k in range(g.num_stages())]


def stitch64(pkg, n, pwin, stages, breaks):
    """the (12, len) rows of stages (dicts with count and the (12, n/2 + 1) f64 rows) merged in f64 by the given Breaks: every
    selected bin times the f32 factor PsdCascade::psd applies to its stage (1 / (gain decimation)), as psdc_zxampm_sidebands does"""
    wt = pwin if isinstance(pwin, pkg.WindowTable) else pkg.WindowTable._kind(n, pwin)
    out = []
    ns = len(stages)
    for i, b in enumerate(breaks):
        if not b.include:
            continue
        s = stages[ns - 1 - i]
        gain = np.float32((n // 2) * s["count"]) * np.float32(wt.nenbw) * np.float32(wt.power)
        gsc = float(np.float32(1.0) / (gain * np.float32(b.decimation)))
        out.append(s["rows12"][:, b.bins.start:b.bins.stop] * gsc)
    return np.concatenate(out, axis=1) if out else np.zeros((12, 0))


def merged_rows(g):
    """sidebands() back as (12, len) f64 rows and the Breaks"""
    sb = g.sidebands()
    c = sb[4:8]
    return np.stack([sb[0], sb[1], sb[2], sb[3], c[0].real, c[1].real, c[0].imag, c[1].imag, c[2].real, c[2].imag, c[3].real,
                     c[3].imag]), sb[8]


def cplx(rows, r):
    """the complex row whose real part is row r: rows 4 .. 7 interleave upper / lower, rows 8 .. 11 are (re, im) pairs"""
    return rows[r] + 1j * rows[r + 2 if r < 8 else r + 1]


def check_rows(got, ref, sib, detrend, what, autos=True):
    """(12, len) rows against the f64 reference's: detrend none: rows 0 ... 3 within the pure 1e-5, every complex row within 1e-5
    sqrt of the two auto rows it pairs.  Under a detrend the widened rule: the auto rows held to the f32 sibling `sib`, the complex
    rows plus 1e-6 of the bound's mean, as assert_parity of tests/test_gpu_zoom_ampm.py widens them (which, as here with
    autos=False, holds a stage's raw auto rows under a detrend through the merged read-out only).  Returns the worst figures."""
    worst = {}
    for r in range(4 if autos else 0):
        if detrend == "none":
            worst[r] = assert_psd_close(got[r], ref[r], f"{what} row {r}", pure=True)
        else:
            worst[r] = assert_psd_close(got[r], ref[r], f"{what} row {r} {detrend}", ref_f32=sib[r])
    for r, (u, v) in PAIRING.items():
        assert_sxy_close(cplx(got, r), cplx(ref, r), ref[u], ref[v], 1e-5, f"{what} {NAMES[r]}", atol_frac=0.0 if detrend == "none" else 1e-6)
        scale = np.sqrt(ref[u] * ref[v])
        worst[r] = float(np.max(np.abs(cplx(got, r) - cplx(ref, r)) / np.maximum(scale, 1e-9 * np.max(scale) + 1e-300))) if scale.size else 0.0
    return worst


def assert_parity(pkg, g, st64, st32, n, pwin, detrend, what):
    """the assertions of both parity tests: g against the f64 restatement st64, with the f32 sibling st32 as the yardstick of the
    widened bounds"""
    for st in (st64, st32 or []):
        for s in st:
            s["rows12"] = twelve(s)
    # 1. Breaks, counts, averages, pendings: exact
    got12, br = merged_rows(g)
    rbr = stitch_zoom_cross(pkg, n, pwin, st64)[6]
    assert br == rbr and g.num_stages() == len(st64)
    got = stage_rows(g)
    for k, (m, s) in enumerate(zip(got, st64)):
        assert (m[0]["count"], m[0]["avg"], m[0]["pending"]) == (s["count"], s["avg"], s["pending"]), k
        if not s["count"]:
            assert not m[1].any(), k
    # 2. the merged rows (the Breaks leave out the transition band of the decimated stages), and all of stage 0's raw rows
    r64 = stitch64(pkg, n, pwin, st64, br)
    r32 = stitch64(pkg, n, pwin, st32, br) if st32 else None
    w = check_rows(got12, r64, r32, detrend, f"{what} merged")
    print(f"{what} merged: worst relative error rows 0-3 {max(w[r] for r in range(4)):.3g}; worst error / pairing scale "
          + ", ".join(f"{NAMES[r]} {w[r]:.3g}" for r in PAIRING))
    if st64[0]["count"]:
        check_rows(got[0][1], st64[0]["rows12"], st32[0]["rows12"] if st32 else None, detrend, f"{what} stage 0",
                   autos=detrend == "none")
    # 3. sidebands(): f64, every bin the stage's accumulator times the stage's factor; csd() is its rows 0 ... 7 in f32
    sb = g.sidebands()
    assert all(a.dtype == np.float64 for a in sb[:4]) and all(a.dtype == np.complex128 for a in sb[4:8])
    gst = [dict(count=m[0]["count"], rows12=m[1]) for m in got]
    assert got12.tobytes() == stitch64(pkg, n, pwin, gst, br).tobytes()
    cs = g.csd()
    assert cs[6] == br and all(a.dtype == np.float32 for a in cs[:4]) and all(a.dtype == np.complex64 for a in cs[4:6])
    for a, b in zip(cs[:6], sb[:6]):
        assert a.tobytes() == b.astype(a.dtype).tobytes()
    return br


def live_stages(st):
    return [s["count"] for s in st if s["count"] > 0]


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_zoom_ampm_cross_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, avg, carriers, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    a = gaussian(length + 3, 5000 + case)
    b = (0.6 * a[:-3] + 0.8 * gaussian(length, 6000 + case)).astype(np.float32)  # coherence neither 0 nor 1
    a = a[3:].copy()
    ftw = tuple(carrier_ftw(pkg, n, c) for c in carriers)
    g = make(pkg, n, ftw, pwin, detrend=DETRENDS[detrend], avg=avg)
    g.process(a, b)
    st64 = restate_zoom_ampm_cross(ora, a, b, n, ftw, (0, 0), owin, detrend, avg)
    st32 = None
    if detrend != "none":
        iq = (mix_f32(emul, a, ftw[0]), mix_f32(emul, b, ftw[1]))
        st32 = restate_zoom_ampm_cross(ora, a, b, n, ftw, (0, 0), owin, detrend, avg, "f32", iq=iq)
    if length > 40 * n:
        teams = max(1, 128 // (n // 16))
        nseg = 1 + (length - n) // (n // 2)
        live = live_stages(st64)
        deep = st64[len(live) - 1]  # five averages, or as many as the stage's limit lets its count show
        assert len(live) >= 3 and live[-1] >= min(5, deep["avg"] + 1) and nseg % 2 == 1 and (teams == 1 or nseg % teams), (live, nseg, teams)
    br = assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"zoom ampm cross case {case}")
    # stages and Breaks are those of the zoom cross object fed the pair
    z = pkg.ZoomCsdCascade(n, window=pwin)
    for side in (0, 1):
        z.set_carrier(ftw=ftw[side], side=side)
    z.set_detrend(DETRENDS[detrend])
    z.set_avg(pkg.AvgOpts(*avg))
    z.process(a, b)
    assert z.csd()[6] == br and g.num_stages() == z.num_stages()


@pytest.mark.parametrize("case", range(len(IQ_PARITY_CASES)))
def test_iq_ampm_cross_parity(pkg, ora, gpu_required, iq_emul, case):  # noqa: F811
    n, route, carrier, avg, detrend = IQ_PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, "hann")
    avg = avg or (U32_MAX, U32_MAX)
    length = n * 200 + 37 if n >= 1024 else n * 401 + 5
    ia, qa = gaussian(length, 7000 + case), gaussian(length, 7100 + case)
    ib = (0.6 * ia + 0.8 * gaussian(length, 7200 + case)).astype(np.float32)
    qb = (0.6 * qa + 0.8 * gaussian(length, 7300 + case)).astype(np.float32)
    ftw = carrier_ftw(pkg, n, carrier)
    g = make(pkg, n, (ftw, ftw), pwin, detrend=DETRENDS[detrend], avg=avg, cls=pkg.IqAmPmCsdCascade)
    if route == "planar":
        g.process((ia, qa), (ib, qb))
    else:
        g.process((ia + 1j * qa).astype(np.complex64), (ib + 1j * qb).astype(np.complex64))
    iq64 = (mix_c_f64(ia, qa, ftw), mix_c_f64(ib, qb, ftw))
    st64 = restate_zoom_ampm_cross(ora, None, None, n, (ftw, ftw), (0, 0), owin, detrend, avg, "f64", iq=iq64)
    st32 = None
    if detrend != "none":
        iq32 = (mix_c_f32(iq_emul, ia, qa, ftw), mix_c_f32(iq_emul, ib, qb, ftw))
        st32 = restate_zoom_ampm_cross(ora, None, None, n, (ftw, ftw), (0, 0), owin, detrend, avg, "f32", iq=iq32)
    live = live_stages(st64)
    assert len(live) >= 3 and live[-1] >= min(5, st64[len(live) - 1]["avg"] + 1)
    assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"iq ampm cross case {case}")


def test_zoom_ampm_cross_rows_0_7_are_the_zoom_cross_objects(pkg, gpu_required):
    """every stage's rows 0 ... 7 against ZoomCsdCascade / IqCsdCascade fed the same pair (N = 1024, 2^19 samples): equal statistics
    and Breaks, auto rows within 2e-6 relative, cross rows within 2e-6 of the pairing scale"""
    n, m = 1024, 1 << 19
    a, b0 = gaussian(m, 77), gaussian(m, 78)
    b = (0.6 * a + 0.8 * b0).astype(np.float32)
    ftw = (pkg.zoom_ftw(0.2)[0], pkg.zoom_ftw(0.2)[0])
    za, zb = (a + 1j * b0).astype(np.complex64), (b + 1j * a).astype(np.complex64)
    for name, new, old, feed in (("zoom", make(pkg, n, ftw), pkg.ZoomCsdCascade(n, f0=0.2), (a, b)),
                                 ("iq", make(pkg, n, ftw, cls=pkg.IqAmPmCsdCascade), pkg.IqCsdCascade(n, f0=0.2), (za, zb))):
        new.process(*feed)
        old.process(*feed)
        assert new.csd()[6] == old.csd()[6] and new.num_stages() == old.num_stages() >= 3
        worst = 0.0
        for k in range(new.num_stages()):
            info, rows = new.stage_rows(k)
            oinfo, orows = old.stage_spectra(k)
            assert info == oinfo, (name, k)
            if not info["count"]:
                continue
            orows = orows.astype(np.float64)
            for r in range(8):
                scale = orows[r] if r < 4 else np.sqrt(orows[PAIRING[4 + r % 2][0]] * orows[PAIRING[4 + r % 2][1]])
                # (the zoom cross object's read-out rounds its rows to f32: 2^-24 of the row's own size is not the kernel's)
                err = np.abs(rows[r] - orows[r]) - 2.0 ** -24 * np.abs(orows[r])
                worst = max(worst, float(np.max(err / scale)))
                assert np.all(err <= 2e-6 * scale), (name, k, r, float(np.max(err / scale)))
        print(f"{name}: rows 0-7 against the eight-row object, worst difference / pairing scale {worst:.3g}")


def test_zoom_ampm_cross_same_stream_is_the_ampm_object(pkg, gpu_required):
    """fed (x, x) with one carrier: sab_up, sab_lo are ZoomAmPmCascade's upper, lower (real), cab and cba its comp, every stage,
    within 2e-6 of the pairing scale"""
    n, m = 512, 1 << 19
    x = gaussian(m, 81)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    g = make(pkg, n, (ftw, ftw))
    g.process(x, x)
    one = pkg.ZoomAmPmCascade(n, ftw=ftw)
    one.process(x)
    assert g.num_stages() == one.num_stages() >= 4
    worst, seen = 0.0, 0
    for k in range(g.num_stages()):
        info, r = g.stage_rows(k)
        oinfo, up, lo, comp = one.stage_rows(k)
        assert info == oinfo
        if not info["count"]:
            continue
        seen += 1
        both = np.sqrt(up * lo)
        for got, want, scale in ((cplx(r, 4), up, up), (cplx(r, 5), lo, lo), (cplx(r, 8), comp, both), (cplx(r, 10), comp, both),
                                 (r[0], up, up), (r[1], lo, lo), (r[2], up, up), (r[3], lo, lo)):
            e = float(np.max(np.abs(got - want) / scale))
            worst = max(worst, e)
            assert e <= 2e-6, (k, e)
    print(f"(x, x) against the AM/PM object over {seen} stages: worst difference / pairing scale {worst:.3g}")
    assert seen >= 3


def test_zoom_ampm_cross_cab_cba_are_the_two_pair_recipe(pkg, gpu_required):
    """cab and cba against the only way to them before: a ZoomCsdCascade fed (a:+ftw, b:-ftw), phase0 = 0, whose S_ab upper is
    conj(Z_a[k] Z_b[kn]) and whose S_ab lower is conj(Z_a[kn] Z_b[k]).  Every stage, within 1e-5 of the pairing scale, the bound
    of test_zoom_ampm_comp_is_the_readme_recipe; the recipe's S_bb rows are this object's with upper and lower swapped."""
    n, m = 512, 1 << 19
    a = gaussian(m, 83)
    b = (0.6 * a + 0.8 * gaussian(m, 84)).astype(np.float32)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    g = make(pkg, n, (ftw, ftw))
    g.process(a, b)
    c = pkg.ZoomCsdCascade(n)
    c.set_carrier(ftw=ftw, side=0)
    c.set_carrier(ftw=(-ftw) & M64, side=1)
    c.process(a, b)
    assert g.num_stages() == c.num_stages() >= 4
    worst, seen = 0.0, 0
    for k in range(g.num_stages()):
        info, r = g.stage_rows(k)
        cinfo, rows = c.stage_spectra(k)
        assert info["count"] == cinfo["count"]
        if not info["count"]:
            continue
        seen += 1
        rows = rows.astype(np.float64)
        for mine, (u, v), theirs in ((8, PAIRING[8], rows[4] + 1j * rows[6]), (10, PAIRING[10], rows[5] + 1j * rows[7])):
            scale = np.sqrt(r[u] * r[v])
            err = np.abs(cplx(r, mine) - np.conj(theirs))
            worst = max(worst, float(np.max(err / scale)))
            assert np.all(err <= 1e-5 * scale), (k, mine, float(np.max(err / scale)))
        assert np.all(np.abs(r[2] - rows[3]) <= 1e-5 * r[2]) and np.all(np.abs(r[3] - rows[2]) <= 1e-5 * r[3]), k
    print(f"cab, cba against conj(S_ab) of the (+ftw, -ftw) recipe over {seen} stages: worst error / pairing scale {worst:.3g}")
    assert seen >= 3


def same_rows(a, b, tol, what=""):
    """tol 0: equal bits; else rows 0 ... 3 within tol relative and the complex rows within tol of the pairing scale, statistics equal"""
    assert len(a) == len(b), what
    for k, (ma, mb) in enumerate(zip(a, b)):
        assert ma[0] == mb[0], (what, k)
        if tol == 0:
            assert ma[1].tobytes() == mb[1].tobytes(), (what, k)
            continue
        if not mb[0]["count"]:
            continue
        for r in range(4):
            assert np.all(np.abs(ma[1][r] - mb[1][r]) <= tol * mb[1][r]), (what, k, r)
        for r, (u, v) in PAIRING.items():
            assert np.all(np.abs(cplx(ma[1], r) - cplx(mb[1], r)) <= tol * np.sqrt(mb[1][u] * mb[1][v])), (what, k, r)


CUTS = np.cumsum([0, 1000, 77_777, (1 << 20) + 3])


def test_zoom_ampm_cross_chunking_and_routes(pkg, gpu_required):
    """One call against calls of 1000, 77 777 and 2^20 + 3 samples, host and device: within 2e-6 of the pairing scale.  The same
    calls twice, host against device, reset and replay (after changing detrend and avg): equal bits."""
    import torch
    n = 512
    length = int(CUTS[-1])
    a, b = gaussian(length, 31), gaussian(length, 32)
    ftw = (pkg.zoom_ftw(0.2718281828459045)[0], pkg.zoom_ftw(0.6180339887498949)[0])
    ph = (0x0123456789ABCDEF, 1 << 62)
    new = lambda: make(pkg, n, ftw, phase0=ph)  # noqa: E731
    one = new()
    one.process(a, b)
    ref = stage_rows(one)
    h = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        h.process(a[s:e], b[s:e])
    got_h = stage_rows(h)
    same_rows(got_h, ref, 2e-6, "host chunks")
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    d = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(da.data_ptr() + 4 * int(s), db.data_ptr() + 4 * int(s), int(e - s))
    got_d = stage_rows(d)
    same_rows(got_d, ref, 2e-6, "device chunks")
    same_rows(got_d, got_h, 0, "host against device, same calls")
    one_d = new()
    one_d.process_device(da.data_ptr(), db.data_ptr(), length)
    same_rows(stage_rows(one_d), ref, 0, "host against device, one call")
    h2 = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        h2.process(a[s:e], b[s:e])
    same_rows(stage_rows(h2), got_h, 0, "same calls twice")
    sb_d = d.sidebands()
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()  # settings too; the single object's carriers are kept
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(da.data_ptr() + 4 * int(s), db.data_ptr() + 4 * int(s), int(e - s))
    same_rows(stage_rows(d), got_d, 0, "reset + replay")
    s2 = d.sidebands()
    assert s2[8] == sb_d[8] and all(u.tobytes() == v.tobytes() for u, v in zip(s2[:8], sb_d[:8]))
    assert d.stats_read()["pairs_in"] == length


def test_iq_ampm_cross_chunking_and_routes(pkg, gpu_required):
    """The same for the complex feed, and its routes: interleaved against planar and host against device give equal bits"""
    import torch
    n = 512
    length = int(CUTS[-1])
    p = [gaussian(length, 33 + c) for c in range(4)]  # I_a, Q_a, I_b, Q_b
    za, zb = (p[0] + 1j * p[1]).astype(np.complex64), (p[2] + 1j * p[3]).astype(np.complex64)
    f = pkg.zoom_ftw(0.2718281828459045)[0]
    new = lambda: make(pkg, n, (f, f), phase0=(0x0123456789ABCDEF, 5), cls=pkg.IqAmPmCsdCascade)  # noqa: E731
    one = new()
    one.process(za, zb)
    ref = stage_rows(one)
    h = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        h.process(za[s:e], zb[s:e])
    got_h = stage_rows(h)
    same_rows(got_h, ref, 2e-6, "host chunks")
    hp = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        hp.process((p[0][s:e], p[1][s:e]), (p[2][s:e], p[3][s:e]))
    same_rows(stage_rows(hp), got_h, 0, "interleaved against planar, host")
    dz = [torch.from_numpy(z).cuda() for z in (za, zb)]
    dp = [torch.from_numpy(v).cuda() for v in p]
    torch.cuda.synchronize()
    d, dpl = new(), new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz[0].data_ptr() + 8 * int(s), dz[1].data_ptr() + 8 * int(s), int(e - s))
        dpl.process_device_planar(*[t.data_ptr() + 4 * int(s) for t in dp], int(e - s))
    got_d = stage_rows(d)
    same_rows(got_d, got_h, 0, "host against device, same calls")
    same_rows(stage_rows(dpl), got_d, 0, "interleaved against planar, device")
    h2 = new()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        h2.process(za[s:e], zb[s:e])
    same_rows(stage_rows(h2), got_h, 0, "same calls twice")
    d.reset()  # the single object's reset keeps its carriers
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz[0].data_ptr() + 8 * int(s), dz[1].data_ptr() + 8 * int(s), int(e - s))
    same_rows(stage_rows(d), got_d, 0, "reset + replay")
    assert d.stats_read()["pairs_in"] == length


@pytest.mark.parametrize("family", ["zoom", "iq"])
def test_zoom_ampm_cross_bank(pkg, gpu_required, family):
    """Two pairs of a bank with different carriers and streams, fed in turn, equal two single objects bit for bit; pair 0 is
    unchanged after pair 1 is fed"""
    n = 256
    lens, step = [300_000, 123_457], [65_536, 33_333]
    car = [(pkg.zoom_ftw(0.2)[0], pkg.zoom_ftw(0.21)[0]), (pkg.zoom_ftw(0.75)[0], pkg.zoom_ftw(0.75)[0])]
    if family == "zoom":
        xs = [(gaussian(m, 400 + c), gaussian(m, 450 + c)) for c, m in enumerate(lens)]
        bank, single = pkg.ZoomAmPmCsdCascadeBank(n, 2), pkg.ZoomAmPmCsdCascade
    else:
        xs = [tuple((gaussian(m, 400 + c + 10 * s) + 1j * gaussian(m, 500 + c + 10 * s)).astype(np.complex64) for s in (0, 1))
              for c, m in enumerate(lens)]
        bank, single = pkg.IqAmPmCsdCascadeBank(n, 2), pkg.IqAmPmCsdCascade
    for c in range(2):
        for side in (0, 1):
            bank.set_carrier(c, ftw=car[c][side], side=side)
    singles = []
    for c, (x, y) in enumerate(xs):
        s = make(pkg, n, car[c], cls=single)
        for q in range(0, x.size, step[c]):
            bank.process(c, x[q:q + step[c]], y[q:q + step[c]])
            s.process(x[q:q + step[c]], y[q:q + step[c]])
        got = [bank.stage_rows(c, k) for k in range(bank.num_stages(c))]
        same_rows(got, stage_rows(s), 0, f"pair {c}")
        for u, v in zip(bank.sidebands(c), s.sidebands()):
            assert u.tobytes() == v.tobytes() if isinstance(u, np.ndarray) else u == v
        singles.append(stage_rows(s))
    same_rows([bank.stage_rows(0, k) for k in range(bank.num_stages(0))], singles[0], 0, "pair 0 afterwards")


# ---- the readings of tests/test_zoom_ampm_cross_host.py on the GPU: the same inputs, the same assertions ----

def gpu_stage0(pkg, ora, case):
    """(count, rows) of stage 0 of the object fed the property input; its count is the restatement's"""
    kind, v = xprop_input(pkg, case)
    if kind == "real":
        g = pkg.ZoomAmPmCsdCascade(PROP_N, f0=PROP_F0)
        g.process(*v)
    else:
        g = pkg.IqAmPmCsdCascade(PROP_N)
        g.process(v[0], v[1])  # two (i, q) pairs: the planar route
    info, rows = g.stage_rows(0)
    assert info["count"] == xprop_restatement(pkg, ora, case)["count"]
    return g, (info["count"], rows)


@pytest.mark.parametrize("case", ["common", "common_real"])
def test_zoom_ampm_cross_common_phase_noise(pkg, ora, gpu_required, case):
    """(a): s_pm within three times the restatement's margin of the common density, complex carriers and real ones at f0 = 0.2;
    am_pm_cross() with the carriers it reads itself is am_pm_cross_from_sidebands of the stage's rows"""
    g, rows = gpu_stage0(pkg, ora, case)
    check_common(pkg, *rows, f"gpu {case}", case)
    out = g.am_pm_cross(opts=pkg.MergeOpts(keep_overlap=True, keep_transition_band=True))
    b0 = [b for b in out[4] if b.decimation == 1][0]  # stage 0's bins in the merged read-out
    want = stage_am_pm_cross(pkg, PROP_N, *rows)
    assert g.carriers() == want[4] and want[4][3] > 1 - 1e-5 and want[4][4] > 1 - 1e-5
    from test_zoom_ampm_host import PROP_BINS
    sl = slice(b0.start + PROP_BINS.start - b0.bins.start, b0.start + PROP_BINS.stop - b0.bins.start)
    top = float(np.max(np.abs(want[1][PROP_BINS])))
    for got, w in zip(out[:4], want[:4]):
        assert got.dtype == np.complex128 and np.allclose(got[sl], w[PROP_BINS], rtol=1e-6, atol=1e-6 * top)


@pytest.mark.parametrize("case", ["delay", "delay_real"])
def test_zoom_ampm_cross_delay_fixes_the_sign(pkg, ora, gpu_required, case):
    """(b): phi_b[n] = phi_a[n - 3]: s_pm / S_phi within the restatement's margin rule of exp(-2 pi i 3 k / N)"""
    check_delay(pkg, *gpu_stage0(pkg, ora, case)[1], f"gpu {case}", case)


def test_zoom_ampm_cross_constant_carriers(pkg, ora, gpu_required):
    """(d): p_ab within 1e-5 relative, arg w and arg q within 1e-5 rad, both locks within 1e-5 of 1; carriers() is that reading;
    under a detrend and without an average it raises, and am_pm_cross() wants the carriers"""
    g, rows = gpu_stage0(pkg, ora, "const")
    car = check_const(pkg, *rows, "gpu const", 1e-5)
    assert g.carriers() == car
    d = pkg.IqAmPmCsdCascade(PROP_N)
    with pytest.raises(pkg.PsdError) as e:
        d.carriers()  # no average yet
    assert e.value.code == pkg.ERR_ARG
    d.set_detrend(pkg.Detrend.MEAN)
    d.process(*xprop_input(pkg, "const")[1])
    for call in (d.carriers, d.am_pm_cross):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "Detrend.NONE" in str(e.value)
    assert d.am_pm_cross(carriers=(0.4, np.exp(0.3j), np.exp(-1.1j)))[0].size == d.csd()[0].size


def test_zoom_ampm_cross_launches(pkg, gpu_required):
    """Eight steady device calls record the launches of ZoomCsdCascade for the same calls (2 + 3 a call: two mixers; segments,
    decimators, fold + tails) and of IqCsdCascade (1 + 3), with three live stages"""
    import torch
    n, m = 1024, 1 << 17
    da, db = torch.randn(m, device="cuda"), torch.randn(m, device="cuda")
    dz = [torch.randn(m, dtype=torch.complex64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    la = {}
    for name, g, args in (("zxampm", pkg.ZoomAmPmCsdCascade(n, f0=0.2), (da, db)), ("zcsd", pkg.ZoomCsdCascade(n, f0=0.2), (da, db)),
                          ("iqxampm", pkg.IqAmPmCsdCascade(n, f0=0.2), dz), ("iqcsd", pkg.IqCsdCascade(n, f0=0.2), dz)):
        for _ in range(8):
            g.process_device(args[0].data_ptr(), args[1].data_ptr(), m)
        g.stats_read(reset=True)
        for _ in range(8):
            g.process_device(args[0].data_ptr(), args[1].data_ptr(), m)
        la[name] = g.stats_read()["launches"]
        g.sync()
        assert g.num_stages() >= 3
        g.close()
    assert la["zxampm"] == la["zcsd"] == pkg.ZCSD_STEADY_LAUNCHES * 8 and la["iqxampm"] == la["iqcsd"] == pkg.IQCSD_STEADY_LAUNCHES * 8, la


@pytest.mark.parametrize("family", ["zxampm", "iqxampm"])
def test_zoom_ampm_cross_argument_errors_on_an_object(pkg, gpu_required, family):
    """Detrend::Linear, pair, side and stage out of range, null sample pointers, set_carrier after the first sample, capacity"""
    import ctypes as C
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    b = (pkg.ZoomAmPmCsdCascadeBank if family == "zxampm" else pkg.IqAmPmCsdCascadeBank)(256, 2)
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED and pre + "set_detrend" in str(e.value)
    x = np.zeros(1000, np.complex64 if family == "iqxampm" else np.float32)
    for call in (lambda: b.process(2, x, x), lambda: b.process_device(7, 4096, 4096, 10), lambda: b.num_stages(2),
                 lambda: b.sidebands(5), lambda: b.stage_rows(2, 0), lambda: b.set_carrier(2, f0=0.1)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "out of range (n_pairs 2)" in str(e.value) and pre[:-1] in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, f0=0.1, side=2)
    assert e.value.code == pkg.ERR_ARG
    assert getattr(L, pre + "set_carrier")(b._h, 0, 2, 1, 0) == pkg.ERR_ARG
    if family == "zxampm":
        one = np.zeros(4, np.float32)
        nulls = [L.psdc_zxampm_process(b._h, 0, pkg._fptr(one), None, 4), L.psdc_zxampm_process_device(b._h, 0, None, None, 4, None)]
    else:
        one = np.zeros(4, np.float32)
        nulls = [L.psdc_iqxampm_process(b._h, 0, pkg._fptr(one), None, pkg._fptr(one), pkg._fptr(one), 4),
                 L.psdc_iqxampm_process_device(b._h, 0, None, None, None, None, 4, None),
                 L.psdc_iqxampm_process_interleaved(b._h, 0, None, None, 4),
                 L.psdc_iqxampm_process_interleaved_device(b._h, 0, None, None, 4, None)]
    assert all(rc == pkg.ERR_ARG for rc in nulls), nulls
    with pytest.raises(pkg.PsdError) as e:
        b.stage_rows(0, 0)  # no sample yet: no stage
    assert e.value.code == pkg.ERR_ARG and pre + "stage_rows: stage 0 out of range" in str(e.value)
    sb = b.sidebands(0)
    assert all(a.size == 0 for a in sb[:8]) and sb[8] == []
    b.process(0, x, x)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    b.set_carrier(1, ftw=1)  # pair 1 has taken nothing yet
    info = b.stage_rows(0, 0)[0]
    assert info["count"] == 6 and b.stats_read()["pairs_in"] == 1000  # 1 + (1000 - 256) // 128 segments
    # an output too small for the merged rows, and no output: the length is still reported
    plen = C.c_size_t()
    small = np.empty(12 * 3, np.float64)
    f = getattr(L, pre + "sidebands")
    assert f(b._h, 0, 0, 1, 0, small.ctypes.data_as(C.POINTER(C.c_double)), 3, C.byref(plen), None, 0, None) == pkg.ERR_CAPACITY
    assert f(b._h, 0, 0, 1, 0, None, 0, C.byref(plen), None, 0, None) == 0 and plen.value == b.csd(0)[0].size
    b.close()


def test_zoom_ampm_cross_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --zoom-ampm-pair 0.2:raw:raw on a phase-modulated carrier at the tuning word: fed (x, x) the
    lines offset, then Re and Im of s_am, s_pm, s_am_pm, s_pm_am against the object's am_pm_cross() (one call here: the file is
    shorter than the tool's 2^20 samples a call), s_pm far above s_am in the band, and the carriers in the summary line"""
    from test_zoom_ampm_host import band_noise
    from test_zoom_host import phases
    fs = 1000.0
    length = (1 << 17) + 777
    f0 = 0.2
    ftw = pkg.zoom_ftw(f0)[0]
    w = 2.0 * np.pi * (phases(length, ftw).astype(np.float64) / 18446744073709551616.0)
    x = (np.cos(w + 0.4 + band_noise(1e-2, 41, length)) + 1e-6 * gaussian(length, 42)).astype(np.float32)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--raw", str(raw), "--zoom-ampm-pair", f"{f0}:raw:raw",
                        "--fs", str(fs), "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("zoom am/pm pair raw:raw @ 0.2")]
    assert len(line) == 1 and " lock_w " in line[0] and " lock_q " in line[0] and "p_ab " in line[0], r.stdout
    bank = pkg.ZoomAmPmCsdCascadeBank(512, 1)  # what the tool builds: no detrend (the carriers are read from bin 0), avg_max 1000
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.set_carrier(0, f0=f0)
    bank.process(0, x, x)
    out = bank.am_pm_cross(0, opts=pkg.MergeOpts(min_count=1))
    p_ab, cw, cq, lock_w, lock_q = bank.carriers(0)
    # x = cos(w + 0.4 + phi): both baseband carriers are 0.5 exp(0.4 i)
    assert abs(p_ab - 0.25) < 1e-3 and lock_w > 0.9999 and lock_q > 0.999 and abs(np.angle(cw)) < 1e-6 and abs(np.angle(cq * np.exp(-0.8j))) < 1e-3
    assert f"lock_w {lock_w:.9g}" in line[0] and f"lock_q {lock_q:.9g}" in line[0]
    d = np.loadtxt(tmp_path / "csv" / "zoomampmpair_raw__raw_0_2.csv", delimiter=",")
    assert d.shape == (out[0].size, 9)
    assert np.allclose(d[:, 0], np.asarray(pkg.Break.frequencies(out[4]), np.float64) * fs, rtol=1e-6, atol=0)
    top = float(np.max(np.abs(out[1])))
    for i, v in enumerate(out[:4]):
        assert np.allclose(d[:, 1 + 2 * i], v.real, rtol=1e-6, atol=1e-9 * top) and np.allclose(d[:, 2 + 2 * i], v.imag, rtol=1e-6, atol=1e-9 * top), i
    band = (d[:, 0] > 0.02 * fs) & (d[:, 0] < 0.08 * fs)
    print(f"band: {band.sum()} bins, median s_pm {np.median(d[band, 3]):.3g}, worst |s_am| / s_pm {np.max(np.abs(d[band, 1]) / d[band, 3]):.3g}")
    assert band.sum() > 10 and np.all(d[band, 3] > 100 * np.abs(d[band, 1]))
