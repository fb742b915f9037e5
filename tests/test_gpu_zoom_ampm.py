"""AM/PM cascades on the GPU (psdc_zampm_*, psdc_iqampm_*, csrc/zoom_ampm.hip) against the f64 restatement of
tests/test_zoom_ampm_host.py and its f32 sibling, against the zoom / IQ / zoom cross objects where the rows make them comparable,
and the readings of am_pm() and carrier() the restatement was shown to give there.  Semantics: include/psdcascade.h, "AM/PM
cascades"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ATOL_FRAC, assert_psd_close
from test_gpu_cross import DETRENDS, assert_sxy_close
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_sk_host import gaussian
from test_zoom_ampm_host import (PROP_F0, PROP_N, check_const, check_delay, check_indep, check_pm_only, prop_input,
                                 prop_restatement, restate_zoom_ampm)
from test_zoom_host import U32_MAX, carrier_ftw, emul, mix_f32, stitch_zoom, windows_of  # noqa: F401

pytestmark = pytest.mark.gpu

# (n, window, detrend, avg (limit, count) or None, carrier, length).  Hann hops n/2, the custom table 3n/4.
# Teams a workgroup (a tile is one segment a team): 32 at n = 64 (wave-level team sync, sixteen teams a wavefront), 2 at 1024 (a
# team is one wavefront); at 2048 one team of two wavefronts and at 4096 one of four (__syncthreads, the largest LDS).
# The lengths leave an odd count of stage-0 segments, a last tile with idle teams where a workgroup has several, and three live
# stages of which the deepest has five averages or more: n (8^2 + 8) + 37 samples leave ONE segment there, and one periodogram
# has bins at 1e-4 of its level (its values are exponentially distributed), where the error of ANY f32 transform -- relative to
# the stage's level -- is beyond 1e-5 of the bin.  The pure rule needs averaged bins; 200 n + 37 samples give 399, 48 and 5.
PARITY_CASES = [
    (64, "hann", "none", None, ("bin", 5), 64 * 401 + 5),
    (1024, "hann", "none", (3, U32_MAX), 0.2345678901234567, 1024 * 200 + 37),       # EWMA from the fifth segment of every stage
    (2048, "hann", "midpoint", None, 3 ** 0.5 / 7, 2048 * 200 + 37),
    (4096, "hann", "mean", (7, 64), 0.6180339887498949, 4096 * 200 + 37),             # limit 7 at stages 0 and 1, then 1
    (4096, "hann", "none", None, 0.7131313131313131, 4096 * 200 + 37),
    (2048, "custom", "none", (7, 64), 0.8660254037844386, 2048 * 201 + 37),           # hop 3n/4: 267 segments
    (1024, "hann", "mean", None, 0.1 * 2 ** 0.5, 1024 * 200 + 37),
    (64, "hann", "none", (3, U32_MAX), 0.2345678901234567, 64 * 3 + 5),               # 5 segments, fewer than the 32 teams
]

# (n, route, carrier, avg, detrend); Hann
IQ_PARITY_CASES = [
    (64, "interleaved", ("bin", 0), None, "none"),
    (1024, "planar", 0.2345678901234567, (7, 64), "mean"),
    (2048, "interleaved", 0.7131313131313131, None, "midpoint"),
    (4096, "planar", ("bin", 100), (3, U32_MAX), "none"),
]

CARRIER = 0.5 * np.exp(0.3j)  # the explicit carrier both sides of an am_pm() comparison are given


def stage_rows(g):
    return [g.stage_rows(k) for k in range(g.num_stages())]


def rel_err(got, ref):
    """the figure to print: the worst relative error (bins a detrend nulls: relative to the row's scale, as conftest.assert_psd_close)"""
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.max(np.abs(ref)) + 1e-300)))


def stitch64(pkg, n, pwin, stages, breaks):
    """(upper, lower, comp) of a restatement merged in f64 by the Breaks of its own f32 stitch: every selected bin times the f32
    factor PsdCascade::psd applies to its stage (1 / (gain decimation)), as psdc_zampm_sidebands does it"""
    wt = pwin if isinstance(pwin, pkg.WindowTable) else pkg.WindowTable._kind(n, pwin)
    out = {"upper": [], "lower": [], "comp": []}
    ns = len(stages)
    for i, b in enumerate(breaks):
        if not b.include:
            continue
        s = stages[ns - 1 - i]
        gain = np.float32((n // 2) * s["count"]) * np.float32(wt.nenbw) * np.float32(wt.power)
        gsc = float(np.float32(1.0) / (gain * np.float32(b.decimation)))
        for name in out:
            out[name].append(s[name][b.bins.start:b.bins.stop] * gsc)
    return tuple(np.concatenate(out[name]) if out[name] else np.zeros(0) for name in ("upper", "lower", "comp"))


def assert_parity(pkg, g, st64, st32, n, pwin, detrend, what):
    """the assertions of both parity tests: g against the f64 restatement st64, with the f32 sibling st32 as the yardstick of the
    widened bounds"""
    # 1. Breaks, counts, averages, pendings: exact
    up, lo, br = g.psd()
    rup, rlo, rbr = stitch_zoom(pkg, n, pwin, st64)
    assert br == rbr and g.num_stages() == len(st64)
    got = stage_rows(g)
    for k, (m, s) in enumerate(zip(got, st64)):
        assert (m[0]["count"], m[0]["avg"], m[0]["pending"]) == (s["count"], s["avg"], s["pending"]), k
    # 2. rows 0 and 1, merged, as test_zoom_parity holds them
    print(f"{what} merged: worst relative error upper {rel_err(up, rup):.3g} lower {rel_err(lo, rlo):.3g}")
    if detrend == "none":
        assert_psd_close(up, rup, f"{what} upper", pure=True)
        assert_psd_close(lo, rlo, f"{what} lower", pure=True)
    else:  # a detrend nulls bin 0 of both rows: the widened bound, held to the f32 sibling's own arithmetic there
        sup, slo, _ = stitch_zoom(pkg, n, pwin, st32)
        assert_psd_close(up, rup, f"{what} upper {detrend}", ref_f32=sup)
        assert_psd_close(lo, rlo, f"{what} lower {detrend}", ref_f32=slo)
    # 3. rows 2 and 3, merged as rows 0 and 1 are (the Breaks leave out the transition band of the decimated stages, where a bin
    #    holds 1e-4 of the stage's power and an f32 transform's error is relative to the stage's largest bin): within 1e-5
    #    sqrt(upper lower) of the restatement's -- the zoom cross test's rule for S_ab (one complex product a bin); under a
    #    detrend plus 1e-6 of the bound's mean, as that test widens it.  Stage 0 has no transition band: all its bins, raw rows.
    sup, slo, scomp, sbr = g.sidebands()
    r64 = stitch64(pkg, n, pwin, st64, br)
    assert_sxy_close(scomp, r64[2], r64[0], r64[1], 1e-5, f"{what} comp", atol_frac=0.0 if detrend == "none" else 1e-6)
    scale = np.sqrt(r64[0] * r64[1])
    worst = float(np.max(np.abs(scomp - r64[2]) / np.maximum(scale, 1e-9 * np.max(scale) + 1e-300))) if scale.size else 0.0
    print(f"{what} comp merged: worst error / sqrt(upper lower) {worst:.3g}")
    for k, (m, s) in enumerate(zip(got, st64)):
        if not s["count"]:
            assert not m[1].any() and not m[2].any() and not m[3].any()
    if st64[0]["count"]:
        m, s = got[0], st64[0]
        if detrend == "none":
            assert_psd_close(m[1], s["upper"], f"{what} upper stage 0", pure=True)
            assert_psd_close(m[2], s["lower"], f"{what} lower stage 0", pure=True)
        assert_sxy_close(m[3], s["comp"], s["upper"], s["lower"], 1e-5, f"{what} comp stage 0",
                         atol_frac=0.0 if detrend == "none" else 1e-6)
    # 4. sidebands(): f64, the Breaks of psd(), rows 0 and 1 psd()'s to f32 rounding, and every bin the stage's accumulator times the
    #    stage's factor
    assert sbr == br and sup.dtype == slo.dtype == np.float64 and scomp.dtype == np.complex128
    assert sup.size == slo.size == scomp.size == up.size
    f32r = 2.0 ** -23  # psd() rounds the row to f32 and then the product: 2^-24 each
    assert np.all(np.abs(sup - up) <= f32r * sup) and np.all(np.abs(slo - lo) <= f32r * slo)
    gst = [dict(count=m[0]["count"], upper=m[1], lower=m[2], comp=m[3]) for m in got]
    for a, b in zip((sup, slo, scomp), stitch64(pkg, n, pwin, gst, br)):
        assert a.tobytes() == b.astype(a.dtype).tobytes()
    # 5. am_pm() with the SAME explicit carrier on both sides: S_am and S_pm within 2e-5 (S_am + S_pm) of the restatement's: with
    #    P S_am = (U + L)/2 + Re D and |dU| <= 1e-5 U, |dL| <= 1e-5 L, |dD| <= 1e-5 sqrt(U L) <= 1e-5 (U + L)/2 the error is at most
    #    2e-5 (U + L)/2 / (2P) = 2e-5 (S_am + S_pm) / 2.  Under a detrend the rows' widened rule adds its absolute term, 1e-6 of
    #    the mean, for each of the three rows that enter.
    s_am, s_pm, s_x, abr = g.am_pm(carrier=CARRIER)
    assert abr == br and s_am.dtype == s_pm.dtype == np.float64 and s_x.dtype == np.complex128
    r_am, r_pm, _ = pkg.am_pm_from_sidebands(*stitch64(pkg, n, pwin, st64, br), CARRIER)
    tot = r_am + r_pm
    bound = 2e-5 * tot + (0.0 if detrend == "none" else 3 * ATOL_FRAC * np.mean(tot))
    e = max(float(np.max(np.abs(s_am - r_am) / bound)), float(np.max(np.abs(s_pm - r_pm) / bound)))
    print(f"{what} am_pm: worst error / bound {e:.3g}")
    assert e <= 1.0, (what, e)
    return br


def live_stages(st):
    return sum(1 for s in st if s["count"] > 0)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_zoom_ampm_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, avg, carrier, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    x = gaussian(length, 1000 + case)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.ZoomAmPmCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    g.process(x)
    st64 = restate_zoom_ampm(ora, x, n, ftw, 0, owin, detrend, avg)
    st32 = restate_zoom_ampm(ora, x, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_f32(emul, x, ftw)) if detrend != "none" else None
    if length > 40 * n:
        teams = max(1, 128 // (n // 16))
        hop = n - (pwin.overlap if isinstance(pwin, pkg.WindowTable) else n // 2)
        nseg = 1 + (length - n) // hop
        assert live_stages(st64) >= 3 and nseg % 2 == 1 and (teams == 1 or nseg % teams), (live_stages(st64), nseg, teams)
    br = assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"zoom ampm case {case}")
    # stages and Breaks are those of the zoom object fed x
    z = pkg.ZoomCascade(n, ftw=ftw, window=pwin)
    z.set_detrend(DETRENDS[detrend])
    z.set_avg(pkg.AvgOpts(*avg))
    z.process(x)
    assert z.psd()[2] == br and g.num_stages() == z.num_stages()


@pytest.mark.parametrize("case", range(len(IQ_PARITY_CASES)))
def test_iq_ampm_parity(pkg, ora, gpu_required, iq_emul, case):  # noqa: F811
    n, route, carrier, avg, detrend = IQ_PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, "hann")
    avg = avg or (U32_MAX, U32_MAX)
    length = n * 200 + 37 if n >= 1024 else n * 401 + 5
    i, q = gaussian(length, 2000 + case), gaussian(length, 3000 + case)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.IqAmPmCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    if route == "planar":
        g.process((i, q))
    else:
        g.process((i + 1j * q).astype(np.complex64))
    st64 = restate_zoom_ampm(ora, i, n, ftw, 0, owin, detrend, avg, "f64", iq=mix_c_f64(i, q, ftw))
    st32 = (restate_zoom_ampm(ora, i, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_c_f32(iq_emul, i, q, ftw))
            if detrend != "none" else None)
    assert live_stages(st64) >= 3
    assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"iq ampm case {case}")


def test_zoom_ampm_rows_0_1_are_the_zoom_objects(pkg, gpu_required):
    """psd() against ZoomCascade / IqCascade fed the same stream (N = 1024, 2^20 samples): equal Breaks and stage counts, 2e-6"""
    n, m = 1024, 1 << 20
    x, y = gaussian(m, 77), gaussian(m, 78)
    z = (x + 1j * y).astype(np.complex64)
    for name, new, old, feed in (("zoom", pkg.ZoomAmPmCascade(n, f0=0.2), pkg.ZoomCascade(n, f0=0.2), x),
                                 ("iq", pkg.IqAmPmCascade(n, f0=0.2), pkg.IqCascade(n, f0=0.2), z)):
        new.process(feed)
        old.process(feed)
        up, lo, br = new.psd()
        oup, olo, obr = old.psd()
        assert br == obr and new.num_stages() == old.num_stages() >= 4
        for k in range(new.num_stages()):
            assert new.stage_rows(k)[0] == old.stage_spectra(k)[0], (name, k)
        ru = assert_psd_close(up, oup, f"{name} ampm upper vs the zoom object", rtol=2e-6, pure=True)
        rl = assert_psd_close(lo, olo, f"{name} ampm lower vs the zoom object", rtol=2e-6, pure=True)
        print(f"{name}: psd() against the two-row object, worst relative difference upper {ru:.3g} lower {rl:.3g}")


def test_zoom_ampm_comp_is_the_readme_recipe(pkg, gpu_required):
    """comp against the only way to it before: a ZoomCsdCascade fed (x, x) with carriers (+ftw, -ftw), phase0 = 0, whose S_ab upper
    is conj(Z_k Z_-k).  Every stage: comp within 1e-5 sqrt(upper lower) of conj(S_ab upper); its S_aa rows are upper and lower."""
    n, m = 512, 1 << 19
    x = gaussian(m, 81)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    g = pkg.ZoomAmPmCascade(n, ftw=ftw)
    g.process(x)
    c = pkg.ZoomCsdCascade(n)
    c.set_carrier(ftw=ftw, side=0)
    c.set_carrier(ftw=(-ftw) % (1 << 64), side=1)
    c.process(x, x)
    assert g.num_stages() == c.num_stages() >= 4
    worst, seen = 0.0, 0
    for k in range(g.num_stages()):
        info, up, lo, comp = g.stage_rows(k)
        cinfo, rows = c.stage_spectra(k)
        assert info["count"] == cinfo["count"]
        if not info["count"]:
            continue
        seen += 1
        scale = np.sqrt(up * lo)
        err = np.abs(comp - np.conj(rows[4].astype(np.float64) + 1j * rows[6]))
        worst = max(worst, float(np.max(err / scale)))
        assert np.all(err <= 1e-5 * scale), (k, float(np.max(err / scale)))
        assert np.all(np.abs(up - rows[0]) <= 1e-5 * up) and np.all(np.abs(lo - rows[1]) <= 1e-5 * lo), k
    print(f"comp against conj(S_ab upper) of the (x, x) recipe over {seen} stages: worst error / sqrt(upper lower) {worst:.3g}")
    assert seen >= 3


def same_rows(a, b, tol, what=""):
    """tol 0: equal bits; else rows 0 and 1 within tol relative and comp within tol sqrt(upper lower), statistics equal"""
    assert len(a) == len(b), what
    for k, (ma, mb) in enumerate(zip(a, b)):
        assert ma[0] == mb[0], (what, k)
        if tol == 0:
            for u, v in zip(ma[1:], mb[1:]):
                assert u.tobytes() == v.tobytes(), (what, k)
        else:
            for u, v in zip(ma[1:3], mb[1:3]):
                assert np.all(np.abs(u - v) <= tol * v), (what, k, rel_err(u, v))
            assert np.all(np.abs(ma[3] - mb[3]) <= tol * np.sqrt(mb[1] * mb[2])), (what, k)


CUTS = np.cumsum([0, 1000, 77_777, (1 << 20) + 3])


def test_zoom_ampm_chunking_and_routes(pkg, gpu_required):
    """One call against calls of 1000, 77 777 and 2^20 + 3 samples, host and device: rows 0 and 1 within 2e-6, rows 2 and 3 within
    2e-6 sqrt(upper lower).  The same calls twice, host against device, reset and replay (after changing detrend and avg): equal
    bits."""
    import torch
    n = 512
    length = int(CUTS[-1])
    x = gaussian(length, 31)
    ftw, ph0 = pkg.zoom_ftw(0.2718281828459045)[0], 0x0123456789ABCDEF
    make = lambda: pkg.ZoomAmPmCascade(n, ftw=ftw, phase0=ph0)  # noqa: E731
    one = make()
    one.process(x)
    ref = stage_rows(one)
    a = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a.process(x[s:e])
    got_a = stage_rows(a)
    same_rows(got_a, ref, 2e-6, "host chunks")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    d = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    got_d = stage_rows(d)
    same_rows(got_d, ref, 2e-6, "device chunks")
    same_rows(got_d, got_a, 0, "host against device, same calls")
    one_d = make()
    one_d.process_device(dx.data_ptr(), length)
    same_rows(stage_rows(one_d), ref, 0, "host against device, one call")
    a2 = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a2.process(x[s:e])
    same_rows(stage_rows(a2), got_a, 0, "same calls twice")
    psd_d, sb_d = d.psd(), d.sidebands()
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()  # settings too; the single object's carrier is kept
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    same_rows(stage_rows(d), got_d, 0, "reset + replay")
    p2, s2 = d.psd(), d.sidebands()
    assert p2[2] == psd_d[2] and all(u.tobytes() == v.tobytes() for u, v in zip(p2[:2] + s2[:3], psd_d[:2] + sb_d[:3]))
    assert d.stats()["samples_in"] == length


def test_iq_ampm_chunking_and_routes(pkg, gpu_required):
    """The same for the complex feed, and its routes: interleaved against planar and host against device give equal bits"""
    import torch
    n = 512
    length = int(CUTS[-1])
    i, q = gaussian(length, 32), gaussian(length, 33)
    z = (i + 1j * q).astype(np.complex64)
    make = lambda: pkg.IqAmPmCascade(n, f0=0.2718281828459045, phase0=0x0123456789ABCDEF)  # noqa: E731
    one = make()
    one.process(z)
    ref = stage_rows(one)
    a = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a.process(z[s:e])
    got_a = stage_rows(a)
    same_rows(got_a, ref, 2e-6, "host chunks")
    p = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        p.process((i[s:e], q[s:e]))
    same_rows(stage_rows(p), got_a, 0, "interleaved against planar, host")
    dz, di, dq = torch.from_numpy(z).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    d = make()
    dp = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz.data_ptr() + 8 * int(s), int(e - s))
        dp.process_device_planar(di.data_ptr() + 4 * int(s), dq.data_ptr() + 4 * int(s), int(e - s))
    got_d = stage_rows(d)
    same_rows(got_d, got_a, 0, "host against device, same calls")
    same_rows(stage_rows(dp), got_d, 0, "interleaved against planar, device")
    one_d = make()
    one_d.process_device(dz.data_ptr(), length)
    same_rows(stage_rows(one_d), ref, 0, "host against device, one call")
    a2 = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a2.process(z[s:e])
    same_rows(stage_rows(a2), got_a, 0, "same calls twice")
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz.data_ptr() + 8 * int(s), int(e - s))
    same_rows(stage_rows(d), got_d, 0, "reset + replay")
    assert d.stats()["samples_in"] == length


@pytest.mark.parametrize("family", ["zoom", "iq"])
def test_zoom_ampm_bank(pkg, gpu_required, family):
    """Two channels of a bank with different carriers and streams, fed in turn, equal two single objects bit for bit (each channel
    fed and read out in turn, so that its rounds are its single object's); channel 0 is unchanged after channel 1 is fed"""
    n = 256
    lens, step = [300_000, 123_457], [65_536, 33_333]
    car = [pkg.zoom_ftw(f)[0] for f in (0.2, 0.75)]
    ph = [12345, 1 << 63]
    if family == "zoom":
        xs = [gaussian(m, 400 + c) for c, m in enumerate(lens)]
        bank, single = pkg.ZoomAmPmCascadeBank(n, 2), pkg.ZoomAmPmCascade
    else:
        xs = [(gaussian(m, 400 + c) + 1j * gaussian(m, 500 + c)).astype(np.complex64) for c, m in enumerate(lens)]
        bank, single = pkg.IqAmPmCascadeBank(n, 2), pkg.IqAmPmCascade
    for c in range(2):
        bank.set_carrier(c, ftw=car[c], phase0=ph[c])
    singles = []
    for c, x in enumerate(xs):
        s = single(n, ftw=car[c], phase0=ph[c])
        for p in range(0, x.size, step[c]):
            bank.process(c, x[p:p + step[c]])
            s.process(x[p:p + step[c]])
        got = [bank.stage_rows(c, k) for k in range(bank.num_stages(c))]
        same_rows(got, stage_rows(s), 0, f"channel {c}")
        for a, b in zip(bank.psd(c) + bank.sidebands(c) + bank.am_pm(c, carrier=CARRIER), s.psd() + s.sidebands() + s.am_pm(carrier=CARRIER)):
            assert a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
        singles.append(stage_rows(s))
    same_rows([bank.stage_rows(0, k) for k in range(bank.num_stages(0))], singles[0], 0, "channel 0 afterwards")


# ---- the readings of tests/test_zoom_ampm_host.py on the GPU: the same inputs, the same assertions ----

def gpu_stage0(pkg, ora, case):
    """(count, upper, lower, comp) of stage 0 of the object fed the property input; its count is the restatement's"""
    kind, v = prop_input(pkg, case)
    g = pkg.ZoomAmPmCascade(PROP_N, f0=PROP_F0) if kind == "real" else pkg.IqAmPmCascade(PROP_N)
    g.process(v)
    info, up, lo, comp = g.stage_rows(0)
    assert info["count"] == prop_restatement(pkg, ora, case)["count"]
    return g, (info["count"], up, lo, comp)


@pytest.mark.parametrize("case", ["indep", "indep_real"])
def test_zoom_ampm_independent_modulations(pkg, ora, gpu_required, case):
    """(a): S_am and S_pm within 8 / sqrt(count) of 2 sigma^2, a complex carrier and a real one at f0 = 0.2; am_pm() with the
    carrier it reads itself is am_pm_from_sidebands of the stage's rows"""
    g, rows = gpu_stage0(pkg, ora, case)
    check_indep(pkg, *rows, f"gpu {case}")
    s_am, s_pm, s_x, br = g.am_pm(opts=pkg.MergeOpts(keep_overlap=True, keep_transition_band=True))
    b0 = [b for b in br if b.decimation == 1][0]  # stage 0's bins in the merged read-out
    power, u, lock = g.carrier()
    assert lock > 1 - 1e-5
    from test_zoom_ampm_host import PROP_BINS, stage_am_pm
    w_am, w_pm, w_x, _ = stage_am_pm(pkg, PROP_N, *rows)
    sl = slice(b0.start + PROP_BINS.start - b0.bins.start, b0.start + PROP_BINS.stop - b0.bins.start)
    assert np.allclose(s_am[sl], w_am[PROP_BINS], rtol=1e-6, atol=0) and np.allclose(s_pm[sl], w_pm[PROP_BINS], rtol=1e-6, atol=0)
    assert np.allclose(s_x[sl], w_x[PROP_BINS], rtol=1e-6, atol=1e-6 * float(np.max(np.abs(w_x[PROP_BINS]))))


def test_zoom_ampm_delayed_pm_fixes_the_sign(pkg, ora, gpu_required):
    """(b): phi[n] = 2 a[n - 3]: s_ampm / s_am within 5e-3 of 2 exp(-2 pi i 3 k / N)"""
    check_delay(pkg, *gpu_stage0(pkg, ora, "delay")[1], "gpu delay")


def test_zoom_ampm_pm_only(pkg, ora, gpu_required):
    """(d): S_am <= 1e-5 S_pm"""
    check_pm_only(pkg, *gpu_stage0(pkg, ora, "pm")[1], "gpu pm")


def test_zoom_ampm_constant_carrier(pkg, ora, gpu_required):
    """(e): |A|^2 within 1e-5 relative, the angle within 1e-5 rad, lock >= 1 - 1e-5; carrier() is that reading; under a detrend it
    raises and am_pm() wants the carrier"""
    g, rows = gpu_stage0(pkg, ora, "const")
    power, u, lock = check_const(pkg, *rows, "gpu const", 1e-5, 1e-5, 1e-5)
    assert g.carrier() == (power, u, lock)
    d = pkg.IqAmPmCascade(PROP_N)
    with pytest.raises(pkg.PsdError) as e:
        d.carrier()  # no average yet
    assert e.value.code == pkg.ERR_ARG
    d.set_detrend(pkg.Detrend.MEAN)
    d.process(prop_input(pkg, "const")[1])
    for call in (d.carrier, d.am_pm):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "Detrend.NONE" in str(e.value)
    assert d.am_pm(carrier=CARRIER)[0].size == d.psd()[0].size


def test_zoom_ampm_launches(pkg, gpu_required):
    """After warm-up to ten live stages (as test_zoom_sk_launches warms) 8 steady device calls record what ZoomCascade records for
    the same calls: 1 + 3 launches a call (mixer; segments, decimators, fold + tails): 32"""
    import torch
    n = 512
    m = 1 << 24
    dx = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    la = {}
    for name, g in (("zampm", pkg.ZoomAmPmCascade(n, f0=0.2)), ("zoom", pkg.ZoomCascade(n, f0=0.2))):
        for _ in range(760):  # 1.3e10 samples: stage 9 takes its first ones after 1.0e10
            g.process_device(dx.data_ptr(), m)
        g.stats_read(reset=True)
        for _ in range(8):
            g.process_device(dx.data_ptr(), m)
        la[name] = g.stats_read()["launches"]
        g.sync()
        assert g.num_stages() >= 10
        g.close()
    assert la["zampm"] == la["zoom"] == 4 * 8, la


@pytest.mark.parametrize("family", ["zampm", "iqampm"])
def test_zoom_ampm_argument_errors_on_an_object(pkg, gpu_required, family):
    """Detrend::Linear, channel and stage out of range, null sample pointers, set_carrier after the first sample"""
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    b = (pkg.ZoomAmPmCascadeBank if family == "zampm" else pkg.IqAmPmCascadeBank)(256, 2)
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED and pre + "set_detrend" in str(e.value)  # as the zoom object refuses it
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(9)
    assert e.value.code == pkg.ERR_ARG
    x = np.zeros(1000, np.complex64 if family == "iqampm" else np.float32)
    for call in (lambda: b.process(2, x), lambda: b.process_device(7, 4096, 10), lambda: b.num_stages(2), lambda: b.psd(2),
                 lambda: b.sidebands(5), lambda: b.stage_rows(2, 0), lambda: b.set_carrier(2, f0=0.1)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "out of range (n_channels 2)" in str(e.value) and pre[:-1] in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, f0=0.1, ftw=5)
    assert e.value.code == pkg.ERR_ARG
    if family == "zampm":
        nulls = {"process": L.psdc_zampm_process(b._h, 0, None, 4), "process_device": L.psdc_zampm_process_device(b._h, 0, None, 4, None)}
        assert L.psdc_zampm_process(b._h, 0, None, 0) == 0  # nothing to read
    else:
        one = np.zeros(4, np.float32)
        nulls = {"process": L.psdc_iqampm_process(b._h, 0, pkg._fptr(one), None, 4),
                 "process_device": L.psdc_iqampm_process_device(b._h, 0, None, None, 4, None),
                 "process_interleaved": L.psdc_iqampm_process_interleaved(b._h, 0, None, 4),
                 "process_interleaved_device": L.psdc_iqampm_process_interleaved_device(b._h, 0, None, 4, None)}
    for name, rc in nulls.items():
        assert rc == pkg.ERR_ARG, name
    assert "null" in getattr(L, pre + "last_error")(b._h).decode()
    with pytest.raises(pkg.PsdError) as e:
        b.stage_rows(0, 0)  # no sample yet: no stage
    assert e.value.code == pkg.ERR_ARG and pre + "stage_rows: stage 0 out of range" in str(e.value)
    up, lo, br = b.psd(0)
    su, sl, sc, br2 = b.sidebands(0)
    assert up.size == lo.size == su.size == sl.size == sc.size == 0 and br == br2 == []
    b.process(0, x)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    b.set_carrier(1, ftw=1)  # channel 1 has taken nothing yet
    info = b.stage_rows(0, 0)[0]
    assert info["count"] == 6 and b.stats_read()["samples_in"] == 1000  # 1 + (1000 - 256) // 128 segments
    ns = b.num_stages(0)  # (stage 1 exists already: 1000 samples put 90 decimated ones behind the drain)
    with pytest.raises(pkg.PsdError) as e:
        b.stage_rows(0, ns)
    assert e.value.code == pkg.ERR_ARG and f"stage {ns} out of range ({ns} stages)" in str(e.value)
    # an output too small for the merged rows, and any output NULL: the length is still reported
    import ctypes as C
    plen = C.c_size_t()
    small = np.empty(3, np.float64)
    dp = C.POINTER(C.c_double)
    f = getattr(L, pre + "sidebands")
    assert f(b._h, 0, 0, 1, 0, small.ctypes.data_as(dp), None, None, None, 3, C.byref(plen), None, 0, None) == pkg.ERR_CAPACITY
    assert f(b._h, 0, 0, 1, 0, None, None, None, None, 0, C.byref(plen), None, 0, None) == 0 and plen.value == b.psd(0)[0].size
    b.close()


def test_zoom_ampm_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --zoom-ampm 0.2 on a carrier at the tuning word with band-limited amplitude noise far above its
    phase noise: the lines offset, S_am, S_pm, Re and Im S_ampm against the object's am_pm() (one call here: the file is shorter
    than the tool's 2^20 samples a call), S_am far above S_pm in the band, and the carrier in the summary line"""
    from test_zoom_ampm_host import band_noise
    from test_zoom_host import phases
    fs = 1000.0
    length = (1 << 17) + 777
    f0 = 0.2
    ftw = pkg.zoom_ftw(f0)[0]
    w = 2.0 * np.pi * (phases(length, ftw).astype(np.float64) / 18446744073709551616.0)
    x = ((1.0 + band_noise(1e-2, 41, length)) * np.cos(w + 0.4) + 1e-6 * gaussian(length, 42)).astype(np.float32)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--raw", str(raw), "--zoom-ampm", str(f0), "--fs", str(fs),
                        "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("zoom am/pm raw @ 0.2")]
    assert len(line) == 1 and " lock " in line[0] and "carrier power " in line[0], r.stdout
    bank = pkg.ZoomAmPmCascadeBank(512, 1)  # what the tool builds: no detrend (the carrier is read from bin 0), avg_max 1000
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.set_carrier(0, f0=f0)
    bank.process(0, x)
    s_am, s_pm, s_x, br = bank.am_pm(0, opts=pkg.MergeOpts(min_count=1))
    power, u, lock = bank.carrier(0)
    # x = (1 + a) cos(w + 0.4): the baseband carrier is 0.5 exp(0.4 i)
    assert abs(power - 0.25) < 1e-3 and lock > 0.9999 and abs(0.5 * np.angle(u * np.exp(-0.8j))) < 1e-3
    assert f"lock {lock:.9g}" in line[0]
    d = np.loadtxt(tmp_path / "csv" / "zoomampm_raw_0_2.csv", delimiter=",")
    assert d.shape == (s_am.size, 5)
    assert np.allclose(d[:, 0], np.asarray(pkg.Break.frequencies(br), np.float64) * fs, rtol=1e-6, atol=0)
    for col, v in zip((1, 2, 3, 4), (s_am, s_pm, s_x.real, s_x.imag)):
        assert np.allclose(d[:, col], v, rtol=1e-6, atol=1e-9 * float(np.max(np.abs(v)))), col
    band = (d[:, 0] > 0.02 * fs) & (d[:, 0] < 0.08 * fs)
    print(f"band: {band.sum()} bins, median S_am {np.median(d[band, 1]):.3g}, worst |S_pm| / S_am {np.max(np.abs(d[band, 2]) / d[band, 1]):.3g}")
    assert band.sum() > 10 and np.all(d[band, 1] > 100 * np.abs(d[band, 2]))
