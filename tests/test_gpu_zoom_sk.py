"""Zoom and IQ spectral kurtosis cascades on the GPU (psdc_zsk_*, psdc_iqsk_*, csrc/zoom_sk.hip) against the f64 restatement of
tests/test_zoom_sk_host.py and its f32 sibling, against the zoom / IQ / spectral kurtosis objects where the rows make them
comparable, and the statistical properties the restatement was shown to have there.  Semantics: include/psdcascade.h, "zoom and
IQ spectral kurtosis cascades"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_sk_host import gaussian
from test_zoom_host import U32_MAX, carrier_ftw, emul, mix_f32, stitch_zoom, windows_of  # noqa: F401
from test_zoom_sk_host import (PROP_F0, PROP_N, check_circular, check_real, check_tone, prop_input, prop_restatement,
                               restate_zoom_sk)

pytestmark = pytest.mark.gpu

ROWS = ("upper", "lower", "s2_upper", "s2_lower")

# (n, window, detrend, avg (limit, count) or None, carrier, length -- or the lengths of the calls the stream is fed in).
# Hann hops n/2, the rectangular window n, the custom table 3n/4.
# Teams a workgroup (a tile is one segment a team): 32 at n = 64, 8 at 256, 2 at 1024; at 2048 one team of two wavefronts, at 4096
# one of four.
PARITY_CASES = [
    (64, "hann", "none", None, ("bin", 5), 200 * 64),
    (256, "rect", "mean", None, 0.2345678901234567, 200 * 256 + 17),
    (1024, "custom", "span", (3, U32_MAX), 0.7131313131313131, 200 * 1024),   # EWMA from the fifth segment of every stage
    (4096, "hann", "midpoint", (7, 64), 0.6180339887498949, 200 * 4096),       # limit 7 at stages 0 and 1, then 1, then 0
    (64, "hann", "none", (3, U32_MAX), ("bin", 5), 64),                        # exactly one segment
    (64, "rect", "span", (7, 64), 0.1 * 2 ** 0.5, 5 * 64),                     # 5 segments, fewer than the 32 teams
    (256, "hann", "midpoint", (7, 64), 0.2345678901234567, 256 + 5 * 128),     # 6 segments, fewer than the 8 teams
    (1024, "hann", "mean", (7, 64), 0.8660254037844386, 200 * 1024 + 511),     # 399 segments, odd, over 2 teams; EWMA starts inside
    (2048, "hann", "none", None, 3 ** 0.5 / 7, 50 * 2048),
    (4096, "hann", "mean", (3, U32_MAX), 0.6180339887498949, 3 * 4096),        # 5 segments
    (1024, "rect", "none", (7, 64), ("bin", 37), (1024, 8 * 1024)),            # boxcar -> EWMA across calls
    (256, "hann", "none", (3, U32_MAX), 0.7131313131313131, (256, 4 * 128, 40_000)),
]

# (n, route, carrier, avg); Hann; the second under Detrend::Mean (the widened rule and its f32 sibling), the others without a detrend
IQ_PARITY_CASES = [
    (64, "interleaved", ("bin", 0), None, "none"),
    (1024, "planar", 0.2345678901234567, (7, 64), "mean"),
    (4096, "interleaved", ("bin", 100), None, "none"),
]


def moments(g):
    return [g.stage_moments(k) for k in range(g.num_stages())]


def sk_by_breaks(pkg, g, breaks):
    """the merged SK rows written out from the stage moments and the Breaks: Break i is stage ns - 1 - i"""
    ns = g.num_stages()
    up, lo = [], []
    for i, b in enumerate(breaks):
        if not b.include:
            continue
        info, u1, l1, u2, l2 = g.stage_moments(ns - 1 - i)
        assert info["count"] == b.count
        up.append(pkg.sk_from_moments(info["count"], u1, u2)[b.bins.start:b.bins.stop])
        lo.append(pkg.sk_from_moments(info["count"], l1, l2)[b.bins.start:b.bins.stop])
    return (np.concatenate(up), np.concatenate(lo)) if up else (np.zeros(0), np.zeros(0))


def rel_err(got, ref):
    """the figure to print: the worst relative error (bins a detrend nulls: relative to the row's scale, as conftest.assert_psd_close)"""
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * np.max(np.abs(ref)) + 1e-300)))


def assert_parity(pkg, g, st64, st32, n, pwin, detrend, what):
    """the assertions of both parity tests: g against the f64 restatement st64, with the f32 sibling st32 as the yardstick of the
    widened bounds"""
    # 1. Breaks, counts, averages, pendings: exact
    up, lo, br = g.psd()
    rup, rlo, rbr = stitch_zoom(pkg, n, pwin, st64)
    assert br == rbr and g.num_stages() == len(st64)
    got = moments(g)
    for k, (m, s) in enumerate(zip(got, st64)):
        assert (m[0]["count"], m[0]["avg"], m[0]["pending"]) == (s["count"], s["avg"], s["pending"]), k
    # 2. rows 0 and 1, merged, as test_zoom_parity holds them
    print(f"{what} merged S1: worst relative error upper {rel_err(up, rup):.3g} lower {rel_err(lo, rlo):.3g}")
    if detrend == "none":
        assert_psd_close(up, rup, f"{what} upper", pure=True)
        assert_psd_close(lo, rlo, f"{what} lower", pure=True)
    else:  # a detrend nulls bin 0 of both rows: the widened bound, held to the f32 sibling's own arithmetic there
        sup, slo, _ = stitch_zoom(pkg, n, pwin, st32)
        assert_psd_close(up, rup, f"{what} upper {detrend}", ref_f32=sup)
        assert_psd_close(lo, rlo, f"{what} lower {detrend}", ref_f32=slo)
    # 3. rows 2 and 3, stage by stage, rtol 2e-5 (squaring doubles the relative error), held to the f32 sibling
    for k, (m, s, s32) in enumerate(zip(got, st64, st32)):
        if s["count"]:
            print(f"{what} stage {k} count {s['count']}: worst relative error " +
                  " ".join(f"{name} {rel_err(m[1 + r], s[name]):.3g}" for r, name in enumerate(ROWS)))
        assert_psd_close(m[3], s["s2_upper"], f"{what} s2_upper stage {k}", rtol=2e-5, ref_f32=s32["s2_upper"])
        assert_psd_close(m[4], s["s2_lower"], f"{what} s2_lower stage {k}", rtol=2e-5, ref_f32=s32["s2_lower"])
    # 4. SK wherever both moments met their pure bounds: dR / R <= e2 + 2 e1 = 4e-5 with R = M S2 / S1^2; NaN below two averages
    worst = 0.0
    for k, (m, s) in enumerate(zip(got, st64)):
        c = s["count"]
        for side, (g1, g2, r1, r2) in enumerate(((m[1], m[3], s["upper"], s["s2_upper"]), (m[2], m[4], s["lower"], s["s2_lower"]))):
            if c < 2:
                assert np.all(np.isnan(pkg.sk_from_moments(c, g1, g2)))
                continue
            ok = (np.abs(g1 - r1) <= 1e-5 * r1) & (np.abs(g2 - r2) <= 2e-5 * r2) & (r1 > 0)
            sk_g, sk_r = pkg.sk_from_moments(c, g1, g2)[ok], pkg.sk_from_moments(c, r1, r2)[ok]
            bound = 4e-5 * (sk_r + (c + 1.0) / (c - 1.0))
            if ok.any():
                worst = max(worst, float(np.max(np.abs(sk_g - sk_r) / bound)))
            assert np.all(np.abs(sk_g - sk_r) <= bound), (k, side, float(np.max(np.abs(sk_g - sk_r) / bound)))
    print(f"{what} SK: worst |SK_gpu - SK_f64| / bound {worst:.3g}")
    # 5. the merged SK is the stages' SK, selected by the Breaks of psd(): exactly, NaNs included
    sup, slo, sbr = g.sk()
    assert sbr == br and sup.dtype == slo.dtype == np.float64 and sup.size == slo.size == up.size
    wup, wlo = sk_by_breaks(pkg, g, br)
    assert np.array_equal(sup, wup, equal_nan=True) and np.array_equal(slo, wlo, equal_nan=True)
    for b in br:
        if b.include and b.count < 2:
            assert np.all(np.isnan(sup[b.start:b.start + b.bins.stop - b.bins.start]))
    return br


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_zoom_sk_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, avg, carrier, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    calls = length if isinstance(length, tuple) else (length,)
    length = sum(calls)
    x = gaussian(length, 1000 + case)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.ZoomSkCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    for s, e in zip(np.cumsum((0,) + calls[:-1]), np.cumsum(calls)):
        g.process(x[s:e])
    st64 = restate_zoom_sk(ora, x, n, ftw, 0, owin, detrend, avg)
    st32 = restate_zoom_sk(ora, x, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_f32(emul, x, ftw))
    if length >= 200 * n:
        assert sum(1 for s in st64 if s["count"] > 0) >= 3
    br = assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"zoom sk case {case}")
    # stages and Breaks are those of the auto-PSD object fed x
    b = pkg.PsdCascadeBank(n, 1, pwin)
    b.set_detrend(DETRENDS[detrend])
    b.set_avg(pkg.AvgOpts(*avg))
    b.process(0, x)
    _, bbr = b.psd(0)
    assert bbr == br and g.num_stages() == b.num_stages(0)


@pytest.mark.parametrize("case", range(len(IQ_PARITY_CASES)))
def test_iq_sk_parity(pkg, ora, gpu_required, iq_emul, case):  # noqa: F811
    n, route, carrier, avg, detrend = IQ_PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, "hann")
    avg = avg or (U32_MAX, U32_MAX)
    length = 200 * n
    i, q = gaussian(length, 2000 + case), gaussian(length, 3000 + case)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.IqSkCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    if route == "planar":
        g.process((i, q))
    else:
        g.process((i + 1j * q).astype(np.complex64))
    st64 = restate_zoom_sk(ora, i, n, ftw, 0, owin, detrend, avg, "f64", iq=mix_c_f64(i, q, ftw))
    st32 = restate_zoom_sk(ora, i, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_c_f32(iq_emul, i, q, ftw))
    assert sum(1 for s in st64 if s["count"] > 0) >= 3
    assert_parity(pkg, g, st64, st32, n, pwin, detrend, f"iq sk case {case}")


def test_zoom_sk_rows_0_1_are_the_zoom_objects(pkg, gpu_required):
    """psd() against ZoomCascade / IqCascade fed the same stream (N = 1024, 2^20 samples): equal Breaks and stage counts, pure 1e-5"""
    n, m = 1024, 1 << 20
    x, y = gaussian(m, 77), gaussian(m, 78)
    z = (x + 1j * y).astype(np.complex64)
    for name, new, old, feed in (("zoom", pkg.ZoomSkCascade(n, f0=0.2), pkg.ZoomCascade(n, f0=0.2), x),
                                 ("iq", pkg.IqSkCascade(n, f0=0.2), pkg.IqCascade(n, f0=0.2), z)):
        new.process(feed)
        old.process(feed)
        up, lo, br = new.psd()
        oup, olo, obr = old.psd()
        assert br == obr and new.num_stages() == old.num_stages() >= 4
        for k in range(new.num_stages()):
            assert new.stage_moments(k)[0] == old.stage_spectra(k)[0], (name, k)
        ru = assert_psd_close(up, oup, f"{name} sk upper vs the first-moment object", pure=True)
        rl = assert_psd_close(lo, olo, f"{name} sk lower vs the first-moment object", pure=True)
        print(f"{name}: psd() against the first-moment object, worst relative difference upper {ru:.3g} lower {rl:.3g}")


def test_iq_sk_fed_a_real_stream_is_the_sk_object(pkg, gpu_required):
    """IqSkCascade(ftw = 0) fed (x, 0) against SkCascade fed x (N = 512): at every stage with count > 0 both upper and lower hold
    s1 within 1e-5 of its s1 and s2 within 2e-5 of its s2"""
    n = 512
    x = gaussian(1 << 20, 79)
    g = pkg.IqSkCascade(n)
    g.process((x, np.zeros_like(x)))
    s = pkg.SkCascade(n)
    s.process(x)
    assert g.num_stages() == s.num_stages() >= 4
    w1 = w2 = 0.0
    seen = 0
    for k in range(g.num_stages()):
        info, u1, l1, u2, l2 = g.stage_moments(k)
        sinfo, s1, s2 = s.stage_moments(k)
        assert (info["count"], info["pending"]) == (sinfo["count"], sinfo["pending"]), k
        if not info["count"]:
            continue
        seen += 1
        for a1, a2 in ((u1, u2), (l1, l2)):
            w1, w2 = max(w1, rel_err(a1, s1)), max(w2, rel_err(a2, s2))
            assert np.all(np.abs(a1 - s1) <= 1e-5 * s1), (k, rel_err(a1, s1))
            assert np.all(np.abs(a2 - s2) <= 2e-5 * s2), (k, rel_err(a2, s2))
    print(f"(x, 0) against SkCascade over {seen} stages: worst relative difference s1 {w1:.3g} s2 {w2:.3g}")
    assert seen >= 3


def same_moments(a, b, tol, what=""):
    """tol 0: equal bits; else all four rows within tol (the pair object's chunking bound), statistics equal"""
    assert len(a) == len(b), what
    for k, (ma, mb) in enumerate(zip(a, b)):
        assert ma[0] == mb[0], (what, k)
        for u, v in zip(ma[1:], mb[1:]):
            if tol == 0:
                assert u.tobytes() == v.tobytes(), (what, k)
            else:
                assert np.all(np.abs(u - v) <= tol * v), (what, k, rel_err(u, v))


CUTS = np.cumsum([0, 1000, 77_777, (1 << 20) + 3])


def test_zoom_sk_chunking_and_routes(pkg, gpu_required):
    """One call against calls of 1000, 77 777 and 2^20 + 3 samples, host and device: all four rows within the pair object's chunking
    bound (2e-6).  The same calls twice, host against device, reset and replay (after changing detrend and avg): equal bits."""
    import torch
    n = 512
    length = int(CUTS[-1])
    x = gaussian(length, 31)
    ftw, ph0 = pkg.zoom_ftw(0.2718281828459045)[0], 0x0123456789ABCDEF
    make = lambda: pkg.ZoomSkCascade(n, ftw=ftw, phase0=ph0)  # noqa: E731
    one = make()
    one.process(x)
    ref = moments(one)
    a = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a.process(x[s:e])
    got_a = moments(a)
    same_moments(got_a, ref, 2e-6, "host chunks")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    d = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    got_d = moments(d)
    same_moments(got_d, ref, 2e-6, "device chunks")
    same_moments(got_d, got_a, 0, "host against device, same calls")
    one_d = make()
    one_d.process_device(dx.data_ptr(), length)
    same_moments(moments(one_d), ref, 0, "host against device, one call")
    a2 = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a2.process(x[s:e])
    same_moments(moments(a2), got_a, 0, "same calls twice")
    psd_d, sk_d = d.psd(), d.sk()
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()  # settings too; the single object's carrier is kept
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    same_moments(moments(d), got_d, 0, "reset + replay")
    p2, s2 = d.psd(), d.sk()
    assert p2[2] == psd_d[2] and all(u.tobytes() == v.tobytes() for u, v in zip(p2[:2] + s2[:2], psd_d[:2] + sk_d[:2]))
    assert d.stats()["samples_in"] == length


def test_iq_sk_chunking_and_routes(pkg, gpu_required):
    """The same for the complex feed, and its routes: interleaved against planar and host against device give equal bits"""
    import torch
    n = 512
    length = int(CUTS[-1])
    i, q = gaussian(length, 32), gaussian(length, 33)
    z = (i + 1j * q).astype(np.complex64)
    make = lambda: pkg.IqSkCascade(n, f0=0.2718281828459045, phase0=0x0123456789ABCDEF)  # noqa: E731
    one = make()
    one.process(z)
    ref = moments(one)
    a = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a.process(z[s:e])
    got_a = moments(a)
    same_moments(got_a, ref, 2e-6, "host chunks")
    p = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        p.process((i[s:e], q[s:e]))
    same_moments(moments(p), got_a, 0, "interleaved against planar, host")
    dz, di, dq = torch.from_numpy(z).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    d = make()
    dp = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz.data_ptr() + 8 * int(s), int(e - s))
        dp.process_device_planar(di.data_ptr() + 4 * int(s), dq.data_ptr() + 4 * int(s), int(e - s))
    got_d = moments(d)
    same_moments(got_d, got_a, 0, "host against device, same calls")
    same_moments(moments(dp), got_d, 0, "interleaved against planar, device")
    one_d = make()
    one_d.process_device(dz.data_ptr(), length)
    same_moments(moments(one_d), ref, 0, "host against device, one call")
    a2 = make()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        a2.process(z[s:e])
    same_moments(moments(a2), got_a, 0, "same calls twice")
    d.set_detrend(3)
    d.set_avg(pkg.AvgOpts(5, 100))
    d.reset()
    for s, e in zip(CUTS[:-1], CUTS[1:]):
        d.process_device(dz.data_ptr() + 8 * int(s), int(e - s))
    same_moments(moments(d), got_d, 0, "reset + replay")
    assert d.stats()["samples_in"] == length


@pytest.mark.parametrize("family", ["zoom", "iq"])
def test_zoom_sk_bank(pkg, gpu_required, family):
    """Two channels of a bank with different carriers and streams, fed in turn, equal two single objects bit for bit (each channel
    fed and read out in turn, so that its rounds are its single object's); channel 0 is unchanged after channel 1 is fed"""
    n = 256
    lens, step = [300_000, 123_457], [65_536, 33_333]
    car = [pkg.zoom_ftw(f)[0] for f in (0.2, 0.75)]
    ph = [12345, 1 << 63]
    if family == "zoom":
        xs = [gaussian(m, 400 + c) for c, m in enumerate(lens)]
        bank, single = pkg.ZoomSkCascadeBank(n, 2), pkg.ZoomSkCascade
    else:
        xs = [(gaussian(m, 400 + c) + 1j * gaussian(m, 500 + c)).astype(np.complex64) for c, m in enumerate(lens)]
        bank, single = pkg.IqSkCascadeBank(n, 2), pkg.IqSkCascade
    for c in range(2):
        bank.set_carrier(c, ftw=car[c], phase0=ph[c])
    singles = []
    for c, x in enumerate(xs):
        s = single(n, ftw=car[c], phase0=ph[c])
        for p in range(0, x.size, step[c]):
            bank.process(c, x[p:p + step[c]])
            s.process(x[p:p + step[c]])
        got = [bank.stage_moments(c, k) for k in range(bank.num_stages(c))]
        same_moments(got, moments(s), 0, f"channel {c}")
        for a, b in zip(bank.psd(c) + bank.sk(c), s.psd() + s.sk()):
            assert a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
        singles.append(moments(s))
    same_moments([bank.stage_moments(0, k) for k in range(bank.num_stages(0))], singles[0], 0, "channel 0 afterwards")


def gpu_stages(pkg, case):
    v = prop_input(case)
    g = pkg.ZoomSkCascade(PROP_N, f0=PROP_F0) if case == "real" else pkg.IqSkCascade(PROP_N)
    g.process(v if case == "real" else (v[0], v[1]))
    return moments(g)


def gpu_sk_rows(pkg, m):
    return pkg.sk_from_moments(m[0]["count"], m[1], m[3]), pkg.sk_from_moments(m[0]["count"], m[2], m[4])


def test_zoom_sk_circular_noise_reads_one_at_every_bin(pkg, ora, gpu_required):
    """(a) of tests/test_zoom_sk_host.py on the GPU: the same input, the same assertions; counts equal the restatement's"""
    st = gpu_stages(pkg, "circular")
    ref = prop_restatement(pkg, ora, "circular")
    assert [m[0]["count"] for m in st] == [s["count"] for s in ref]
    check_circular(lambda k: gpu_sk_rows(pkg, st[k]), [m[0]["count"] for m in st])


def test_zoom_sk_real_stream_rises_at_its_dc_and_nyquist(pkg, gpu_required):
    """(b): ZoomSkCascade(f0 = 0.2) on real Gaussian noise, stage 0"""
    m = gpu_stages(pkg, "real")[0]
    check_real(*gpu_sk_rows(pkg, m), m[0]["count"])


def test_zoom_sk_complex_tone_reads_zero_on_its_side(pkg, ora, gpu_required):
    """(c): the tone's bin reads 0 in `upper` only: the row orientation"""
    m = gpu_stages(pkg, "tone")[0]
    assert m[0]["count"] == prop_restatement(pkg, ora, "tone")[0]["count"]
    check_tone(*gpu_sk_rows(pkg, m))


def test_zoom_sk_launches(pkg, gpu_required):
    """After warm-up to ten live stages (as test_sk_launches warms) 8 steady device calls record what ZoomCascade records for the same
    calls: 1 + 3 launches a call (mixer; segments, decimators, fold + tails)"""
    import torch
    n = 512
    m = 1 << 24
    dx = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    la = {}
    for name, g in (("zsk", pkg.ZoomSkCascade(n, f0=0.2)), ("zoom", pkg.ZoomCascade(n, f0=0.2))):
        for _ in range(760):  # 1.3e10 samples: stage 9 takes its first ones after 1.0e10
            g.process_device(dx.data_ptr(), m)
        g.stats_read(reset=True)
        for _ in range(8):
            g.process_device(dx.data_ptr(), m)
        la[name] = g.stats_read()["launches"]
        g.sync()
        assert g.num_stages() >= 10
        g.close()
    assert la["zsk"] == la["zoom"] == 4 * 8, la


@pytest.mark.parametrize("family", ["zsk", "iqsk"])
def test_zoom_sk_argument_errors_on_an_object(pkg, gpu_required, family):
    """Detrend::Linear, channel and stage out of range, null sample pointers, set_carrier after the first sample"""
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    b = (pkg.ZoomSkCascadeBank if family == "zsk" else pkg.IqSkCascadeBank)(256, 2)
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED and pre + "set_detrend" in str(e.value)  # as the zoom object refuses it
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(9)
    assert e.value.code == pkg.ERR_ARG
    x = np.zeros(1000, np.complex64 if family == "iqsk" else np.float32)
    for call in (lambda: b.process(2, x), lambda: b.process_device(7, 4096, 10), lambda: b.num_stages(2), lambda: b.psd(2),
                 lambda: b.sk(5), lambda: b.stage_moments(2, 0), lambda: b.set_carrier(2, f0=0.1)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "out of range (n_channels 2)" in str(e.value) and pre[:-1] in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, f0=0.1, ftw=5)
    assert e.value.code == pkg.ERR_ARG
    if family == "zsk":
        nulls = {"process": L.psdc_zsk_process(b._h, 0, None, 4), "process_device": L.psdc_zsk_process_device(b._h, 0, None, 4, None)}
        assert L.psdc_zsk_process(b._h, 0, None, 0) == 0  # nothing to read
    else:
        one = np.zeros(4, np.float32)
        nulls = {"process": L.psdc_iqsk_process(b._h, 0, pkg._fptr(one), None, 4),
                 "process_device": L.psdc_iqsk_process_device(b._h, 0, None, None, 4, None),
                 "process_interleaved": L.psdc_iqsk_process_interleaved(b._h, 0, None, 4),
                 "process_interleaved_device": L.psdc_iqsk_process_interleaved_device(b._h, 0, None, 4, None)}
    for name, rc in nulls.items():
        assert rc == pkg.ERR_ARG, name
    assert "null" in getattr(L, pre + "last_error")(b._h).decode()
    with pytest.raises(pkg.PsdError) as e:
        b.stage_moments(0, 0)  # no sample yet: no stage
    assert e.value.code == pkg.ERR_ARG and pre + "stage_moments: stage 0 out of range" in str(e.value)
    up, lo, br = b.psd(0)
    su, sl, br2 = b.sk(0)
    assert up.size == lo.size == su.size == sl.size == 0 and br == br2 == []
    b.process(0, x)
    with pytest.raises(pkg.PsdError) as e:
        b.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    b.set_carrier(1, ftw=1)  # channel 1 has taken nothing yet
    info = b.stage_moments(0, 0)[0]
    assert info["count"] == 6 and b.stats_read()["samples_in"] == 1000  # 1 + (1000 - 256) // 128 segments
    ns = b.num_stages(0)  # (stage 1 exists already: 1000 samples put 90 decimated ones behind the drain)
    with pytest.raises(pkg.PsdError) as e:
        b.stage_moments(0, ns)
    assert e.value.code == pkg.ERR_ARG and f"stage {ns} out of range ({ns} stages)" in str(e.value)
    b.close()


def test_zoom_sk_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --zoom-sk 0.2001 on noise plus a line 1e-3 fs above the carrier: the lines offset,psd,sk against
    the object's read-out laid out by two_sided (one call here: the file is shorter than the tool's 2^20 samples a call), the
    line's bin the smallest SK, and the count line.  (A real line has two images around a carrier: +df, read from the deepest
    stage, and -(2 f0 + df), read from stage 0; both read 0, and which of the two rounding leaves smaller is not the tool's doing.)"""
    fs = 1000.0
    length = (1 << 17) + 777
    f0, df = 0.2001, 1e-3
    x = (gaussian(length, 41) + 30.0 * np.cos(2 * np.pi * (f0 + df) * np.arange(length))).astype(np.float32)
    raw = tmp_path / "x.f32"
    x.astype("<f4").tofile(raw)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--raw", str(raw), "--zoom-sk", str(f0), "--fs", str(fs),
                        "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("zoom sk raw @ 0.2001")]
    assert len(line) == 1 and "bins beyond 8 sigma of 1: " in line[0], r.stdout
    assert int(line[0].rsplit(": ", 1)[1]) >= 1
    bank = pkg.ZoomSkCascadeBank(512, 1)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.set_carrier(0, f0=f0)
    bank.process(0, x)
    up, lo, br = bank.psd(0, pkg.MergeOpts(min_count=1))
    sup, slo, _ = bank.sk(0, pkg.MergeOpts(min_count=1))
    off, psd = pkg.two_sided(up, lo, br)
    _, sk = pkg.two_sided(sup, slo, br)
    d = np.loadtxt(tmp_path / "csv" / "zoomsk_raw_0_2001.csv", delimiter=",")
    assert d.shape == (psd.size, 3)
    assert np.allclose(d[:, 0], off * fs, rtol=1e-6, atol=0) and np.all(np.diff(d[:, 0]) > 0)
    assert np.all(np.abs(d[:, 1] - psd) <= 2e-6 * psd + 1e-6 * np.mean(psd))
    assert np.array_equal(np.isnan(d[:, 2]), np.isnan(sk)) and np.allclose(d[:, 2], sk, rtol=1e-5, atol=1e-6, equal_nan=True)
    skv = np.where(np.isnan(d[:, 2]), np.inf, d[:, 2])
    k = int(np.argmin(skv))
    near = np.abs(d[:, 0] - df * fs) <= fs / 512  # the line's bins above the carrier
    kl = int(np.flatnonzero(near)[np.argmin(skv[near])])
    print(f"line at offset {d[kl, 0]:.4g} reads SK {d[kl, 2]:.3g}; the smallest SK of the read-out is {d[k, 2]:.3g} at offset {d[k, 0]:.4g}")
    assert d[kl, 2] < 0.05  # the line reads 0 where everything else reads about 1
    assert k == kl or abs(d[k, 0] + (2 * f0 + df) * fs) <= fs / 512, (d[k, 0], d[k, 2])  # the smallest SK is the line's (or its image's)
