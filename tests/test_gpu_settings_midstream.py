"""Mid-stream set_detrend / set_avg on every object kind of csrc/cross_runtime.cpp, on the GPU.  The header's promise (include/
psdcascade.h, cross section; src/psd.rs:431-443) is that samples fed before a change are analysed with the old setting.  The
runtime keeps it by draining the rounds a process call left queued in front of the assignment (set_detrend_impl, set_avg_impl).

One walk a case: a bank of two units fed unevenly by host and device calls (odd pointer offsets; the complex kinds alternate
planar and interleaved), with set_detrend / set_avg and read-outs in between (settings_schedule.make_walk; its conditions are
checked in tests/test_settings_schedule_host.py).  At every read-out and at the end the unit is held to the f64 restatement of its
family run under the unit's own Schedule, with the f32 sibling under the same Schedule as the yardstick of the widened bounds:
stages, counts, averages, pendings and Breaks exactly; every real row of every live stage by assert_psd_close (a stage >= 1 that
ran under Midpoint or Span with conftest.anchored_terms at bins 0 and 1); cross and complementary rows, S2 rows and the stitched
read-outs by the helpers and bounds of the family's own parity test.  The cross rows of a decimated stage are held through the
stitched read-out, as those tests hold them: its Breaks leave out the transition band, where a bin holds 1e-4 of the stage's power
and no bound relative to the bin can hold in f32.  The integer and stream-frame routes are bit for bit the f32 sample route in
their own suites and stay out."""
import numpy as np
import pytest

import test_gpu_waterfall
import test_gpu_zoom_ampm
import test_gpu_zoom_ampm_cross
import test_gpu_zoom_sk
from conftest import anchored_terms, assert_psd_close, stage_stream_scale
from settings_schedule import KINDS, UNITS, WALKS, WF_BLOCK, WF_DEPTH, Schedule, make_walk, segments_after, unit_events
from test_cross_host import restate, stitch_rows
from test_gpu_cross import DETRENDS, assert_sxy_close, noise
from test_gpu_csm import channels
from test_gpu_iq import iq_noise
from test_gpu_iq_cross import pair_iq
from test_gpu_sk import sk_by_breaks, stitched
from test_gpu_zoom_cross import assert_cross_rows
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_sk_host import gaussian, restate_sk
from test_waterfall_host import WF_ROWS, ZWF_ROWS, restate_waterfall, restate_zoom_waterfall
from test_zoom_ampm_cross_host import restate_zoom_ampm_cross
from test_zoom_ampm_host import restate_zoom_ampm
from test_zoom_cross_host import pair_input, restate_zoom_cross, stitch_zoom_cross
from test_zoom_host import emul, mix_f32, mix_f64, parity_input, restate_zoom, stitch_zoom, windows_of  # noqa: F401
from test_zoom_sk_host import restate_zoom_sk

pytestmark = pytest.mark.gpu

F0 = (0.2345678901234567, 0.3141592653589793)  # carriers off the bin grid, as the parity cases of the zoom and IQ families have them
CSM_M = 3  # the channels of a matrix unit in the walks of this file; a Case may say otherwise (tests/test_gpu_segment_instances.py)


class Unit:
    """one unit of a bank behind the surface of the family's single object, which the parity helpers of the family's own test
    take: unit.psd() is bank.psd(unit), unit.stage_rows(k) is bank.stage_rows(unit, k)"""

    def __init__(self, bank, unit):
        self._bank, self._unit = bank, unit

    def __getattr__(self, name):
        fn = getattr(self._bank, name)
        return lambda *a, **kw: fn(self._unit, *a, **kw)


class Case:
    """what the steps of one walk share: the window in its three spellings, the carriers, the units' streams behind the mixer"""

    def __init__(self, pkg, ora, kind, n, wkind, emuls, m=CSM_M):
        self.pkg, self.ora, self.kind, self.n, self.wkind, self.emuls = pkg, ora, kind, n, wkind, emuls
        self.m = m  # the channels of a matrix unit (csm alone reads it)
        self.pwin, self.owin = windows_of(pkg, n, wkind)
        self.wt = self.pwin if isinstance(self.pwin, pkg.WindowTable) else pkg.WindowTable._kind(n, self.pwin)  # (a caller's table)
        self.overlap = self.wt.overlap
        self.ftw = tuple(pkg.zoom_ftw(f)[0] for f in F0)
        self.mixed = {}

    def mix(self, unit, side, planes, prec):
        """(I, Q) of one side of a unit behind the mixer, whole stream, computed once: f64 from the exact phases, f32 from the
        kernel's own oscillator run on the host"""
        key = (unit, side, prec)
        if key not in self.mixed:
            ftw = self.ftw[side]
            if KINDS[self.kind][1]:
                i, q = planes[2 * side], planes[2 * side + 1]
                self.mixed[key] = mix_c_f64(i, q, ftw) if prec == "f64" else mix_c_f32(self.emuls[1], i, q, ftw)
            else:
                self.mixed[key] = mix_f64(planes[side], ftw) if prec == "f64" else mix_f32(self.emuls[0], planes[side], ftw)
        return self.mixed[key]


def extra_of(c, sched, k, nseg, count, scale, row):
    """the anchored-detrend allowance of bins 0 and 1 of a stage's row (conftest.anchored_terms, as check_against_oracle of
    tests/test_gpu_parity.py applies it): for a stage >= 1 that ran segments under Midpoint or Span.  scale: max |sample| of the
    stage's stream (of I and Q for the two-sided rows of a mixed stream)."""
    if k == 0 or not count or not sched.detrends_of_stage(k, nseg) & {"midpoint", "span"}:
        return None
    t = anchored_terms(c.n, count, scale, row[0], row[1], "hann" if c.wkind == "hann" else "rect")
    return {0: t[0], 1: t[1]}


def merged_extra(c, br, extras):
    """extras {stage: extra_of()} carried to the stitched row: a stage's bins 0 and 1 are in it only where its range starts at 0,
    scaled by 1 / (gain decimation); Break i is stage ns - 1 - i"""
    out = {}
    for i, b in enumerate(br):
        e = extras.get(len(br) - 1 - i)
        if e and b.include and b.bins.start == 0:
            sc = 1.0 / ((c.n // 2) * b.count * float(c.wt.nenbw) * float(c.wt.power) * b.decimation)
            out[b.start], out[b.start + 1] = e[0] * sc, e[1] * sc
    return out or None


def scale_of(c, streams, k):
    return max(stage_stream_scale(c.ora, s, k) for s in streams)


def exact(infos, st, what):
    assert len(infos) == len(st), (what, len(infos), len(st))
    for k, (info, s) in enumerate(zip(infos, st)):
        assert (info["count"], info["avg"], info["pending"]) == (s["count"], s["avg"], s["pending"]), (what, k, info)


# ---- the families: input, feed, restatement, comparison ----

class Family:
    cls = None
    sides = 1          # streams a unit takes (complex kinds: complex streams)
    list_feed = False  # the matrix object takes its channels as one list

    def sides_of(self, c):
        return self.sides

    def make(self, c):
        return getattr(c.pkg, self.cls)(c.n, UNITS, window=c.pwin)

    def carriers(self, c, bank):
        pass

    def host(self, c, bank, u, parts, layout):
        if not KINDS[c.kind][1]:
            return bank.process(u, parts) if self.list_feed else bank.process(u, *parts)
        if layout == "planar":
            z = [(parts[2 * s], parts[2 * s + 1]) for s in range(self.sides)]
        else:
            z = [(parts[2 * s] + 1j * parts[2 * s + 1]).astype(np.complex64) for s in range(self.sides)]
        bank.process(u, *z)

    def device(self, c, bank, u, ptrs, length, layout):
        if not KINDS[c.kind][1]:
            return bank.process_device(u, ptrs, length) if self.list_feed else bank.process_device(u, *ptrs, length)
        (bank.process_device_planar if layout == "planar" else bank.process_device)(u, *ptrs, length)


class Cross(Family):
    cls = "CsdCascadeBank"
    sides = 2

    def input(self, c, length, seed):
        x = noise(length, seed)
        return [x, (0.6 * x + 0.8 * noise(length, seed + 7)).astype(np.float32)]

    def restate(self, c, u, planes, prec, sched):
        return restate(c.ora, planes[0], planes[1], c.n, c.owin, prec=prec, schedule=sched)

    def pair(self, c, sched, segs, planes, st64, st32, stage, csd, what):
        """one pair of real streams: stage(k) -> (sxx, syy, sxy), csd -> (sxx, syy, sxy, breaks)"""
        extras = [{}, {}]
        for k, (s, s32) in enumerate(zip(st64, st32)):
            if not s["count"]:
                continue
            got = stage(k)
            for side, key in enumerate(("sxx", "syy")):
                e = extra_of(c, sched, k, segs[k], s["count"], scale_of(c, [planes[side]], k) if k else 0.0, s[key])
                extras[side][k] = e
                assert_psd_close(got[side], s[key], f"{what} {key} stage {k}", ref_f32=s32[key], extra_tol=e)
            if k == 0:
                assert_sxy_close(got[2], s["sxy"], s["sxx"], s["syy"], 1e-5, f"{what} stage 0", atol_frac=1e-6)
        rx, ry, rxy, rbr = stitch_rows(c.pkg, c.n, c.wt, st64, c.pkg.MergeOpts())
        sx, sy, _, _ = stitch_rows(c.pkg, c.n, c.wt, st32, c.pkg.MergeOpts())
        sxx, syy, sxy, br = csd
        assert br == rbr, what
        assert_psd_close(sxx, rx, f"{what} Sxx", ref_f32=sx, extra_tol=merged_extra(c, br, extras[0]))
        assert_psd_close(syy, ry, f"{what} Syy", ref_f32=sy, extra_tol=merged_extra(c, br, extras[1]))
        assert_sxy_close(sxy, rxy, rx, ry, 1e-5, f"{what} Sxy", atol_frac=1e-6)

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what):
        got = [bank.stage_spectra(u, k) for k in range(bank.num_stages(u))]
        exact([g[0] for g in got], st64, what)
        self.pair(c, sched, segs, planes, st64, st32, lambda k: got[k][1:], bank.csd(u), what)


class Csm(Cross):
    cls = "CsmCascadeBank"
    sides = None  # the case's channel count
    list_feed = True

    def sides_of(self, c):
        return c.m

    def pairs(self, c):
        return [(a, b) for a in range(c.m) for b in range(a + 1, c.m)]

    def make(self, c):
        return c.pkg.CsmCascadeBank(c.n, c.m, UNITS, window=c.pwin)

    def input(self, c, length, seed):
        return channels(c.m, length, seed)

    def restate(self, c, u, planes, prec, sched):
        return {p: restate(c.ora, planes[p[0]], planes[p[1]], c.n, c.owin, prec=prec, schedule=sched) for p in self.pairs(c)}

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what):
        got = [bank.stage_spectra(u, k) for k in range(bank.num_stages(u))]
        S, br = bank.csd(u)
        for a, b in self.pairs(c):
            exact([g[0] for g in got], st64[a, b], what)
            self.pair(c, sched, segs, [planes[a], planes[b]], st64[a, b], st32[a, b],
                      lambda k: (got[k][1][a, a].real, got[k][1][b, b].real, got[k][1][a, b]),
                      (S[a, a].real, S[b, b].real, S[a, b], br), f"{what} S[{a},{b}]")


class Zoom(Family):
    cls = "ZoomCascadeBank"

    def carriers(self, c, bank):
        for u in range(UNITS):
            bank.set_carrier(u, ftw=c.ftw[0])

    def input(self, c, length, seed):
        return [parity_input(c.n + seed, length)]

    restate_fn = staticmethod(restate_zoom)

    def restate(self, c, u, planes, prec, sched, taken=None, **kw):
        i, q = c.mix(u, 0, planes, prec)
        return self.restate_fn(c.ora, None, c.n, c.ftw[0], 0, c.owin, prec=prec, iq=(i[:taken], q[:taken]), schedule=sched, **kw)

    def real_rows(self, c, u, sched, segs, planes, taken, st64, st32, rows, names, what):
        """the two-sided real rows of every live stage: rows(k) -> the arrays named `names` of the restated stage"""
        extras = {name: {} for name in names}
        iq = c.mix(u, 0, planes, "f64")
        for k, (s, s32) in enumerate(zip(st64, st32)):
            if not s["count"]:
                continue
            scale = scale_of(c, [v[:taken] for v in iq], k) if k else 0.0
            for name, got in zip(names, rows(k)):
                e = extra_of(c, sched, k, segs[k], s["count"], scale, s[name])
                extras[name][k] = e
                assert_psd_close(got, s[name], f"{what} {name} stage {k}", ref_f32=s32[name], extra_tol=e)
        return extras

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        got = [bank.stage_spectra(u, k) for k in range(bank.num_stages(u))]
        exact([g[0] for g in got], st64, what)
        ex = self.real_rows(c, u, sched, segs, planes, taken, st64, st32, lambda k: got[k][1:], ("upper", "lower"), what)
        up, lo, br = bank.psd(u)
        rup, rlo, rbr = stitch_zoom(c.pkg, c.n, c.pwin, st64)
        sup, slo, _ = stitch_zoom(c.pkg, c.n, c.pwin, st32)
        assert br == rbr, what
        assert_psd_close(up, rup, f"{what} upper", ref_f32=sup, extra_tol=merged_extra(c, br, ex["upper"]))
        assert_psd_close(lo, rlo, f"{what} lower", ref_f32=slo, extra_tol=merged_extra(c, br, ex["lower"]))


class Iq(Zoom):
    cls = "IqCascadeBank"

    def input(self, c, length, seed):
        return list(iq_noise(length, seed))


class ZoomCsd(Family):
    cls = "ZoomCsdCascadeBank"
    sides = 2

    def carriers(self, c, bank):
        for u in range(UNITS):
            for side in (0, 1):
                bank.set_carrier(u, ftw=c.ftw[side], side=side)

    def input(self, c, length, seed):
        return list(pair_input(length, seed))

    restate_fn = staticmethod(restate_zoom_cross)

    def restate(self, c, u, planes, prec, sched, taken=None, **kw):
        iq = tuple(tuple(v[:taken] for v in c.mix(u, side, planes, prec)) for side in (0, 1))
        return self.restate_fn(c.ora, None, None, c.n, c.ftw, (0, 0), c.owin, prec=prec, iq=iq, schedule=sched, **kw)

    def auto_rows(self, c, u, sched, segs, planes, taken, st64, st32, rows, what):
        """rows 0 ... 3 of every live stage: rows(k) -> the stage's (8 or 12, n/2 + 1) array"""
        extras = [{} for _ in range(4)]
        for k, (s, s32) in enumerate(zip(st64, st32)):
            if not s["count"]:
                continue
            got = rows(k)
            for r in range(4):
                iq = c.mix(u, r // 2, planes, "f64")
                e = extra_of(c, sched, k, segs[k], s["count"], scale_of(c, [v[:taken] for v in iq], k) if k else 0.0, s["rows"][r])
                extras[r][k] = e
                assert_psd_close(got[r], s["rows"][r], f"{what} row {r} stage {k}", ref_f32=s32["rows"][r], extra_tol=e)
        return extras

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        got = [bank.stage_spectra(u, k) for k in range(bank.num_stages(u))]
        exact([g[0] for g in got], st64, what)
        ex = self.auto_rows(c, u, sched, segs, planes, taken, st64, st32, lambda k: got[k][1], what)
        if st64[0]["count"]:  # the cross rows of stage 0, raw: within 1e-5 sqrt(S_aa S_bb) of their side
            r, g = st64[0]["rows"], got[0][1]
            for lo in (0, 1):
                assert_sxy_close(g[4 + lo] + 1j * g[6 + lo], r[4 + lo] + 1j * r[6 + lo], r[lo], r[2 + lo], 1e-5,
                                 f"{what} S_ab {'lower' if lo else 'upper'} stage 0", atol_frac=1e-6)
        res = bank.csd(u)
        ref = stitch_zoom_cross(c.pkg, c.n, c.pwin, st64)
        sib = stitch_zoom_cross(c.pkg, c.n, c.pwin, st32)
        assert res[6] == ref[6], what
        for r in range(4):
            assert_psd_close(res[r], ref[r], f"{what} merged row {r}", ref_f32=sib[r], extra_tol=merged_extra(c, res[6], ex[r]))
        assert_cross_rows(res, ref, 1e-5, what, atol_frac=1e-6)


class IqCsd(ZoomCsd):
    cls = "IqCsdCascadeBank"

    def input(self, c, length, seed):
        a, b = pair_iq(length, seed)
        return [a[0], a[1], b[0], b[1]]


class Sk(Family):
    cls = "SkCascadeBank"

    def input(self, c, length, seed):
        return [gaussian(length, seed)]

    def restate(self, c, u, planes, prec, sched):
        return restate_sk(c.ora, planes[0], c.n, c.owin, prec=prec, schedule=sched)

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what):
        pkg = c.pkg
        got = [bank.stage_moments(u, k) for k in range(bank.num_stages(u))]
        exact([g[0] for g in got], st64, what)
        extras = {}
        for k, ((info, s1, s2), s, s32) in enumerate(zip(got, st64, st32)):
            if not s["count"]:
                continue
            extras[k] = extra_of(c, sched, k, segs[k], s["count"], scale_of(c, planes, k) if k else 0.0, s["s1"])
            assert_psd_close(s1, s["s1"], f"{what} S1 stage {k}", ref_f32=s32["s1"], extra_tol=extras[k])
            # rows 1 as test_sk_parity holds them: rtol 2e-5 (squaring doubles the relative error), held to the f32 restatement
            assert_psd_close(s2, s["s2"], f"{what} S2 stage {k}", rtol=2e-5, ref_f32=s32["s2"])
        for k, ((info, s1, s2), s) in enumerate(zip(got, st64)):  # SK wherever both rows met their pure bounds, as test_sk_parity
            m = s["count"]
            if m < 2:
                assert np.all(np.isnan(pkg.sk_from_moments(m, s1, s2)))
                continue
            ok = (np.abs(s1 - s["s1"]) <= 1e-5 * s["s1"]) & (np.abs(s2 - s["s2"]) <= 2e-5 * s["s2"]) & (s["s1"] > 0)
            sk_g, sk_r = pkg.sk_from_moments(m, s1, s2)[ok], pkg.sk_from_moments(m, s["s1"], s["s2"])[ok]
            assert np.all(np.abs(sk_g - sk_r) <= 4e-5 * (sk_r + (m + 1.0) / (m - 1.0))), (what, k)
        psd, br = bank.psd(u)
        ref0, rbr = stitched(pkg, c.n, c.pwin, st64, "s1")
        assert br == rbr, what
        assert_psd_close(psd, ref0, f"{what} psd", ref_f32=stitched(pkg, c.n, c.pwin, st32, "s1")[0], extra_tol=merged_extra(c, br, extras))
        sk, sbr = bank.sk(u)
        assert sbr == br and np.array_equal(sk, sk_by_breaks(pkg, Unit(bank, u), br), equal_nan=True), what


class ZoomSk(Zoom):
    cls = "ZoomSkCascadeBank"
    restate_fn = staticmethod(restate_zoom_sk)

    def input(self, c, length, seed):
        return [gaussian(length, seed)]

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        got = [bank.stage_moments(u, k) for k in range(bank.num_stages(u))]
        self.real_rows(c, u, sched, segs, planes, taken, st64, st32, lambda k: got[k][1:3], ("upper", "lower"), what)
        test_gpu_zoom_sk.assert_parity(c.pkg, Unit(bank, u), st64, st32, c.n, c.pwin, "scheduled", what)


class IqSk(ZoomSk):
    cls = "IqSkCascadeBank"

    def input(self, c, length, seed):
        return [gaussian(length, seed), gaussian(length, seed + 1000)]


class ZoomAmPm(Zoom):
    cls = "ZoomAmPmCascadeBank"
    restate_fn = staticmethod(restate_zoom_ampm)

    def input(self, c, length, seed):
        return [gaussian(length, seed)]

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        got = [bank.stage_rows(u, k) for k in range(bank.num_stages(u))]
        self.real_rows(c, u, sched, segs, planes, taken, st64, st32, lambda k: got[k][1:3], ("upper", "lower"), what)
        test_gpu_zoom_ampm.assert_parity(c.pkg, Unit(bank, u), st64, st32, c.n, c.pwin, "scheduled", what)


class IqAmPm(ZoomAmPm):
    cls = "IqAmPmCascadeBank"

    def input(self, c, length, seed):
        return [gaussian(length, seed), gaussian(length, seed + 1000)]


class ZoomAmPmCsd(ZoomCsd):
    cls = "ZoomAmPmCsdCascadeBank"
    restate_fn = staticmethod(restate_zoom_ampm_cross)

    def input(self, c, length, seed):  # the pair of test_zoom_ampm_cross_parity: coherence neither 0 nor 1
        a = gaussian(length + 3, seed)
        return [a[3:].copy(), (0.6 * a[:-3] + 0.8 * gaussian(length, seed + 1000)).astype(np.float32)]

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        got = [bank.stage_rows(u, k) for k in range(bank.num_stages(u))]
        self.auto_rows(c, u, sched, segs, planes, taken, st64, st32, lambda k: got[k][1], what)
        test_gpu_zoom_ampm_cross.assert_parity(c.pkg, Unit(bank, u), st64, st32, c.n, c.pwin, "scheduled", what)


class IqAmPmCsd(ZoomAmPmCsd):
    cls = "IqAmPmCsdCascadeBank"

    def input(self, c, length, seed):  # the pair of test_iq_ampm_cross_parity
        ia, qa = gaussian(length, seed), gaussian(length, seed + 100)
        return [ia, qa, (0.6 * ia + 0.8 * gaussian(length, seed + 200)).astype(np.float32),
                (0.6 * qa + 0.8 * gaussian(length, seed + 300)).astype(np.float32)]


class Waterfall(Family):
    cls = "WaterfallCascadeBank"

    def make(self, c):
        return c.pkg.WaterfallCascadeBank(c.n, UNITS, block=WF_BLOCK, depth=WF_DEPTH, window=c.pwin)

    def input(self, c, length, seed):
        return [gaussian(length, seed)]

    def restate(self, c, u, planes, prec, sched):
        return restate_waterfall(c.ora, planes[0], c.n, WF_BLOCK, c.owin, prec=prec, schedule=sched)

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what):
        test_gpu_waterfall.assert_parity(Unit(bank, u), st64, st32, WF_BLOCK, WF_DEPTH, WF_ROWS, what)


class ZoomWaterfall(Zoom):
    cls = "ZoomWaterfallCascadeBank"

    def make(self, c):
        return c.pkg.ZoomWaterfallCascadeBank(c.n, UNITS, block=WF_BLOCK, depth=WF_DEPTH, window=c.pwin)

    def input(self, c, length, seed):
        return [gaussian(length, seed)]

    def restate(self, c, u, planes, prec, sched, taken=None):
        i, q = c.mix(u, 0, planes, prec)
        return restate_zoom_waterfall(c.ora, None, c.n, c.ftw[0], WF_BLOCK, c.owin, prec=prec, iq=(i[:taken], q[:taken]), schedule=sched)

    def check(self, c, bank, u, sched, segs, planes, st64, st32, what, taken=None):
        test_gpu_waterfall.assert_parity(Unit(bank, u), st64, st32, WF_BLOCK, WF_DEPTH, ZWF_ROWS, what)


FAMILIES = {"cross": Cross(), "csm": Csm(), "zoom": Zoom(), "zcsd": ZoomCsd(), "iq": Iq(), "iqcsd": IqCsd(), "sk": Sk(), "zsk": ZoomSk(),
            "iqsk": IqSk(), "zampm": ZoomAmPm(), "iqampm": IqAmPm(), "zxampm": ZoomAmPmCsd(), "iqxampm": IqAmPmCsd(),
            "wf": Waterfall(), "zwf": ZoomWaterfall()}
assert FAMILIES.keys() == KINDS.keys()


def device_buffers(walk, planes, complex_in):
    """per device call of the walk its pointers: every stream of the call copied behind an odd number of elements of an
    allocation of its own (the interleaved layout: one complex64 stream a side, so an odd number of 8-byte elements).  All copies
    are made, and complete, before the first call; the tensors are returned too, to be kept until the walk ends."""
    import torch
    keep, ptrs = [], {}
    pos = [0] * UNITS
    for i, op in enumerate(walk):
        if op[0] not in ("host", "device"):
            continue
        u, length = op[1], op[2]
        if op[0] == "device":
            parts = [p[pos[u]:pos[u] + length] for p in planes[u]]
            if complex_in and op[3] == "interleaved":
                parts = [(parts[2 * s] + 1j * parts[2 * s + 1]).astype(np.complex64) for s in range(len(parts) // 2)]
            ptrs[i] = []
            for p in parts:
                t = torch.empty(length + op[4], dtype=torch.from_numpy(p).dtype, device="cuda")
                t[op[4]:] = torch.from_numpy(p).cuda()
                keep.append(t)
                ptrs[i].append(t.data_ptr() + op[4] * p.itemsize)
        pos[u] += length
    torch.cuda.synchronize()
    return keep, ptrs


@pytest.mark.parametrize("kind,n,seed,wkind", WALKS)
def test_settings_midstream(pkg, ora, gpu_required, emul, iq_emul, kind, n, seed, wkind):  # noqa: F811
    fam = FAMILIES[kind]
    has_avg, complex_in = KINDS[kind]
    c = Case(pkg, ora, kind, n, wkind, (emul, iq_emul))
    walk = make_walk(kind, n, seed, wkind)
    totals = [unit_events(walk, u)[1] for u in range(UNITS)]
    planes = [fam.input(c, totals[u], 10 * seed + u) for u in range(UNITS)]
    assert all(len(p) == fam.sides_of(c) * (2 if complex_in else 1) and all(v.size == totals[u] for v in p) for u, p in enumerate(planes))
    keep, ptrs = device_buffers(walk, planes, complex_in)
    bank = fam.make(c)
    fam.carriers(c, bank)
    pos = [0] * UNITS
    events = [[] for _ in range(UNITS)]
    mixed = isinstance(fam, (Zoom, ZoomCsd))

    def check(u, when):
        taken = pos[u]
        sched = Schedule(n, c.overlap, events[u])
        segs = segments_after(n, c.overlap, taken)
        cut = [p[:taken] for p in planes[u]]
        kw = {"taken": taken} if mixed else {}
        st64 = fam.restate(c, u, planes[u] if mixed else cut, "f64", sched, **kw)
        st32 = fam.restate(c, u, planes[u] if mixed else cut, "f32", sched, **kw)
        assert bank.num_stages(u) == len(segs), (when, u)
        fam.check(c, bank, u, sched, segs, planes[u] if mixed else cut, st64, st32, f"{kind} n={n} unit {u} {when}", **kw)

    reads = 0
    for i, op in enumerate(walk):
        if op[0] == "host":
            u, length = op[1], op[2]
            fam.host(c, bank, u, [p[pos[u]:pos[u] + length] for p in planes[u]], op[3])
            pos[u] += length
        elif op[0] == "device":
            u, length = op[1], op[2]
            fam.device(c, bank, u, ptrs[i], length, op[3])
            pos[u] += length
        elif op[0] == "detrend":
            bank.set_detrend(DETRENDS[op[1]])
            for u in range(UNITS):
                events[u].append((pos[u], op[1], None))
        elif op[0] == "avg":
            bank.set_avg(pkg.AvgOpts(op[1], op[2]))
            for u in range(UNITS):
                events[u].append((pos[u], None, (op[1], op[2])))
        else:
            reads += 1
            check(op[1], f"read-out {reads} (op {i})")
    assert pos == totals
    for u in range(UNITS):
        check(u, "at the end")
    bank.close()
    del keep
