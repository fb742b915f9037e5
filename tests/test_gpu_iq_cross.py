"""IQ cross cascade on the GPU (psdc_iqcsd_*, csrc/iq_cross.hip, csrc/iq_cross_frames.hip) against the f64 restatement of
tests/test_zoom_cross_host.py fed the complex f64 mix of tests/test_iq_host.py, against its complex64 sibling, and against the
objects that exist (ZoomCsdCascade, IqCascade, CsmCascade) where they are comparable.  Semantics: include/psdcascade.h, "IQ cross
cascade".  The tolerances are those of the zoom cross and IQ suites."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS, assert_breaks, assert_sxy_close
from test_gpu_iq import frames_of
from test_gpu_payload_formats import make_frames, random_payloads
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_zoom_cross_host import pair_input, restate_zoom_cross, stitch_zoom_cross
from test_zoom_host import U32_MAX, carrier_ftw, windows_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF

# (n, window, detrend, avg, carriers (a, b), phase0 (a, b), length): the issue's three cases.  64: carriers on bins (two
# oscillators), a length off every grid; 512: a caller's window, a detrend, an EWMA, two carriers with start phases; 2048: one
# carrier on both sides (the shared oscillator), a team of two wavefronts and an odd segment count.
PARITY_CASES = [
    (64, "hann", "none", None, (("bin", 5), ("bin", 11)), (0, 0), (1 << 16) + 37),
    (512, "custom", "span", (U32_MAX, 1000), (0.7131313131313131, 0.3141592653589793), (0x0123456789ABCDEF, 1 << 63), 1 << 17),
    (2048, "hann", "none", None, (0.6180339887498949, 0.6180339887498949), (0, 0), (1 << 18) + 3 * 2048),
]


def pair_iq(length, seed):
    """((I_a, Q_a), (I_b, Q_b)): two complex streams whose coherence is neither 0 nor 1 (pair_input on I and on Q)"""
    ia, ib = pair_input(length, seed)
    qa, qb = pair_input(length, seed + 7919)
    return (ia, qa), (ib, qb)


def make(pkg, n, ftw, window=None, phase0=(0, 0), detrend=None, avg=None):
    g = pkg.IqCsdCascade(n, window=window if window is not None else pkg.Window.HANN)
    for side in (0, 1):
        g.set_carrier(ftw=ftw[side], phase0=phase0[side], side=side)
    if detrend is not None:
        g.set_detrend(detrend)
    if avg is not None:
        g.set_avg(pkg.AvgOpts(*avg))
    return g


def bits(bank, pair=0):
    """csd() and every stage's raw rows and stats of one pair"""
    bank = getattr(bank, "_b", bank)
    return bank.csd(pair), [bank.stage_spectra(pair, k) for k in range(bank.num_stages(pair))]


def assert_bits(a, b, what):
    (ca, sa), (cb, sb) = a, b
    assert ca[6] == cb[6], what
    for u, v in zip(ca[:6], cb[:6]):
        assert u.tobytes() == v.tobytes(), what
    assert len(sa) == len(sb), what
    for k, (u, v) in enumerate(zip(sa, sb)):
        assert u[0] == v[0], (what, k)
        assert u[1].tobytes() == v[1].tobytes(), (what, k)


def assert_cross_rows(got, ref, tol, what, atol_frac=0.0):
    """the two complex rows of a csd() tuple against a reference tuple: tol sqrt(S_aa S_bb) of the reference, side by side"""
    assert_sxy_close(got[4], ref[4], ref[0], ref[2], tol, what + " S_ab upper", atol_frac=atol_frac)
    assert_sxy_close(got[5], ref[5], ref[1], ref[3], tol, what + " S_ab lower", atol_frac=atol_frac)


def truth(ora, a, b, n, ftw, ph, owin="hann", detrend="none", avg=(U32_MAX, U32_MAX)):
    """the f64 restatement of a pair: restate_zoom_cross fed the complex f64 mix of each side"""
    iq = (mix_c_f64(a[0], a[1], ftw[0], ph[0]), mix_c_f64(b[0], b[1], ftw[1], ph[1]))
    return restate_zoom_cross(ora, None, None, n, ftw, ph, owin, detrend, avg, iq=iq)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_iq_cross_parity(pkg, ora, gpu_required, iq_emul, case):  # noqa: F811
    n, wkind, detrend, avg, carriers, ph, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    a, b = pair_iq(length, 3000 + n)
    ftw = tuple(carrier_ftw(pkg, n, c) for c in carriers)
    g = make(pkg, n, ftw, pwin, ph, DETRENDS[detrend], avg)
    g.process(a, b)
    got = g.csd()
    ref = stitch_zoom_cross(pkg, n, pwin, truth(ora, a, b, n, ftw, ph, owin, detrend, avg))
    assert got[6] == ref[6]
    names = ("S_aa upper", "S_aa lower", "S_bb upper", "S_bb lower")
    if detrend == "none":
        for name, u, v in zip(names, got[:4], ref[:4]):
            rel = assert_psd_close(u, v, f"iq cross {name} case {case}", pure=True)
            print(f"case {case} {name}: worst relative error {rel:.3g}")
        err = max(float(np.max(np.abs(got[4 + i] - ref[4 + i]) / np.sqrt(ref[i].astype(np.float64) * ref[2 + i]))) for i in (0, 1))
        print(f"case {case} S_ab: worst error / sqrt(S_aa S_bb) {err:.3g}")
        assert_cross_rows(got, ref, 1e-5, f"case {case}")
    else:  # a detrend nulls bin 0: the widened bound, held to the complex64 sibling's own f32 arithmetic there
        iq = (mix_c_f32(iq_emul, a[0], a[1], ftw[0], ph[0]), mix_c_f32(iq_emul, b[0], b[1], ftw[1], ph[1]))
        sib = stitch_zoom_cross(pkg, n, pwin, restate_zoom_cross(ora, None, None, n, ftw, ph, owin, detrend, avg, "f32", iq=iq))
        for name, u, v, s in zip(names, got[:4], ref[:4], sib[:4]):
            assert_psd_close(u, v, f"iq cross {name} case {case} {detrend}", ref_f32=s)
        for name, u, v in zip(names, got[:4], ref[:4]):
            print(f"case {case} {name}: worst |error| / (value + 1e-6 mean) {float(np.max(np.abs(u - v) / (v + 1e-6 * np.mean(v)))):.3g}")
        scale = [np.sqrt(ref[i].astype(np.float64) * ref[2 + i]) for i in (0, 1)]
        err = max(float(np.max(np.abs(got[4 + i] - ref[4 + i]) / (scale[i] + 0.1 * np.mean(scale[i])))) for i in (0, 1))
        print(f"case {case} S_ab: worst error / (sqrt(S_aa S_bb) + 0.1 of its mean) {err:.3g}")
        assert_cross_rows(got, ref, 1e-5, f"case {case} {detrend}", atol_frac=1e-6)
    # Breaks are those of an IqCascade fed side a, and of the oracle's cascade
    z = pkg.IqCascade(n, ftw=ftw[0], phase0=ph[0], window=pwin)
    z.set_detrend(DETRENDS[detrend])
    z.set_avg(pkg.AvgOpts(*avg))
    z.process(a)
    assert z.psd()[2] == got[6] and z.num_stages() == g.num_stages()
    o = ora.PsdCascade(n, "f64", window=owin)
    o.set_detrend(detrend)
    o.set_avg(*avg)
    o.process(a[0])
    assert_breaks(got[6], o.psd()[1])
    if case == 0:  # the raw rows of a stage, in the header's order: a fresh object fed the stream's head against the restatement
        head = n * 40
        ah, bh = tuple(v[:head] for v in a), tuple(v[:head] for v in b)
        st0 = truth(ora, ah, bh, n, ftw, ph, owin, detrend, avg)[0]
        h = make(pkg, n, ftw, pwin, ph, DETRENDS[detrend], avg)
        h.process(ah, bh)
        info, rows = h.stage_spectra(0)
        assert rows.shape == (8, n // 2 + 1) and info["count"] == st0["count"] and info["pending"] == st0["pending"]
        for r in range(8):
            bound = 1e-5 * (st0["rows"][r] if r < 4 else np.sqrt(st0["rows"][r % 2] * st0["rows"][2 + r % 2]))
            assert np.all(np.abs(rows[r] - st0["rows"][r]) <= bound), r


@pytest.mark.parametrize("n", [64, 1024])
def test_iq_cross_with_q_zero_is_the_zoom_cross_object(pkg, gpu_required, n):
    """With Q_a = Q_b = 0 the object gives the bytes of ZoomCsdCascade fed (a, b) with the same carriers and start phases: the mix
    formula with Q = 0 is zoom_mix, and everything behind the mixer is the same code.  Two receivers' noise streams (no exact
    zeros), one call each, so the rounds coincide."""
    a, b = pair_input(1 << 18, 51 + n)
    assert not np.any(a == 0) and not np.any(b == 0)
    ftw = (pkg.zoom_ftw(0.2)[0], pkg.zoom_ftw(0.2718281828459045)[0])
    ph = (0x0123456789ABCDEF, 1 << 62)
    z = pkg.ZoomCsdCascade(n)
    for side in (0, 1):
        z.set_carrier(ftw=ftw[side], phase0=ph[side], side=side)
    z.process(a, b)
    g = make(pkg, n, ftw, phase0=ph)
    g.process((a, np.zeros_like(a)), (b, np.zeros_like(b)))
    assert_bits(bits(g), bits(z), f"(a, 0), (b, 0) against the zoom cross object, n = {n}")


def test_iq_cross_against_existing_objects(pkg, gpu_required):
    """IQ anchor: the auto rows are two IqCascades' fed the sides (2e-6, the chunking bound of the header: the partial sums are
    ordered differently).  The same stream and carrier on both sides: S_ab = S_aa within 1e-6 and the coherence is 1 within 1e-5.
    The helpers take the rows as they are."""
    n, length = 512, 1 << 18
    a, b = pair_iq(length, 91)
    ftw = (pkg.zoom_ftw(0.2718281828459045)[0], pkg.zoom_ftw(0.6180339887498949)[0])
    ph = (0x0123456789ABCDEF, 1 << 62)
    g = make(pkg, n, ftw, phase0=ph)
    g.process(a, b)
    got = g.csd()
    for side, x in enumerate((a, b)):
        z = pkg.IqCascade(n, ftw=ftw[side], phase0=ph[side])
        z.process(x)
        up, lo, br = z.psd()
        assert br == got[6]
        for name, u, v in (("upper", got[2 * side], up), ("lower", got[2 * side + 1], lo)):
            rel = float(np.max(np.abs(u - v) / v))
            print(f"side {side} {name} against IqCascade: {rel:.3g}")
            assert rel <= 2e-6, (side, name, rel)
    s = make(pkg, n, (ftw[0], ftw[0]), phase0=(ph[0], ph[0]))
    s.process(a, a)
    aup, alo, bup, blo, xup, xlo, _ = s.csd()
    for auto, x in ((aup, xup), (alo, xlo)):
        print(f"same stream: |S_ab - S_aa| / S_aa {float(np.max(np.abs(x - auto) / auto)):.3g}")
        assert np.all(np.abs(x.real - auto) <= 1e-6 * auto) and np.all(np.abs(x.imag) <= 1e-6 * auto)
    assert np.all(np.abs(pkg.coherence(aup, bup, xup) - 1.0) <= 1e-5) and np.all(np.abs(pkg.coherence(alo, blo, xlo) - 1.0) <= 1e-5)
    off, dens = pkg.two_sided(got[0], got[1], got[6])
    assert off.size == dens.size and np.all(np.diff(off) > 0)
    h1 = pkg.transfer(got[0], got[4])
    assert h1.shape == got[4].shape and np.all(np.isfinite(h1))
    coh = pkg.coherence(got[0], got[2], got[4])
    assert coh.shape == got[0].shape and np.all((coh >= 0) & (coh <= 1 + 1e-5))


def test_iq_cross_against_the_matrix_object(pkg, gpu_required):
    """Matrix anchor, carriers 0.  A CsmCascade(512, 4) fed the planar streams x0 = I_a, x1 = Q_a, x2 = I_b, x3 = Q_b keeps
    S[c, d][k] = conj(X_c[k]) X_d[k], X_c the transform of the real stream x_c, k = 0 ... N/2.  The transforms are linear, so
    Z_a = X_0 + i X_1 and Z_b = X_2 + i X_3 at every bin, and
        S_ab[k] = conj(Z_a) Z_b = (conj X_0 - i conj X_1)(X_2 + i X_3) = S[0, 2] + S[1, 3] + i (S[0, 3] - S[1, 2]),
        S_aa[k] = |Z_a|^2 = S[0, 0] + S[1, 1] + i (S[0, 1] - S[1, 0]) = S[0, 0] + S[1, 1] - 2 Im S[0, 1], S_bb likewise from 2, 3.
    These are the `upper` rows (bin k itself).  Every row of both objects goes through the same read-out, which is linear, so
    the identity holds for csd() as for the raw rows.  Bound: assert_sxy_close at 1e-5 sqrt(S_aa S_bb), the matrix side's."""
    n, length = 512, 1 << 18
    a, b = pair_iq(length, 77)
    g = make(pkg, n, (0, 0))
    g.process(a, b)
    got = g.csd()
    m = pkg.CsmCascade(n, 4)
    m.process([a[0], a[1], b[0], b[1]])
    S, br = m.csd()
    assert br == got[6]
    S = S.astype(np.complex128)
    sab = S[0, 2] + S[1, 3] + 1j * (S[0, 3] - S[1, 2])
    saa = (S[0, 0] + S[1, 1]).real - 2.0 * S[0, 1].imag
    sbb = (S[2, 2] + S[3, 3]).real - 2.0 * S[2, 3].imag
    err = float(np.max(np.abs(got[4] - sab) / np.sqrt(saa * sbb)))
    print(f"S_ab upper against CsmCascade(512, 4): worst error / sqrt(S_aa S_bb) {err:.3g}")
    assert_sxy_close(got[4], sab, saa, sbb, 1e-5, "S_ab upper against the matrix object")
    m.close()


def test_iq_cross_routes_agree_bit_for_bit(pkg, gpu_required):
    """The same data by the four sample routes and by one frames call (host and device): equal bytes.  The data are the decoded
    traces of AdcDac frames, so that the frames route can carry them."""
    import torch
    n = 64
    batches, nf = 19, 260
    data, fs, tr = frames_of(pkg, 1, batches, nf, 4242)
    ia, qa, ib, qb = (np.array(t) for t in tr)
    length = ia.size
    assert length == nf * batches * 8
    za, zb = (ia + 1j * qa).astype(np.complex64), (ib + 1j * qb).astype(np.complex64)
    dev = [torch.from_numpy(v).cuda() for v in (ia, qa, ib, qb, za, zb)]
    dfr = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    ftw = (pkg.zoom_ftw(0.3)[0], pkg.zoom_ftw(0.123)[0])
    ph = (5, 1 << 63)
    got = {}
    for route in ("planar host", "planar device", "interleaved host", "interleaved device", "frames host", "frames device"):
        g = make(pkg, n, ftw, phase0=ph)
        if route == "planar host":
            g.process((ia, qa), (ib, qb))
        elif route == "planar device":
            g.process_device_planar(*[d.data_ptr() for d in dev[:4]], length)
        elif route == "interleaved host":
            g.process(za, zb)
        elif route == "interleaved device":
            g.process_device(dev[4].data_ptr(), dev[5].data_ptr(), length)
        elif route == "frames host":
            assert g.process_frames(data, fs, ((0, 1), (2, 3))) == nf
        else:
            assert g.process_frames_device(dfr.data_ptr(), fs, nf, ((0, 1), (2, 3))) == nf
        got[route] = bits(g)
        assert g.stats_read()["pairs_in"] == length and g.num_stages() >= 2
    for route in list(got)[1:]:
        assert_bits(got[route], got["planar host"], route)


def test_iq_cross_alignment_and_cuts(pkg, gpu_required):
    """Every source judged on its own: planar device sources offset by 0 ... 3 floats, each stream taking every offset while the
    others differ from it, and interleaved sources offset by 0 and 1 complex sample a side, in one call each; then the stream cut
    into calls of 1, 2, 3, 5, 9, 14 and 7 samples and the rest, which takes the destination offset through 1, 3, 2, 3, 0, 2, 1
    (mod 4) with heads of every length and partial last quads.  The short calls hold 41 samples together, fewer than one
    segment, so the last call's round plans the segments the one-call run plans: each case equals the one-call result by bytes."""
    import torch
    n = 64
    length = (1 << 15) + 37
    lens = [1, 2, 3, 5, 9, 14, 7]
    assert sum(lens) < n and {int(c) % 4 for c in np.cumsum([0] + lens)} == {0, 1, 2, 3}
    lens.append(length - sum(lens))
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    a, b = pair_iq(length, 71)
    flat = (a[0], a[1], b[0], b[1])
    za, zb = (a[0] + 1j * a[1]).astype(np.complex64), (b[0] + 1j * b[1]).astype(np.complex64)
    ftw = (pkg.zoom_ftw(0.123)[0], pkg.zoom_ftw(0.456)[0])
    ph = (0x0123456789ABCDEF, 77)
    one = make(pkg, n, ftw, phase0=ph)
    one.process(a, b)
    ref = bits(one)

    def planar_dev(offs):
        t = []
        for v, o in zip(flat, offs):
            x = torch.zeros(length + 4)
            x[o:o + length] = torch.from_numpy(v)
            t.append(x.cuda())
        torch.cuda.synchronize()
        return t

    def inter_dev(offs):
        t = []
        for z, o in zip((za, zb), offs):
            x = torch.zeros(length + 1, dtype=torch.complex64)
            x[o:o + length] = torch.from_numpy(z)
            t.append(x.cuda())
        torch.cuda.synchronize()
        return t

    offsets = [(0, 0, 0, 0), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (0, 1, 2, 3)]
    assert all({o[c] for o in offsets} == {0, 1, 2, 3} for c in range(4))
    for offs in offsets:
        t = planar_dev(offs)
        g = make(pkg, n, ftw, phase0=ph)
        g.process_device_planar(*[x.data_ptr() + 4 * o for x, o in zip(t, offs)], length)
        assert_bits(bits(g), ref, f"one call, planar sources offset by {offs} floats")
    for offs in ((0, 0), (1, 0), (0, 1), (1, 1)):
        t = inter_dev(offs)
        g = make(pkg, n, ftw, phase0=ph)
        g.process_device(*[x.data_ptr() + 8 * o for x, o in zip(t, offs)], length)
        assert_bits(bits(g), ref, f"one call, interleaved sources offset by {offs} complex samples")
    # the cut stream, by every route
    g = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        g.process(tuple(v[s:e] for v in a), tuple(v[s:e] for v in b))
    assert_bits(bits(g), ref, "planar host, cut")
    g = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        g.process(za[s:e], zb[s:e])
    assert_bits(bits(g), ref, "interleaved host, cut")
    offs = (1, 2, 3, 0)
    t = planar_dev(offs)
    g = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        g.process_device_planar(*[x.data_ptr() + 4 * (o + int(s)) for x, o in zip(t, offs)], int(e - s))
    assert_bits(bits(g), ref, "planar device, offset sources, cut")
    offs = (1, 0)
    t = inter_dev(offs)
    g = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        g.process_device(*[x.data_ptr() + 8 * (o + int(s)) for x, o in zip(t, offs)], int(e - s))
    assert_bits(bits(g), ref, "interleaved device, offset sources, cut")
    assert g.stats_read()["pairs_in"] == length
    # misaligned pointers are refused: an interleaved side off the 8-byte grid, a planar stream off the 4-byte grid
    L = pkg.lib()
    h = g._b._h
    p = [x.data_ptr() for x in t]
    assert L.psdc_iqcsd_process_interleaved_device(h, 0, C.c_void_p(p[0]), C.c_void_p(p[1] + 4), 10, None) == pkg.ERR_ARG
    assert "8 bytes" in L.psdc_iqcsd_last_error(h).decode()
    assert L.psdc_iqcsd_process_interleaved_device(h, 0, C.c_void_p(p[0] + 4), C.c_void_p(p[1]), 10, None) == pkg.ERR_ARG
    for k in range(4):
        q = [C.c_void_p(p[0] + (2 if c == k else 0)) for c in range(4)]
        assert L.psdc_iqcsd_process_device(h, 0, *q, 10, None) == pkg.ERR_ARG, k
        assert "4 bytes" in L.psdc_iqcsd_last_error(h).decode()
    assert g.stats_read()["pairs_in"] == length


@pytest.mark.parametrize("kind", ["equal carriers", "distinct carriers", "equal ftw, different phase0"])
def test_iq_cross_mixer_is_iq_lo(pkg, gpu_required, iq_emul, kind):  # noqa: F811
    """The route by which the IQ suite anchors its mixer, for the pair mixer and both of its branches: a pair with the carriers
    (ftw, phase0) gives the bytes of a carrier-0 pair fed csrc/iq_lo.h's output of each side (mix_c_f32: the header run on the
    host; with carrier 0 the mixer returns finite input unchanged).  Equal (ftw, phase0) takes the shared-oscillator branch;
    distinct carriers, and equal ftw with different phase0, take the two-oscillator branch."""
    n, length = 64, (1 << 15) + 3
    a, b = pair_iq(length, 23)
    f = pkg.zoom_ftw(0.2345678901234567)[0]
    ftw, ph = {"equal carriers": ((f, f), (0x9E3779B97F4A7C15, 0x9E3779B97F4A7C15)),
               "distinct carriers": ((f, pkg.zoom_ftw(0.7131313131313131)[0]), (1, 1 << 63)),
               "equal ftw, different phase0": ((f, f), (0, 1 << 62))}[kind]
    g = make(pkg, n, ftw, phase0=ph)
    g.process(a, b)
    ma = mix_c_f32(iq_emul, a[0], a[1], ftw[0], ph[0])
    mb = mix_c_f32(iq_emul, b[0], b[1], ftw[1], ph[1])
    assert not any(np.any(v == 0) for v in (*ma, *mb))  # (the identity holds up to the sign of a zero: there is none)
    z = make(pkg, n, (0, 0))
    z.process(ma, mb)
    assert_bits(bits(g), bits(z), kind)
    # and through the interleaved kernel
    gi = make(pkg, n, ftw, phase0=ph)
    gi.process((a[0] + 1j * a[1]).astype(np.complex64), (b[0] + 1j * b[1]).astype(np.complex64))
    assert_bits(bits(gi), bits(z), kind + ", interleaved")


def test_iq_cross_phase_continuity_and_carrier_rule(pkg, gpu_required):
    """A stream cut into sample calls (all four routes) and frames calls (host and device) equals one call: the 64-bit stream
    index, and so both phases, continues across calls and routes.  N = 1024 and the cut calls hold fewer than 1024 samples
    before the last one, so the rounds coincide and the comparison is by bytes; the same stream cut into large calls is held to
    the header's chunking bound (2e-6).  Then the carrier rule."""
    import torch
    n = 1024
    batches, nf = 17, 3000
    data, fs, tr = frames_of(pkg, 3, batches, nf, 515)
    ia, qa, ib, qb = (np.array(t) for t in tr)
    length = ia.size
    za, zb = (ia + 1j * qa).astype(np.complex64), (ib + 1j * qb).astype(np.complex64)
    dev = [torch.from_numpy(v).cuda() for v in (ia, qa, ib, qb, za, zb)]
    dfr = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    ftw = (pkg.zoom_ftw(0.2)[0], pkg.zoom_ftw(0.2)[0] + 12345)
    ph = (3, 1 << 61)
    pair = ((0, 1), (2, 3))
    one = make(pkg, n, ftw, phase0=ph)
    one.process((ia, qa), (ib, qb))
    ref = bits(one)

    def feed(g, route, f0, f1):
        s, e = f0 * batches, f1 * batches
        if route == "planar":
            g.process((ia[s:e], qa[s:e]), (ib[s:e], qb[s:e]))
        elif route == "interleaved":
            g.process(za[s:e], zb[s:e])
        elif route == "planar device":
            g.process_device_planar(*[d.data_ptr() + 4 * s for d in dev[:4]], e - s)
        elif route == "interleaved device":
            g.process_device(dev[4].data_ptr() + 8 * s, dev[5].data_ptr() + 8 * s, e - s)
        elif route == "frames":
            assert g.process_frames(data[f0 * fs:f1 * fs], fs, pair) == f1 - f0
        else:
            assert g.process_frames_device(dfr.data_ptr() + f0 * fs, fs, f1 - f0, pair) == f1 - f0

    routes = ["planar", "frames", "interleaved", "frames device", "planar device", "interleaved device", "frames"]
    small = [0, 3, 10, 11, 25, 30, 41, 55]  # frames: 55 * 17 = 935 samples < n
    assert small[-1] * batches < n
    g = make(pkg, n, ftw, phase0=ph)
    for r, f0, f1 in zip(routes, small[:-1], small[1:]):
        feed(g, r, f0, f1)
    feed(g, "planar", small[-1], nf)
    assert_bits(bits(g), ref, "short calls by every route, then the rest")
    big = [0, 301, 1000, 1001, 1777, 2500, 2999, nf]
    g2 = make(pkg, n, ftw, phase0=ph)
    for r, f0, f1 in zip(routes, big[:-1], big[1:]):
        feed(g2, r, f0, f1)
    assert g2.stats_read()["pairs_in"] == length
    c2, cr = g2.csd(), ref[0]
    assert c2[6] == cr[6]
    for u, v in zip(c2[:4], cr[:4]):
        assert np.all(np.abs(u - v) <= 2e-6 * v)
    assert_cross_rows(c2, cr, 2e-6, "large calls by every route")
    # a carrier is set before the first sample only, by whichever route the sample came
    for route in ("planar", "frames"):
        bank = pkg.IqCsdCascadeBank(n, 2)
        bank.set_carrier(0, ftw=ftw[0], phase0=7)
        if route == "planar":
            bank.process(0, (ia[:10], qa[:10]), (ib[:10], qb[:10]))
        else:
            assert bank.process_frames(data[:2 * fs], fs, [pair]) == 2
        for side in (0, 1):
            with pytest.raises(pkg.PsdError) as err:
                bank.set_carrier(0, ftw=1, side=side)
            assert err.value.code == pkg.ERR_ARG and "before the first" in str(err.value)
        bank.set_carrier(1, ftw=ftw[1], side=1)  # a pair the call (the map) left out is still free
        assert bank.carriers[(1, 1)] == (ftw[1], 0)
        bank.reset()
        assert all(v == (0, 0) for v in bank.carriers.values())
        bank.process(0, (ia[:50_000], qa[:50_000]), (ib[:50_000], qb[:50_000]))
        z0 = pkg.IqCsdCascade(n)
        z0.process((ia[:50_000], qa[:50_000]), (ib[:50_000], qb[:50_000]))
        assert_bits(bits(bank), bits(z0), "a bank's reset puts the carriers back to 0")


def raw_frames_call(pkg, bank, data_or_ptr, fs, nf, m, device=False):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    bank = getattr(bank, "_b", bank)
    mp = np.asarray(m, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None
    ok = C.c_size_t(77)
    if device:
        rc = L.psdc_iqcsd_process_frames_device(bank._h, mp, C.c_void_p(data_or_ptr), fs, nf, C.byref(ok), None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_iqcsd_process_frames(bank._h, mp, buf.ctypes.data_as(C.c_void_p), fs, nf, C.byref(ok))
    return rc, ok.value


# the issue's table: (format, batches, (I_a, Q_a, I_b, Q_b)); batches odd for the one-sample formats: the second call starts off the
# 16-byte grid and calls end in a partial run of the four-batch threads
@pytest.mark.parametrize("fmt,batches,four", [(1, 19, (0, 1, 2, 3)), (2, 25, ("BI", "BQ", "AR", "AP")), (3, 17, (3, 1, 0, 2)),
                                              (4, 61, (0, 1, 2, 2))])
def test_iq_cross_frames_against_the_sample_route(pkg, gpu_required, fmt, batches, four):
    """Calls of one piece each: the same bytes as the planar sample route fed Payload::traces at the same cuts, from host and from
    device memory (base offsets 0 and 1: the aligned loads, then bytes); different carriers, then one carrier on both sides."""
    import torch
    n = 64
    spf = batches * (8 if fmt == 1 else 1)
    nf = 40_000 // spf
    data, fs, tr = frames_of(pkg, fmt, batches, nf, 10 * fmt + batches)
    x = [tr[pkg.trace_index(t)] for t in four]
    pair = ((four[0], four[1]), (four[2], four[3]))
    cuts = [0, 1, nf // 3, nf]
    host_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    f = pkg.zoom_ftw(0.2718281828459045)[0]
    for ftw, ph in (((f, pkg.zoom_ftw(0.41)[0]), (0x0123456789ABCDEF, 9)), ((f, f), (5, 5))):
        g, twin = make(pkg, n, ftw, phase0=ph), make(pkg, n, ftw, phase0=ph)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert g.process_frames(data[a * fs:b * fs], fs, pair) == b - a
            s = slice(a * spf, b * spf)
            twin.process((x[0][s], x[1][s]), (x[2][s], x[3][s]))
        assert g.num_stages() >= 2
        assert_bits(bits(g), bits(twin), f"format {fmt}, host frames")
        assert g.stats_read()["pairs_in"] == nf * spf
        assert g.loss() == {"received": nf * batches, "dropped": 0}
        for shift in (0, 1):
            buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
            buf[shift:shift + len(data)].copy_(host_bytes)
            torch.cuda.synchronize()
            d = make(pkg, n, ftw, phase0=ph)
            for a, b in zip(cuts[:-1], cuts[1:]):
                assert d.process_frames_device(buf.data_ptr() + shift + a * fs, fs, b - a, pair) == b - a
            assert_bits(bits(d), bits(g), f"format {fmt}, device frames at offset {shift}")
            assert d.loss() == g.loss()


def test_iq_cross_frames_gap_errors_and_nine_pairs(pkg, gpu_required):
    """A sequence gap in Loss; a map that names a trace the format lacks (PSDC_ERR_ARG at the run's first frame, *n_ok counting the
    frames before it); the map errors; and a 9-pair bank, which takes two decode launches a piece."""
    n = 64
    rng = np.random.default_rng(5)
    L = pkg.lib()
    # AdcDac (3 batches) and Mpll (8 batches) frames share frame_size 200; a gap of 7 batches at frame 6
    ad, fs = make_frames(1, 3, random_payloads(rng, 1, 3, 10, wild=False), seq0=0xFFFFFFF4)
    ad = bytearray(ad)
    for f in range(6, 10):
        seq = int.from_bytes(ad[f * fs + 4:f * fs + 8], "little")
        ad[f * fs + 4:f * fs + 8] = ((seq + 7) & 0xFFFFFFFF).to_bytes(4, "little")
    ad = bytes(ad)
    mp, fs2 = make_frames(4, 8, random_payloads(rng, 4, 8, 4, wild=False), seq0=100)
    assert fs == fs2 == 200
    from stabilizer_stream_amd import source
    dec = [source.decode_frame(ad[f * fs:(f + 1) * fs])[3] for f in range(10)]
    tr = [np.concatenate([d[c][1] for d in dec]).astype(np.float32) for c in range(4)]
    spf = 24
    car = ((pkg.zoom_ftw(0.2)[0], (1 << 63) - 1), (3, 9))

    def twin_of(four, frames=10):
        t = make(pkg, n, car[0], phase0=car[1])
        m = frames * spf
        t.process((tr[four[0]][:m], tr[four[1]][:m]), (tr[four[2]][:m], tr[four[3]][:m]))
        return bits(t)

    g = make(pkg, n, car[0], phase0=car[1])
    assert g.process_frames(ad, fs, (("ADC0", "DAC1"), ("ADC1", "ADC0"))) == 10  # a trace may feed several sides
    assert g.loss() == {"received": 30, "dropped": 7}
    assert_bits(bits(g), twin_of((0, 3, 1, 0)), "a gap is counted and the samples are taken")
    # Mpll has no trace 3: PSDC_ERR_ARG at the run's first frame, the AdcDac run before it is ingested and counted
    b1 = make(pkg, n, car[0], phase0=car[1])
    assert raw_frames_call(pkg, b1, ad + mp, fs, 14, [0, 1, 2, 3]) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_iqcsd_last_error(b1._b._h).decode()
    assert b1.stats_read()["pairs_in"] == 10 * spf
    assert_bits(bits(b1), twin_of((0, 1, 2, 3)), "the run before the refused one")
    import torch
    t = torch.from_numpy(np.frombuffer(ad + mp, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    db = make(pkg, n, car[0], phase0=car[1])
    assert raw_frames_call(pkg, db, t.data_ptr(), fs, 14, [0, 1, 2, 3], device=True) == (pkg.ERR_ARG, 10)
    assert db.loss() == b1.loss()
    assert_bits(bits(db), bits(b1), "device path after an error")
    # map errors ingest nothing: NULL, a trace >= 4, one to three PSDC_TRACE_NONE in a pair, no pair fed
    before = (g.stats_read()["pairs_in"], g.loss())
    for mm in (None, [0, 1, 2, 4], [0, NONE, 1, 2], [NONE, NONE, 1, 2], [NONE, NONE, NONE, 2], [NONE] * 4):
        assert raw_frames_call(pkg, g, ad, fs, 10, mm) == (pkg.ERR_ARG, 0), mm
        assert raw_frames_call(pkg, g, t.data_ptr(), fs, 10, mm, device=True) == (pkg.ERR_ARG, 0), mm
    assert (g.stats_read()["pairs_in"], g.loss()) == before
    # nine pairs in one call: every pair is its single object within the bank bound of the header (2e-6: the pairs share rounds)
    bank = pkg.IqCsdCascadeBank(n, 9)
    maps = [((p % 4, (p + 1) % 4), ((p + 2) % 4, (3 * p) % 4)) for p in range(9)]
    for p in range(9):
        bank.set_carrier(p, ftw=car[0][p % 2] + p, phase0=p)
    assert bank.process_frames(ad, fs, maps) == 10
    assert bank.stats_read()["pairs_in"] == 9 * 10 * spf
    for p in (0, 7, 8):
        s = pkg.IqCsdCascade(n, ftw=car[0][p % 2] + p, phase0=p)
        four = (*maps[p][0], *maps[p][1])
        s.process((tr[four[0]], tr[four[1]]), (tr[four[2]], tr[four[3]]))
        got, want = bank.csd(p), s.csd()
        assert got[6] == want[6]
        for u, v in zip(got[:4], want[:4]):
            assert np.all(np.abs(u - v) <= 2e-6 * v), p
        assert_cross_rows(got, want, 2e-6, f"pair {p} of nine")
    # a decode launch takes 8 pairs: steady one-piece calls with nine fed pairs are 2 + 3 launches, with eight 1 + 3
    data, fsz, _ = frames_of(pkg, 1, 20, 1200, 31)
    per = 150
    m9 = [((0, 1), (2, 3))] * 9
    for k in range(4):  # the first calls make the stages and grow the buffers
        bank.process_frames(data[k * per * fsz:(k + 1) * per * fsz], fsz, m9)
    bank.stats_read(reset=True)
    for k in range(4, 6):
        assert bank.process_frames(data[k * per * fsz:(k + 1) * per * fsz], fsz, m9) == per
    assert bank.stats_read(reset=True)["launches"] == 2 * (2 + 3)
    for k in range(6, 8):
        assert bank.process_frames(data[k * per * fsz:(k + 1) * per * fsz], fsz, m9[:8]) == per
    assert bank.stats_read()["launches"] == 2 * (1 + 3)


def test_iq_cross_bank(pkg, gpu_required):
    """Three pairs with different carriers against three single objects: bit for bit when fed and read out in turn."""
    n = 256
    lens = [100_000, 65_537, 1 << 16]
    step = [10_000, 33_333, 65_536]
    data = [pair_iq(m, 500 + i) for i, m in enumerate(lens)]
    car = [tuple(pkg.zoom_ftw(f)[0] for f in fs) for fs in ((0.2, 0.2), (0.0123456789, 0.75), (0.4999, 0.4999))]
    ph = [(0, 0), (1 << 63, 12345), ((1 << 64) - 1, 7)]
    bank = pkg.IqCsdCascadeBank(n, 3)
    for i in range(3):
        for side in (0, 1):
            bank.set_carrier(i, ftw=car[i][side], phase0=ph[i][side], side=side)
    for i in range(3):
        s = make(pkg, n, car[i], phase0=ph[i])
        a, b = data[i]
        for p in range(0, lens[i], step[i]):
            cut = (tuple(v[p:p + step[i]] for v in a), tuple(v[p:p + step[i]] for v in b))
            s.process(*cut)
            bank.process(i, *cut)
        assert_bits(bits(bank, i), bits(s), f"pair {i}, fed in turn")
    for i in range(3):
        assert bank.stats_read()["pairs_in"] == sum(lens)


def test_iq_cross_launch_count(pkg, gpu_required):
    """A steady-state one-piece sample call on one pair is PSDC_IQCSD_STEADY_LAUNCHES = 1 + 3 launches (pair mixer; segments,
    decimators, fold + tails), from device and from host memory, planar and interleaved; a one-piece frames call reads 4 from
    host memory and 5 from device memory (the header gather)."""
    import torch
    n, m = 1024, 1 << 17
    dz = [torch.randn(m, dtype=torch.complex64, device="cuda") for _ in range(2)]
    dp = [torch.randn(m, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    g = pkg.IqCsdCascade(n, f0=0.2)
    for _ in range(8):
        g.process_device(dz[0].data_ptr(), dz[1].data_ptr(), m)
    g.stats_read(reset=True)
    for _ in range(4):
        g.process_device(dz[0].data_ptr(), dz[1].data_ptr(), m)
        g.process_device_planar(*[d.data_ptr() for d in dp], m)
    assert g.stats_read(reset=True)["launches"] == pkg.IQCSD_STEADY_LAUNCHES * 8 == 32
    hz = np.ones(m, np.complex64)
    g.process(hz, hz)
    g.stats_read(reset=True)
    g.process(hz, hz)
    g.process((hz.real.copy(), hz.imag.copy()), (hz.real.copy(), hz.imag.copy()))
    assert g.stats_read(reset=True)["launches"] == pkg.IQCSD_STEADY_LAUNCHES * 2
    g.sync()
    assert g.num_stages() >= 3
    data, fs, _ = frames_of(pkg, 2, 25, 1600, 77)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    f = pkg.IqCsdCascade(64, f0=0.1)
    per = 200
    pair = (("BI", "BQ"), ("AR", "AP"))
    for k in range(4):
        f.process_frames_device(t.data_ptr() + k * per * fs, fs, per, pair)
    f.stats_read(reset=True)
    for k in range(4, 6):
        assert f.process_frames_device(t.data_ptr() + k * per * fs, fs, per, pair) == per
    assert f.stats_read(reset=True)["launches"] == 5 * 2
    for k in range(6, 8):
        assert f.process_frames(data[k * per * fs:(k + 1) * per * fs], fs, pair) == per
    assert f.stats_read()["launches"] == 4 * 2


def test_iq_cross_argument_errors_on_an_object(pkg, gpu_required):
    """What needs an object: pair and side out of range, Detrend::Linear, NULL pointers, unequal inputs."""
    L = pkg.lib()
    bank = pkg.IqCsdCascadeBank(256, 2)
    x = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    z = (x + 1j * x).astype(np.complex64)
    with pytest.raises(pkg.PsdError) as e:
        bank.process(2, (x, x), (x, x))
    assert e.value.code == pkg.ERR_ARG and "pair 2 out of range (n_pairs 2)" in str(e.value)
    assert L.psdc_iqcsd_set_carrier(bank._h, 2, 0, 1, 0) == pkg.ERR_ARG
    assert L.psdc_iqcsd_set_carrier(bank._h, 0, 2, 1, 0) == pkg.ERR_ARG
    assert "side 2 out of range" in L.psdc_iqcsd_last_error(bank._h).decode()
    with pytest.raises(pkg.PsdError) as e:
        bank.set_carrier(0, ftw=1, side=2)
    assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.PsdError) as e:
        bank.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED
    fp = pkg._fptr(x)
    for k in range(4):
        ptrs = [None if c == k else fp for c in range(4)]
        assert L.psdc_iqcsd_process(bank._h, 0, *ptrs, 10) == pkg.ERR_ARG, k
        assert "null sample pointer" in L.psdc_iqcsd_last_error(bank._h).decode()
        assert L.psdc_iqcsd_process_device(bank._h, 0, *[None if c == k else C.c_void_p(256) for c in range(4)], 10, None) == pkg.ERR_ARG
    zp = z.ctypes.data_as(C.POINTER(C.c_float))
    assert L.psdc_iqcsd_process_interleaved(bank._h, 0, zp, None, 10) == pkg.ERR_ARG
    assert L.psdc_iqcsd_process_interleaved(bank._h, 0, None, zp, 10) == pkg.ERR_ARG
    assert L.psdc_iqcsd_process_interleaved_device(bank._h, 0, None, None, 10, None) == pkg.ERR_ARG
    assert L.psdc_iqcsd_process(bank._h, 0, None, None, None, None, 0) == 0  # (an empty call is accepted, as everywhere)
    with pytest.raises(pkg.PsdError) as e:
        bank.process(0, (x, x), (x, x[:10]))
    assert e.value.code == pkg.ERR_ARG and "differ in length" in str(e.value)
    with pytest.raises(pkg.PsdError):
        bank.process(0, z, z[:10])
    with pytest.raises(pkg.PsdError):
        bank.process(0, z, (x, x))
    with pytest.raises(pkg.PsdError):
        bank.process(0, x, x)
    assert bank.num_stages(0) == 0 and bank.stats_read()["pairs_in"] == 0
    with pytest.raises(pkg.PsdError) as e:
        bank.stage_spectra(0, 0)
    assert e.value.code == pkg.ERR_ARG and "stage 0 out of range" in str(e.value)


def test_iq_cross_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --iq-pair on two raw planar pairs (four f32 files) against the object's csd() at the tool's print precision
    (test_iq_cli's method: the tool feeds about 2^20 samples a call, the stream here is shorter, the bound is the chunking bound
    2e-6 with the mean term for the bins the default detrend nulls)."""
    fs = 1000.0
    length = (1 << 17) + 777
    a, b = pair_iq(length, 41)
    tone = 2 * np.pi * 0.2001 * np.arange(length)
    a = ((a[0] + np.cos(tone)).astype(np.float32), (a[1] + np.sin(tone)).astype(np.float32))
    files = []
    for name, v in zip(("ia", "qa", "ib", "qb"), (*a, *b)):
        p = tmp_path / f"{name}.f32"
        v.astype("<f4").tofile(p)
        files.append(str(p))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--iq-pair", ":".join(files) + ":0.2", "--iq-pair",
                        ":".join(files[2:] + files[:2]), "--fs", str(fs), "--csv", str(tmp_path / "csv")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "iq pair ia.f32:qa.f32:ib.f32:qb.f32 @ 0.2" in r.stdout and "iq pair ib.f32:qb.f32:ia.f32:qa.f32 @ 0" in r.stdout
    for name, f0, sides in (("iqpair_ia_f32__qa_f32__ib_f32__qb_f32_0_2.csv", 0.2, (a, b)),
                            ("iqpair_ib_f32__qb_f32__ia_f32__qa_f32_0.csv", 0.0, (b, a))):
        d = np.loadtxt(tmp_path / "csv" / name, delimiter=",")
        bank = pkg.IqCsdCascadeBank(512, 1)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
        bank.set_detrend(pkg.Detrend.MEAN)
        bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
        bank.set_carrier(0, f0=f0)
        bank.process(0, *sides)
        aup, alo, bup, blo, xup, xlo, br = bank.csd(0)
        assert d.shape == (aup.size, 9)
        assert np.allclose(d[:, 0], pkg.Break.frequencies(br) * fs, rtol=1e-6, atol=0)
        for col, want in ((1, aup), (2, bup), (3, xup.real), (4, xup.imag), (5, alo), (6, blo), (7, xlo.real), (8, xlo.imag)):
            scale = np.sqrt((aup if col < 5 else alo).astype(np.float64) * (bup if col < 5 else blo)) if col in (3, 4, 7, 8) else want
            assert np.all(np.abs(d[:, col] - want) <= 2e-6 * scale + 1e-6 * np.mean(scale)), (name, col)
    d = np.loadtxt(tmp_path / "csv" / "iqpair_ia_f32__qa_f32__ib_f32__qb_f32_0_2.csv", delimiter=",")
    assert abs(d[int(np.argmax(d[:, 1])), 0] - 0.0001 * fs) <= 0.5 * fs / (512 * 8)  # the tone, 1e-4 fs above the carrier
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--iq-pair", ":".join(files[:3])],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "IA:QA:IB:QB" in r.stderr
