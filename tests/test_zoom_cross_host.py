"""Zoom cross cascade (psdc_zcsd_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "zoom cross cascade".

restate_zoom_cross below is the yardstick of tests/test_gpu_zoom_cross.py: restate_zoom (tests/test_zoom_host.py) on two channels
at once, with conj(Z_a) Z_b added.  It is anchored to that restatement here -- its auto rows are restate_zoom's of each channel
alone -- and restate_zoom is anchored to the oracle in its own module."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, U32_MAX, _window
from test_zoom_host import M64, mix_f64, noise, restate_zoom, windows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZCSD_SYMBOLS = ["psdc_zcsd_supported", "psdc_zcsd_create", "psdc_zcsd_create_window", "psdc_zcsd_destroy", "psdc_zcsd_reset",
                "psdc_zcsd_set_detrend", "psdc_zcsd_set_avg", "psdc_zcsd_set_carrier", "psdc_zcsd_process",
                "psdc_zcsd_process_device", "psdc_zcsd_sync", "psdc_zcsd_num_stages", "psdc_zcsd_stage_spectra", "psdc_zcsd_csd",
                "psdc_zcsd_stats_read", "psdc_zcsd_last_error"]

ROWS = ("saa_up", "saa_lo", "sbb_up", "sbb_lo", "re_up", "re_lo", "im_up", "im_lo")  # the row table of the header, in order


def restate_zoom_cross(ora, xa, xb, n, ftw, phase0=(0, 0), window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64",
                       iq=None, schedule=None):
    """Zoom cross cascade of the streams xa, xb with the carriers ftw = (ftw_a, ftw_b): per stage dict(count, avg, pending,
    rows (8, n/2 + 1) in the header's order), stage 0 first.  prec / iq as restate_zoom: "f64" is truth; "f32" the complex64
    sibling with iq = ((I_a, Q_a), (I_b, Q_b)) from mix_f32.  schedule as restate_zoom takes it."""
    win, _, _, overlap, kind = _window(ora, n, window)
    hop = n - overlap
    h = n // 2 + 1
    ft = np.float64 if prec == "f64" else np.float32
    ct = np.complex128 if prec == "f64" else np.complex64
    if iq is None:
        iq = (mix_f64(xa, ftw[0], phase0[0]), mix_f64(xb, ftw[1], phase0[1]))
    s = [np.asarray(v, ft) for pair in iq for v in pair]  # I_a, Q_a, I_b, Q_b
    lower_idx = (n - np.arange(h)) % n
    stages = []
    k = 0
    while s[0].size:
        size = s[0].size
        nseg = 0 if size < n else 1 + (size - n) // hop
        sh = 3 * k
        a = min((avg[1] >> sh) if sh < 32 else 0, avg[0])
        rows = np.zeros((8, h), ft)
        count = 0

        def prep(seg):  # detrend and window of one real segment (each of the four streams separately)
            if kind is not None:
                return ora.detrend_apply(seg, detrend, kind, prec).real
            return ora.detrend_apply(seg, detrend, "rect", prec).real * win.astype(ft)

        def spec(si, sq, j):
            z = (prep(si[j * hop:j * hop + n]) + 1j * prep(sq[j * hop:j * hop + n])).astype(ct)
            return np.fft.fft(z) if prec == "f64" else ora.fft_forward(z, "f32").astype(ct)

        for j in range(nseg):
            if schedule is not None:  # the settings in force when segment j of stage k completed
                detrend, a = schedule.stage(k, j)
            Za, Zb = spec(s[0], s[1], j), spec(s[2], s[3], j)
            pa = (Za.real * Za.real + Za.imag * Za.imag).astype(ft)
            pb = (Zb.real * Zb.real + Zb.imag * Zb.imag).astype(ft)
            x = (np.conj(Za) * Zb).astype(ct)
            g = 1.0
            if count > a:
                g = float(np.float32(a) / np.float32(count))  # src/psd.rs:220: defined in f32
                count = a
            count += 1
            vals = (pa, pb, x.real.astype(ft), x.imag.astype(ft))
            new = np.stack([v[idx] for v in vals for idx in (slice(0, h), lower_idx)])
            rows = ft(g) * rows + new
        pending = size if nseg == 0 else size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, rows=rows))
        p = nseg * hop + overlap if nseg else 0
        s = [ora.hbf_dec8(v[:p], prec)[DRAIN:].astype(ft) for v in s]
        k += 1
    return stages


def stitch_zoom_cross(pkg, n, window, stages, opts=None):
    """(saa_up, saa_lo, sbb_up, sbb_lo, sab_up, sab_lo, breaks) of a restatement: pkg.stitch (psdc_stitch_window) on each row"""
    opts = opts or pkg.MergeOpts()
    wt = window if isinstance(window, pkg.WindowTable) else pkg.WindowTable._kind(n, window)
    args = ([s["count"] for s in stages], [s["avg"] for s in stages], [s["pending"] for s in stages])
    out, br = [], None
    for r in range(8):
        row, b = pkg.stitch(n, *args, np.stack([s["rows"][r] for s in stages]).astype(np.float32), opts, window=wt)
        assert br is None or b == br
        out.append(row)
        br = b
    return (out[0], out[1], out[2], out[3], (out[4] + 1j * out[6]).astype(np.complex64), (out[5] + 1j * out[7]).astype(np.complex64),
            br)


def pair_input(length, seed):
    """Channel b = 0.6 (a delayed by 3 samples) + independent noise: the coherence is neither 0 nor 1"""
    a = noise(length + 3, seed)
    b = (0.6 * a[:-3] + 0.8 * noise(length, seed + 7)).astype(np.float32)
    return a[3:].copy(), b


def test_zcsd_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_zcsd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ZCSD_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_zcsd_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    # the row table and the sign of S_ab are written down
    assert "S_ab[j] = conj(Z_a[j]) Z_b[j]" in hdr and "not conjugated" in hdr
    table = re.findall(r"\*\s+(S_aa = \|Z_a\|\^2|S_bb = \|Z_b\|\^2|Re S_ab|Im S_ab)\s+(\d)\s+(\d)\s*\n", hdr)
    assert [(int(u), int(lo)) for _, u, lo in table] == [(0, 1), (2, 3), (4, 5), (6, 7)]
    m = re.search(r"#define PSDC_ZCSD_STEADY_LAUNCHES (\d+)", hdr)
    assert m and int(m.group(1)) == pkg.ZCSD_STEADY_LAUNCHES <= 5  # at most 2 + 3


def test_zcsd_supported(pkg):
    for n in (64, 128, 256, 512, 1024, 2048):
        assert pkg.zcsd_supported(n), n
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.zcsd_supported(n), n
    assert pkg.zcsd_supported(4096) in (True, False)


def test_zoom_cross_bin_emulation(tmp_path):
    """csrc/zoom_cross_fft.h on the host (tests/host/zoom_cross_emul.cpp) against an f64 DFT, N = 64 and 1024, random complex
    inputs: each of the four values of every bin within 8 log2 N eps sqrt(S_aa S_bb) (the reasoning is in the program), and the
    eight rows as the header's table places them.  The program asserts; the figures it prints are checked again here."""
    exe = str(tmp_path / "zoom_cross_emul")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "zoom_cross_emul.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    got = re.findall(r"zoom_cross N=(\d+) worst ([0-9.e+-]+) bound ([0-9.e+-]+)", r.stdout)
    assert sorted({int(n) for n, _, _ in got}) == [64, 1024]
    for n, worst, bound in got:
        assert float(bound) == 8.0 * np.log2(int(n)) and float(worst) <= float(bound), (n, worst, bound)
    assert "WRONG" not in r.stdout


@pytest.mark.parametrize("n,window,detrend,avg,length", [
    (64, "hann", "none", None, 40_000),
    (128, "rect", "mean", None, 30_000),
    (256, "custom", "span", (U32_MAX, 500), 60_000),
    (64, "hann", "midpoint", (40, U32_MAX), 30_000),
])
def test_restatement_auto_rows_are_restate_zoom(pkg, ora, n, window, detrend, avg, length):
    """The auto rows of restate_zoom_cross are restate_zoom of each channel alone with that channel's carrier, to 1e-12
    relative; stages, counts and pendings equal.  (A check of the yardstick: it passes without the library's new code.)"""
    a, b = pair_input(length, 11 * n)
    _, owin = windows_of(pkg, n, window)
    avg = avg or (U32_MAX, U32_MAX)
    ftw = (pkg.zoom_ftw(0.2345678901234567)[0], pkg.zoom_ftw(0.7131313131313131)[0])
    ph = (0x0123456789ABCDEF, 1 << 63)
    st = restate_zoom_cross(ora, a, b, n, ftw, ph, owin, detrend, avg)
    for x, side in ((a, 0), (b, 1)):
        ref = restate_zoom(ora, x, n, ftw[side], ph[side], owin, detrend, avg)
        assert len(ref) == len(st)
        for k, (s, r) in enumerate(zip(st, ref)):
            assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
            for row, want in ((2 * side, r["upper"]), (2 * side + 1, r["lower"])):
                assert np.all(np.abs(s["rows"][row] - want) <= 1e-12 * np.abs(want)), (side, k, row)
    # with one carrier on both sides the input's coherence shows: neither 0 nor 1 (b = 0.6 a delayed + 0.8 noise: 0.36)
    s0 = restate_zoom_cross(ora, a[:20_000], b[:20_000], n, (ftw[0], ftw[0]), ph, owin)[0]["rows"]
    coh = (s0[4] ** 2 + s0[6] ** 2) / (s0[0] * s0[2])
    assert 0.2 < np.median(coh) < 0.6


def test_restatement_same_stream_and_conjugate_carriers(pkg, ora):
    """Two identities of the definition, in f64.  The same stream and carrier on both sides: S_ab = S_aa.  The same stream with
    ftw and -ftw (phase0 = 0): Z_b[k] = conj(Z_a[-k]), so S_bb upper is S_aa lower and the reverse, and S_ab upper is
    conj(Z_a[k] Z_a[-k]): symmetric in k <-> -k, so its lower row equals its upper row."""
    n = 128
    x = noise(30_000, 5)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    for s in restate_zoom_cross(ora, x, x, n, (ftw, ftw)):
        r = s["rows"]
        assert np.allclose(r[4], r[0], rtol=1e-12, atol=0) and np.allclose(r[5], r[1], rtol=1e-12, atol=0)
        assert np.all(np.abs(r[6]) <= 1e-12 * r[0]) and np.all(np.abs(r[7]) <= 1e-12 * r[1])
    for s in restate_zoom_cross(ora, x, x, n, (ftw, (-ftw) & M64)):
        r = s["rows"]
        scale = np.sqrt(r[0] * r[2])
        assert np.allclose(r[2], r[1], rtol=1e-9, atol=0) and np.allclose(r[3], r[0], rtol=1e-9, atol=0)
        assert np.all(np.abs(r[4] - r[5]) <= 1e-9 * scale) and np.all(np.abs(r[6] - r[7]) <= 1e-9 * scale)


def test_zcsd_argument_errors(pkg):
    """What can be refused without a device: sizes, windows, pair counts, NULL handles.  (Pair and side out of range and
    Detrend::Linear need an object: tests/test_gpu_zoom_cross.py.)"""
    import ctypes as C
    L = pkg.lib()
    for n in (1000, 32, 8192, 0):
        assert not pkg.zcsd_supported(n)
        with pytest.raises(pkg.PsdError) as e:
            pkg.ZoomCsdCascadeBank(n, 1)
        assert e.value.code == pkg.ERR_ARG and f"n = {n} is not supported" in str(e.value)
        w = np.ones(max(n, 1), np.float32)
        assert not L.psdc_zcsd_create_window(n, pkg._fptr(w), 1.0, 1.0, 0, 1, 0)
        assert f"n = {n} is not supported" in L.psdc_zcsd_last_error(None).decode()
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not L.psdc_zcsd_create_window(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in L.psdc_zcsd_last_error(None).decode()
    assert not L.psdc_zcsd_create_window(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in L.psdc_zcsd_last_error(None).decode()
    assert not L.psdc_zcsd_create(256, 7, 1, 0)
    assert "window_kind" in L.psdc_zcsd_last_error(None).decode()
    assert not L.psdc_zcsd_create(256, 1, 0, 0)
    assert "n_pairs" in L.psdc_zcsd_last_error(None).decode()
    assert L.psdc_zcsd_process(None, 0, None, None, 4) == pkg.ERR_ARG
    assert "null handle" in L.psdc_zcsd_last_error(None).decode()
    for rc in (L.psdc_zcsd_process_device(None, 0, None, None, 4, None), L.psdc_zcsd_sync(None), L.psdc_zcsd_reset(None),
               L.psdc_zcsd_set_carrier(None, 0, 0, 1, 2), L.psdc_zcsd_set_detrend(None, 0), L.psdc_zcsd_set_avg(None, 1, 1),
               L.psdc_zcsd_num_stages(None, 0), L.psdc_zcsd_stage_spectra(None, 0, 0, None, None),
               L.psdc_zcsd_csd(None, 0, 0, 1, 0, None, None, None, None, None, None, 0, None, None, 0, None),
               L.psdc_zcsd_stats_read(None, C.byref(C.c_uint64()), None, 0)):
        assert rc == pkg.ERR_ARG
    L.psdc_zcsd_destroy(None)
    with pytest.raises(pkg.PsdError) as e:
        pkg.ZoomCsdCascadeBank(256, 1, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG


def test_zcsd_no_gpu_fails_loudly(pkg):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    if has_gpu():
        pkg.ZoomCsdCascade(1024, f0=0.2).close()
        return
    with pytest.raises(pkg.PsdError) as e:
        pkg.ZoomCsdCascade(1024, f0=0.2)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)
