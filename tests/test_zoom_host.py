"""Zoom cascade (psdc_zoom_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "zoom cascade".

restate_zoom below is the yardstick of tests/test_gpu_zoom.py: the zoom cascade written out from integer phases, an f64 local
oscillator and the oracle's own pieces (detrend_apply, hbf_dec8), with numpy's FFT.  It is anchored to the oracle here: a
bin-aligned carrier only permutes the bins of the oracle's stage-0 spectrum, and ftw = 0 gives the oracle's cascade on both
rows.  Its complex64 sibling takes I and Q from csrc/zoom_lo.h itself (tests/host/zoom_emul.cpp) and does everything else in
f32: it shows, without a GPU, that the GPU test's bounds can be met in f32 on that test's own inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_psd_close
from test_cross_host import DRAIN, U32_MAX, _window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1

ZOOM_SYMBOLS = ["psdc_zoom_create", "psdc_zoom_create_window", "psdc_zoom_destroy", "psdc_zoom_reset", "psdc_zoom_set_detrend",
                "psdc_zoom_set_avg", "psdc_zoom_set_carrier", "psdc_zoom_process", "psdc_zoom_process_device", "psdc_zoom_sync",
                "psdc_zoom_num_stages", "psdc_zoom_stage_spectra", "psdc_zoom_psd", "psdc_zoom_stats_read", "psdc_zoom_last_error"]

_EMUL = {}


def zoom_emul(tmp_dir):
    """tests/host/zoom_emul.cpp compiled once a session (-ffp-contract=off: zoom_lo.h leaves nothing to contract anyway)."""
    if "exe" not in _EMUL:
        exe = os.path.join(str(tmp_dir), "zoom_emul")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "zoom_emul.cpp"), "-o", exe], check=True)
        _EMUL["exe"] = exe
    return _EMUL["exe"]


@pytest.fixture(scope="session")
def emul(tmp_path_factory):
    return zoom_emul(tmp_path_factory.mktemp("zoom_emul"))


def phases(length, ftw, phase0=0):
    """phi_j = phase0 + ftw j mod 2^64 as uint64 (numpy's unsigned arithmetic wraps, as the device's does)"""
    with np.errstate(over="ignore"):
        return np.uint64(phase0 & M64) + np.uint64(ftw & M64) * np.arange(length, dtype=np.uint64)


def mix_f64(x, ftw, phase0=0):
    """I, Q in f64 from the exact integer phases (the full 64 bits, rounded once to f64's 53)"""
    a = 2.0 * np.pi * (phases(x.size, ftw, phase0).astype(np.float64) / 18446744073709551616.0)
    xd = np.asarray(x, np.float32).astype(np.float64)
    return xd * np.cos(a), -xd * np.sin(a)


def mix_f32(emul, x, ftw, phase0=0):
    """I, Q as zoom_mix_kernel stores them: csrc/zoom_lo.h run on the host"""
    d = os.path.dirname(emul)
    fin, fout = os.path.join(d, "mix_in.f32"), os.path.join(d, "mix_out.f32")
    np.asarray(x, np.float32).tofile(fin)
    subprocess.run([emul, "mix", str(ftw & M64), str(phase0 & M64), fin, fout], check=True)
    iq = np.fromfile(fout, np.float32)
    return iq[:x.size].copy(), iq[x.size:].copy()


def restate_zoom(ora, x, n, ftw, phase0=0, window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64", iq=None,
                 schedule=None):
    """Zoom cascade of the stream x: per stage dict(count, avg, pending, upper, lower), stage 0 first.  prec "f64": truth (f64
    LO, numpy FFT); "f32": the complex64 sibling -- iq = (I, Q) from mix_f32, f32 detrend / decimator, complex64 FFT, f32 rows.
    schedule: a settings_schedule.Schedule of mid-stream set_detrend / set_avg calls; it then replaces detrend and avg."""
    win, _, _, overlap, kind = _window(ora, n, window)
    hop = n - overlap
    h = n // 2 + 1
    ft = np.float64 if prec == "f64" else np.float32
    ct = np.complex128 if prec == "f64" else np.complex64
    si, sq = mix_f64(x, ftw, phase0) if iq is None else iq
    si, sq = np.asarray(si, ft), np.asarray(sq, ft)
    lower_idx = (n - np.arange(h)) % n
    stages = []
    k = 0
    while si.size:
        nseg = 0 if si.size < n else 1 + (si.size - n) // hop
        sh = 3 * k
        a = min((avg[1] >> sh) if sh < 32 else 0, avg[0])
        upper, lower = np.zeros(h, ft), np.zeros(h, ft)
        count = 0

        def prep(seg):  # detrend and window of one real segment (I and Q separately)
            if kind is not None:
                return ora.detrend_apply(seg, detrend, kind, prec).real
            return ora.detrend_apply(seg, detrend, "rect", prec).real * win.astype(ft)

        for j in range(nseg):
            if schedule is not None:  # the settings in force when segment j of stage k completed
                detrend, a = schedule.stage(k, j)
            z = (prep(si[j * hop:j * hop + n]) + 1j * prep(sq[j * hop:j * hop + n])).astype(ct)
            Z = np.fft.fft(z) if prec == "f64" else ora.fft_forward(z, "f32").astype(ct)
            p = (Z.real * Z.real + Z.imag * Z.imag).astype(ft)
            g = 1.0
            if count > a:
                g = float(np.float32(a) / np.float32(count))  # src/psd.rs:220: defined in f32
                count = a
            count += 1
            upper = ft(g) * upper + p[:h]
            lower = ft(g) * lower + p[lower_idx]
        pending = si.size if nseg == 0 else si.size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, upper=upper, lower=lower))
        p = nseg * hop + overlap if nseg else 0
        si = ora.hbf_dec8(si[:p], prec)[DRAIN:].astype(ft)
        sq = ora.hbf_dec8(sq[:p], prec)[DRAIN:].astype(ft)
        k += 1
    return stages


def stitch_zoom(pkg, n, window, stages, opts=None):
    """(upper, lower, breaks) of a restatement: pkg.stitch (psdc_stitch_window) on each row"""
    opts = opts or pkg.MergeOpts()
    wt = window if isinstance(window, pkg.WindowTable) else pkg.WindowTable._kind(n, window)
    args = ([s["count"] for s in stages], [s["avg"] for s in stages], [s["pending"] for s in stages])
    up, br = pkg.stitch(n, *args, np.stack([s["upper"] for s in stages]).astype(np.float32), opts, window=wt)
    lo, br2 = pkg.stitch(n, *args, np.stack([s["lower"] for s in stages]).astype(np.float32), opts, window=wt)
    assert br == br2
    return up, lo, br


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def custom_window(pkg, n):
    """a caller's table: sqrt-Hann, overlap n/4 -- (package window, oracle window)"""
    w = np.sqrt(pkg.WindowTable.hann(n).win).astype(np.float32)
    return pkg.WindowTable(w, 0.5, 1.2, n // 4), (w, 0.5, 1.2, n // 4)


def windows_of(pkg, n, kind):
    if kind == "hann":
        return pkg.Window.HANN, "hann"
    if kind == "rect":
        return pkg.Window.RECTANGULAR, "rect"
    return custom_window(pkg, n)


def carrier_ftw(pkg, n, carrier):
    """("bin", j): bin j of the n-point transform, exactly; a number: zoom_ftw of it"""
    if isinstance(carrier, tuple):
        return (carrier[1] << 64) // n
    return pkg.zoom_ftw(carrier)[0]


# The parity cases of tests/test_gpu_zoom.py: (n, window, detrend, avg, carrier, length).  Sizes 64 ... 4096; Hann, rectangular
# and a caller's window; every detrend; pure sums and both EWMA forms; carriers on a bin, "irrational" and above 0.5.
PARITY_CASES = [
    (64, "hann", "none", None, ("bin", 5), 1 << 17),
    (256, "rect", "mean", None, 0.2345678901234567, 1 << 18),
    (512, "custom", "span", (U32_MAX, 1000), 0.7131313131313131, 1 << 18),
    (1024, "hann", "midpoint", (100, U32_MAX), 0.1 * 2 ** 0.5, 1 << 19),
    (4096, "hann", "none", None, 0.6180339887498949, 1 << 20),
    (1024, "custom", "none", (40, U32_MAX), 0.8660254037844386, 1 << 19),
    (256, "hann", "none", (U32_MAX, 700), ("bin", 37), 1 << 18),
    (512, "rect", "none", None, 3 ** 0.5 / 7, 1 << 18),
]


def parity_input(n, length):
    return noise(length, 1000 + n)


def test_zoom_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_zoom_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ZOOM_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_zoom_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert "2^-64 turn" in hdr and "upper[k] = g upper[k] + |Z[k]|^2" in hdr  # the semantics are written down


def test_zoom_lo_accuracy(emul):
    """zoom_lo against f64 cos / sin of the same 32-bit-truncated phase over 3.1e6 phases (every octant boundary +-64 steps, 2^21
    random 64-bit phases, a sweep of every octant): absolute error <= 2^-23, quarter turns exact.  The program asserts; the
    figure it prints is checked again here."""
    r = subprocess.run([emul, "check"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    m = re.search(r"zoom_lo: (\d+) phases, worst \|error\| ([0-9.e+-]+)", r.stdout)
    assert int(m.group(1)) >= 1 << 20 and float(m.group(2)) <= 2.0 ** -23


def test_zoom_lo_mix_matches_f64(emul):
    """The emulated mixer against the f64 one on a stream with a start phase: I and Q within 2^-23 |x| + the phase truncation"""
    x = noise(50_000, 9)
    ftw, ph0 = 0x3C6EF372FE94F82B, 0x9E3779B97F4A7C15
    i32, q32 = mix_f32(emul, x, ftw, ph0)
    i64, q64 = mix_f64(x, ftw, ph0)
    tol = (2.0 ** -23 + 2 * np.pi * 2.0 ** -32 + 2.0 ** -24) * np.abs(x.astype(np.float64))  # LO, truncation, the product's rounding
    assert np.all(np.abs(i32 - i64) <= tol) and np.all(np.abs(q32 - q64) <= tol)


def test_zoom_ftw_and_two_sided(pkg):
    assert pkg.zoom_ftw(0.25) == (1 << 62, 0.25)
    assert pkg.zoom_ftw(0.0) == (0, 0.0)
    assert pkg.zoom_ftw(1.25)[0] == 1 << 62  # wraps
    assert pkg.zoom_ftw(-0.25)[0] == 3 << 62
    assert pkg.zoom_ftw(1.0 - 2.0 ** -70)[0] == 0  # rounds up to a full turn, and wraps
    from fractions import Fraction
    ftw, f0 = pkg.zoom_ftw(Fraction(1, 3))
    assert ftw == round(Fraction(1 << 64, 3)) and abs(f0 - 1 / 3) < 1e-15
    assert pkg.zoom_ftw(0.2)[0] == round(Fraction(0.2) * (1 << 64))
    # two_sided of a stitched two-stage read-out (n = 64): ascending offsets, DC once, Nyquist once
    n = 64
    h = n // 2 + 1
    rows = np.arange(2 * h, dtype=np.float32).reshape(2, h) + 1
    up, br = pkg.stitch(n, [10, 10], [U32_MAX, U32_MAX], [0, 0], rows, pkg.MergeOpts())
    lo, _ = pkg.stitch(n, [10, 10], [U32_MAX, U32_MAX], [0, 0], rows + 100, pkg.MergeOpts())
    f = pkg.Break.frequencies(br)
    off, d = pkg.two_sided(up, lo, br)
    assert off.size == d.size == 2 * f.size - int(np.sum(f == 0)) - int(np.sum(f == 0.5))
    assert np.all(np.diff(off) > 0) and off[0] > -0.5 and off[-1] == 0.5 and np.sum(off == 0) == 1
    pos = off >= 0
    order = np.argsort(f, kind="stable")
    assert np.array_equal(off[pos], f[order]) and np.array_equal(d[pos], up[order])
    inner = (f[order] > 0) & (f[order] < 0.5)
    assert np.array_equal(off[~pos], -f[order][inner][::-1]) and np.array_equal(d[~pos], lo[order][inner][::-1])


def test_zoom_argument_errors(pkg):
    import ctypes as C
    L = pkg.lib()
    for n in (1000, 32, 8192, 0):
        with pytest.raises(pkg.PsdError) as e:
            pkg.ZoomCascadeBank(n, 1)
        assert e.value.code == pkg.ERR_ARG and "power of two in [64, 4096]" in str(e.value)
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not L.psdc_zoom_create_window(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in L.psdc_zoom_last_error(None).decode()
    assert not L.psdc_zoom_create_window(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in L.psdc_zoom_last_error(None).decode()
    assert not L.psdc_zoom_create(256, 7, 1, 0)
    assert "window_kind" in L.psdc_zoom_last_error(None).decode()
    assert not L.psdc_zoom_create(256, 1, 0, 0)
    assert "n_channels" in L.psdc_zoom_last_error(None).decode()
    assert L.psdc_zoom_process(None, 0, None, 4) == pkg.ERR_ARG
    assert "null handle" in L.psdc_zoom_last_error(None).decode()
    for rc in (L.psdc_zoom_process_device(None, 0, None, 4, None), L.psdc_zoom_sync(None), L.psdc_zoom_reset(None),
               L.psdc_zoom_set_carrier(None, 0, 1, 2), L.psdc_zoom_set_detrend(None, 0), L.psdc_zoom_set_avg(None, 1, 1),
               L.psdc_zoom_num_stages(None, 0), L.psdc_zoom_stage_spectra(None, 0, 0, None, None, None),
               L.psdc_zoom_psd(None, 0, 0, 1, 0, None, None, 0, None, None, 0, None),
               L.psdc_zoom_stats_read(None, C.byref(C.c_uint64()), None, 0)):
        assert rc == pkg.ERR_ARG
    L.psdc_zoom_destroy(None)


def test_zoom_no_gpu_fails_loudly(pkg):
    from conftest import has_gpu
    if has_gpu():
        pytest.skip("a HIP device is visible")
    with pytest.raises(pkg.PsdError) as e:
        pkg.ZoomCascade(1024, f0=0.2)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("n,window,j,length", [(64, "hann", 5, 20_000), (256, "rect", 100, 30_000), (128, "custom", 64, 20_000),
                                               (64, "hann", 0, 10_000)])
def test_restatement_bin_aligned_is_the_oracle(pkg, ora, n, window, j, length):
    """ftw = j 2^64 / N: the mixer turns segment s by a constant phase and shifts its bins by j, so stage-0 upper[k] is the oracle's
    stage-0 spectrum bin j + k (j + k <= N/2) and lower[k] its bin j - k (k <= j).  1e-9 relative, f64 against f64."""
    x = noise(length, 3 * n + j)
    owin = custom_window(pkg, n)[1] if window == "custom" else window
    st = restate_zoom(ora, x, n, (j << 64) // n, 0, owin)
    ref = ora.PsdCascade(n, "f64", window=owin)
    ref.process(x)
    r = ref.stage_spectrum(0)
    info = ref.stage_info(0)
    assert (info["count"], info["pending"]) == (st[0]["count"], st[0]["pending"])
    h = n // 2 + 1
    ku = np.arange(0, h - j)
    assert ku.size and np.max(np.abs(st[0]["upper"][ku] - r[j + ku]) / r[j + ku]) <= 1e-9
    kl = np.arange(0, j + 1)
    assert np.max(np.abs(st[0]["lower"][kl] - r[j - kl]) / r[j - kl]) <= 1e-9


@pytest.mark.parametrize("n,window,detrend,avg,length", [
    (64, "hann", "none", None, 40_000),
    (128, "rect", "mean", None, 30_000),
    (256, "hann", "span", (U32_MAX, 500), 60_000),
    (64, "custom", "midpoint", (40, U32_MAX), 30_000),
])
def test_restatement_ftw0_is_the_oracle_cascade(pkg, ora, n, window, detrend, avg, length):
    """ftw = 0: I = x and Q = 0, so both rows are the oracle's cascade psd of x: stages, counts, pendings, and the stitched psd to
    1e-9 relative (bins a detrend nulls: of the spectrum's mean)."""
    x = noise(length, n)
    pwin, owin = windows_of(pkg, n, window)
    avg = avg or (U32_MAX, U32_MAX)
    st = restate_zoom(ora, x, n, 0, 0, owin, detrend, avg)
    ref = ora.PsdCascade(n, "f64", window=owin)
    ref.set_detrend(detrend)
    ref.set_avg(*avg)
    ref.process(x)
    assert ref.num_stages == len(st)
    for k, s in enumerate(st):
        info = ref.stage_info(k)
        assert (info["count"], info["pending"]) == (s["count"], s["pending"]), k
        r = ref.stage_spectrum(k)
        floor = 1e-9 * np.mean(r) if detrend != "none" else 0.0
        for row in ("upper", "lower"):
            assert np.all(np.abs(s[row] - r) <= 1e-9 * r + floor), (row, k)
    p, rbr, _ = ref.psd()
    up, lo, br = stitch_zoom(pkg, n, pwin, st)
    assert len(br) == len(rbr) and up.shape == p.shape
    floor = 1e-6 * np.mean(p) if detrend != "none" else 0.0  # (the stitch works on f32 rows: 1e-9 holds before it, 1e-6 after)
    for row in (up, lo):
        assert np.all(np.abs(row - p) <= 2e-7 * p + floor)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_complex64_sibling_meets_the_gpu_bounds(pkg, ora, emul, case):
    """The complex64 sibling (I and Q from zoom_lo.h, everything in f32) on the exact inputs of the GPU parity test, against the
    f64 restatement, both rows: the pure 1e-5 of conftest.assert_psd_close where the GPU test asserts it (detrend none).  Under a
    detrend the GPU test uses the widened bound with this sibling as its f32 yardstick (a detrend nulls bin 0 of both rows, where
    no relative bound can hold); here the sibling must then stay inside that widened bound."""
    n, wkind, detrend, avg, carrier, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    x = parity_input(n, length)
    ftw = carrier_ftw(pkg, n, carrier)
    ref = stitch_zoom(pkg, n, pwin, restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg))
    sib = stitch_zoom(pkg, n, pwin, restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_f32(emul, x, ftw)))
    assert sib[2] == ref[2]
    for name, got, want in (("upper", sib[0], ref[0]), ("lower", sib[1], ref[1])):
        rel = assert_psd_close(got, want, f"complex64 sibling {name} case {case}", pure=detrend == "none")
        print(f"case {case} {name}: worst relative error {rel:.3g}")
