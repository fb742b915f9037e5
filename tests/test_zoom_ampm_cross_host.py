"""AM/PM cross cascades (psdc_zxampm_*, psdc_iqxampm_*): the parts that run without a GPU.  Semantics: include/psdcascade.h,
"AM/PM cross cascades".

restate_zoom_ampm_cross below is the yardstick of tests/test_gpu_zoom_ampm_cross.py: restate_zoom_cross of
tests/test_zoom_cross_host.py with the two complementary cross rows cab = sum w Z_a[k] Z_b[kn] and cba = sum w Z_a[kn] Z_b[k] kept
beside its eight.  It is anchored: its rows 0 ... 7 are restate_zoom_cross' rows bit for bit (f64, and the f32 sibling given the
same I and Q), and counts, averages, pendings and Breaks are equal.  What the GPU tests assert of am_pm_cross() and carriers() --
a common phase modulation under independent ones, the sign of a delay, (x, x) against the AM/PM object, the carriers' read-out, the
lock of a detuned carrier -- is checked on the f64 restatement first, so that the reference itself is inside the bounds the GPU is
held to.

The per-bin arithmetic of the kernel (csrc/zoom_ampm_cross_fft.h) runs on the host in tests/host/zoom_ampm_cross_emul.cpp, which
this file compiles itself: once plainly and once under the address and undefined-behaviour sanitizers (a stand-alone program;
nothing is loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, U32_MAX, _window
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_zoom_ampm_host import (PROP_BAND, PROP_BINS, PROP_F0, PROP_LEN, PROP_N, band_noise, prop_input, prop_restatement,  # noqa: F401
                                 stage_am_pm, stage_psd_scale)
from test_zoom_cross_host import pair_input, restate_zoom_cross, stitch_zoom_cross
from test_zoom_host import emul, mix_f32, mix_f64, noise, phases, windows_of  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = ["supported", "create", "create_window", "destroy", "reset", "set_detrend", "set_avg", "set_carrier", "sync", "num_stages",
           "stage_rows", "sidebands", "stats_read", "last_error"]
ZXAMPM_SYMBOLS = ["psdc_zxampm_" + s for s in _COMMON + ["process", "process_device"]]
IQXAMPM_SYMBOLS = ["psdc_iqxampm_" + s for s in _COMMON + ["process", "process_device", "process_interleaved", "process_interleaved_device"]]


def restate_zoom_ampm_cross(ora, xa, xb, n, ftw, phase0=(0, 0), window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64",
                            iq=None, max_stages=None, schedule=None):
    """AM/PM cross cascade of the streams xa, xb with the carriers ftw = (ftw_a, ftw_b): per stage dict(count, avg, pending,
    rows (8, n/2 + 1) computed as restate_zoom_cross computes them, cab, cba complex), stage 0 first.  prec / iq / schedule as
    restate_zoom_cross takes them.  max_stages: stop after that many stages (the property tests look at stage 0 only)."""
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
    while s[0].size and (max_stages is None or k < max_stages):
        size = s[0].size
        nseg = 0 if size < n else 1 + (size - n) // hop
        sh = 3 * k
        a = min((avg[1] >> sh) if sh < 32 else 0, avg[0])
        rows = np.zeros((8, h), ft)
        cab, cba = np.zeros(h, ct), np.zeros(h, ct)
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
            cab = (ft(g) * cab + (Za[:h] * Zb[lower_idx]).astype(ct)).astype(ct)
            cba = (ft(g) * cba + (Za[lower_idx] * Zb[:h]).astype(ct)).astype(ct)
        pending = size if nseg == 0 else size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, rows=rows, cab=cab, cba=cba))
        p = nseg * hop + overlap if nseg else 0
        s = [ora.hbf_dec8(v[:p], prec)[DRAIN:].astype(ft) for v in s]
        k += 1
    return stages


def twelve(stage):
    """the (12, n/2 + 1) f64 rows of a restated stage, in the header's order"""
    r = np.asarray(stage["rows"], np.float64)
    cab, cba = np.asarray(stage["cab"], np.complex128), np.asarray(stage["cba"], np.complex128)
    return np.concatenate([r, np.stack([cab.real, cab.imag, cba.real, cba.imag])])


def stage_carriers(pkg, n, count, rows):
    """carriers_from_rows of a stage 0's twelve raw rows, Hann"""
    return pkg.carriers_from_rows(n, pkg.WindowTable.hann(n).power, count, rows[0][0], rows[2][0], rows[3][0],
                                  rows[4][0] + 1j * rows[6][0], rows[8][0] + 1j * rows[9][0])


def stage_am_pm_cross(pkg, n, count, rows, carriers=None):
    """(s_am, s_pm, s_am_pm, s_pm_am, carriers) of one stage 0 from its twelve raw rows (a restated stage's through twelve(), or
    stage_rows()'s), Hann: the carriers from bin 0 unless they are given, the rows in the normalisation of psd()"""
    car = stage_carriers(pkg, n, count, rows) if carriers is None else carriers
    g = stage_psd_scale(pkg, n, count)
    r = np.asarray(rows, np.float64) * g
    return (*pkg.am_pm_cross_from_sidebands(r[4] + 1j * r[6], r[5] + 1j * r[7], r[8] + 1j * r[9], r[10] + 1j * r[11], *car[:3]), car)


# ---- the inputs of the properties, shared with tests/test_gpu_zoom_ampm_cross.py (each restatement is computed once a session) ----

XSEED = 20261020  # fixed; if a restatement missed a bound below, the seed or the input would change, never the bound
SIGMA_PHI = 3e-3  # of the common phase modulation and of each channel's own
SIGMA_A = 1e-3    # of each channel's own amplitude modulation
AMP = (0.8 * np.exp(0.7j), 0.5 * np.exp(-0.4j))  # A_a, A_b of the baseband carriers
DELAY = 3
DETUNE = 1e-5
# Margins: the worst deviation of the f64 restatement, in units of 1 / sqrt(count), as test_restatement_* print it (count 8191, bins
# 4 ... 45; DESIGN.md section 4.7 has the table), and the bound every reading is held to, three times that.
#   (a) the common part of two channels with equal independent parts: the cross spectrum of two half-coherent channels scatters
#       by about sqrt(S_aa S_bb) / sqrt(count_eff) = 2 S / sqrt(count_eff), count_eff ~ count / 1.06 under Hann at half overlap,
#       and the worst of 42 bins is near 2.5 sigma: about 5 is what to expect.
#   (b) one modulation on both channels: what is left is the scatter of the periodogram of phi itself about its density 2 sigma^2,
#       1 / sqrt(count_eff) a bin, about 3 for the worst of 42 bins.
K_MEASURED = {"common": 4.37, "common_real": 4.37, "delay": 3.23, "delay_real": 3.23}
K_FACTOR = 3.0


def xprop_modulation(case):
    """((a_a, phi_a), (a_b, phi_b)) in f64"""
    zero = np.zeros(PROP_LEN)
    base = case.replace("_real", "")
    if base == "common":  # (a)
        c = band_noise(SIGMA_PHI, XSEED)
        return ((band_noise(SIGMA_A, XSEED + 1), c + band_noise(SIGMA_PHI, XSEED + 2)),
                (band_noise(SIGMA_A, XSEED + 3), c + band_noise(SIGMA_PHI, XSEED + 4)))
    if base == "delay":  # (b): phi_b[n] = phi_a[n - 3]
        p = band_noise(SIGMA_PHI, XSEED + 5)
        return (zero, p), (zero, np.roll(p, DELAY))
    if base in ("const", "detuned"):  # (d), (e)
        return (zero, zero), (zero, zero)
    raise KeyError(case)


def xprop_input(pkg, case):
    """("iq", ((i_a, q_a), (i_b, q_b))) f32 of the complex carriers z_x = A_x (1 + a_x) exp(i phi_x); ("real", (x_a, x_b)) f32 of the
    real carriers 2 Re(z_x exp(2 pi i f0 j)) at the tuning word of PROP_F0 for the "_real" cases.  "detuned": carrier b turns by
    DETUNE cycles a sample."""
    mods = xprop_modulation(case)
    out = []
    for side, (a, phi) in enumerate(mods):
        if case == "detuned" and side == 1:
            phi = 2.0 * np.pi * ((DETUNE * np.arange(PROP_LEN)) % 1.0)
        out.append(AMP[side] * (1.0 + a) * np.exp(1j * phi))
    if case.endswith("_real"):
        ftw = pkg.zoom_ftw(PROP_F0)[0]
        w = 2.0 * np.pi * (phases(PROP_LEN, ftw).astype(np.float64) / 18446744073709551616.0)
        return "real", tuple((2.0 * (z * np.exp(1j * w)).real).astype(np.float32) for z in out)
    return "iq", tuple((z.real.astype(np.float32), z.imag.astype(np.float32)) for z in out)


_XPROP = {}


def restate_pair_stage0(pkg, ora, kind, v):
    """stage 0 of the f64 restatement of a pair given as xprop_input gives it"""
    if kind == "real":
        ftw = pkg.zoom_ftw(PROP_F0)[0]
        return restate_zoom_ampm_cross(ora, v[0], v[1], PROP_N, (ftw, ftw), max_stages=1)[0]
    iq = (mix_c_f64(v[0][0], v[0][1], 0), mix_c_f64(v[1][0], v[1][1], 0))
    return restate_zoom_ampm_cross(ora, None, None, PROP_N, (0, 0), iq=iq, max_stages=1)[0]


def xprop_restatement(pkg, ora, case):
    if case not in _XPROP:
        _XPROP[case] = restate_pair_stage0(pkg, ora, *xprop_input(pkg, case))
    return _XPROP[case]


def check_common(pkg, count, rows, what, case):
    """(a): s_pm within K / sqrt(count) of the common density 2 sigma_phi^2 at every in-band bin, K three times the restatement's"""
    _, s_pm, _, _, car = stage_am_pm_cross(pkg, PROP_N, count, rows)
    d = float(np.max(np.abs(s_pm[PROP_BINS] / (2 * SIGMA_PHI ** 2) - 1)))
    k = d * np.sqrt(count)
    print(f"{what}: count {count}, median Re s_pm / 2 sigma^2 {np.median(s_pm[PROP_BINS].real) / (2 * SIGMA_PHI ** 2):.4f}, worst "
          f"|s_pm / 2 sigma^2 - 1| {k:.2f} / sqrt(count) (measured on the restatement {K_MEASURED[case]}); locks {car[3]:.9f} {car[4]:.9f}")
    assert count == 8191
    assert k <= K_FACTOR * K_MEASURED[case], (what, k)
    return k


def check_delay(pkg, count, rows, what, case):
    """(b): phi_b[n] = phi_a[n - 3]: s_pm / (2 sigma_phi^2) within K / sqrt(count) of exp(-2 pi i 3 k / N): the sign convention
    s_pm = conj(phi_a) phi_b"""
    _, s_pm, _, _, _ = stage_am_pm_cross(pkg, PROP_N, count, rows)
    kk = np.arange(PROP_N // 2 + 1)[PROP_BINS]
    d = float(np.max(np.abs(s_pm[PROP_BINS] / (2 * SIGMA_PHI ** 2) - np.exp(-2j * np.pi * DELAY * kk / PROP_N))))
    k = d * np.sqrt(count)
    print(f"{what}: worst |s_pm / S_phi - exp(-2 pi i 3 k / N)| {k:.2f} / sqrt(count) (measured on the restatement {K_MEASURED[case]})")
    assert count == 8191
    assert k <= K_FACTOR * K_MEASURED[case], (what, k)
    return k


def const_truth(pkg):
    """(|A_a| |A_b|, arg w, arg q) of the constant inputs as the f32 samples hold them"""
    _, ((ia, qa), (ib, qb)) = xprop_input(pkg, "const")
    a, b = complex(float(ia[0]), float(qa[0])), complex(float(ib[0]), float(qb[0]))
    return abs(a) * abs(b), float(np.angle(np.conj(a) * b)), float(np.angle(a * b))


def check_const(pkg, count, rows, what, tol):
    """(d): constant carriers: p_ab (relative), arg w, arg q and both locks within tol"""
    p_ab, w, q, lock_w, lock_q = stage_carriers(pkg, PROP_N, count, rows)
    p0, aw, aq = const_truth(pkg)
    dw, dq = abs(float(np.angle(w * np.exp(-1j * aw)))), abs(float(np.angle(q * np.exp(-1j * aq))))
    print(f"{what}: p_ab relative error {abs(p_ab / p0 - 1):.3g}, arg w error {dw:.3g}, arg q error {dq:.3g}, 1 - lock_w "
          f"{1 - lock_w:.3g}, 1 - lock_q {1 - lock_q:.3g}")
    assert abs(p_ab / p0 - 1) <= tol and dw <= tol and dq <= tol and abs(1 - lock_w) <= tol and abs(1 - lock_q) <= tol, what
    return p_ab, w, q, lock_w, lock_q


# ---- the kernel's per-bin arithmetic on the host ----

_EMUL = {}


def zoom_ampm_cross_emul_exe(tmp_dir, sanitize):
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "zoom_ampm_cross_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "zoom_ampm_cross_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def zoom_ampm_cross_emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("zoom_ampm_cross_emul")


def run_zoom_ampm_cross_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    got = re.findall(r"zoom_ampm_cross N=(\d+) worst ([0-9.e+-]+) bound ([0-9.e+-]+) \((auto|cross)\)", r.stdout)
    assert sorted((int(n), row) for n, _, _, row in got) == [(64, "auto"), (64, "cross"), (1024, "auto"), (1024, "cross")]
    for n, worst, bound, row in got:
        # rows 0 ... 3 within 2e-6 nx^2, rows 4 ... 11 within 4e-6 nx^2: the AM/PM emulation's bounds for the same sums
        assert float(bound) == (2e-6 if row == "auto" else 4e-6) and float(worst) <= float(bound), (n, row, worst, bound)
    assert "WRONG" not in r.stdout and "FAIL" not in r.stdout
    # amplitude 1 at three scales, the EWMA amplitudes down to 2^-50, an inactive team
    for text in ("amp=1 ", "scale=0.001", "scale=1000", "amp=0.707 ", "amp=8.88e-16", "active=0"):
        assert text in r.stdout, text


def test_zoom_ampm_cross_bin_emulation(zoom_ampm_cross_emul_dir):
    """csrc/zoom_ampm_cross_fft.h for every lane against f64 DFTs at N = 64 and 1024: the twelve values of the bins the team
    transforms leave in the two frames, every (row, bin) written once, rows 8 ... 11 from FFT indices (k, kn) and (kn, k)
    (tests/host/zoom_ampm_cross_emul.cpp; the program asserts, the figures it prints are checked again here)"""
    run_zoom_ampm_cross_emul(zoom_ampm_cross_emul_exe(zoom_ampm_cross_emul_dir, sanitize=False))


def test_zoom_ampm_cross_bin_emulation_under_sanitizers(zoom_ampm_cross_emul_dir):
    """the same program built with -fsanitize=address,undefined: the team's frames and the partial rows have their exact sizes"""
    run_zoom_ampm_cross_emul(zoom_ampm_cross_emul_exe(zoom_ampm_cross_emul_dir, sanitize=True))


# ---- exports, arguments ----

CLASSES = ("ZoomAmPmCsdCascadeBank", "ZoomAmPmCsdCascade", "IqAmPmCsdCascadeBank", "IqAmPmCsdCascade")


def test_zoom_ampm_cross_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    L = pkg.lib()
    for prefix, symbols in (("psdc_zxampm_", ZXAMPM_SYMBOLS), ("psdc_iqxampm_", IQXAMPM_SYMBOLS)):
        declared = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr))
        assert declared == set(symbols)
        assert set(re.findall(r" T (" + prefix + r"[a-z0-9_]+)", out)) == declared
        assert declared <= set(pkg.EXPORTS)
        for name in symbols:  # mirrored in lib(): a prototype, not ctypes' default
            assert getattr(L, name).argtypes is not None, name
    assert L.psdc_abi_version() == 3
    # the host runtime reaches the kernel through the zoom cross launcher: the library exports no launcher of its own for it, and
    # the f32 sample routes only: no frames, Loss or integer feeds for the new handles, in the header or in the library
    for text in (hdr, out):
        assert not re.search(r"psdc_(zxampm|iqxampm)_process_frames|psdc_(zxampm|iqxampm)_loss_read|psdc_s?int_(zxampm|iqxampm)", text)
    for cls in CLASSES:
        for m in ("set_carrier", "process", "process_device", "set_detrend", "set_avg", "num_stages", "stage_rows", "csd", "sidebands",
                  "carriers", "am_pm_cross", "sync", "reset", "stats_read", "close"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)
        for m in ("process_frames", "process_frames_device", "loss", "process_int", "process_int_device"):
            assert not hasattr(getattr(pkg, cls), m), (cls, m)
        assert callable(getattr(getattr(pkg, cls), "process_device_planar", None)) == cls.startswith("Iq")
        doc = " ".join((getattr(pkg, cls).__doc__ + pkg.ZoomAmPmCsdCascadeBank.__doc__).split())
        for text in ("small-modulation", "second order", "locks", "tuning words", "bins 0 and 1"):
            assert text in doc, (cls, text)
    for fn in ("am_pm_cross_from_sidebands", "carriers_from_rows", "zoom_ampm_cross_supported"):
        assert callable(getattr(pkg, fn))
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "AM/PM cross cascades" in hdr
    for text in ("cab[k] = sum_j w_j Z_a,j[k] Z_b,j[kn]", "cba[k] = sum_j w_j Z_a,j[kn] Z_b,j[k]", "WITHOUT a conjugate",
                 "s_pm = conj(phi_a) phi_b = (T1 - T2 - T3 + T4) / (4 P)", "ONE set of Breaks", "no scratch memory",
                 "stream frames, the loss record and the integer feeds are not offered"):
        assert text in flat, text


def test_zoom_ampm_cross_supported(pkg):
    L = pkg.lib()
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        assert pkg.zoom_ampm_cross_supported(n) and L.psdc_iqxampm_supported(n) == 1 and L.psdc_zxampm_supported(n) == 1, n
        assert pkg.zcsd_supported(n)  # the zoom cross object's sizes
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.zoom_ampm_cross_supported(n) and L.psdc_iqxampm_supported(n) == 0, n
    assert not pkg.zoom_ampm_cross_supported(-1) and not pkg.zoom_ampm_cross_supported(1 << 32)


@pytest.mark.parametrize("family", ["zxampm", "iqxampm"])
def test_zoom_ampm_cross_argument_errors(pkg, family):
    """what is refused before any device is touched: sizes, windows, pair counts, null handles, and the pure functions' arguments"""
    import ctypes as C
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    f = lambda name: getattr(L, pre + name)  # noqa: E731
    bank = pkg.ZoomAmPmCsdCascadeBank if family == "zxampm" else pkg.IqAmPmCsdCascadeBank
    single = pkg.ZoomAmPmCsdCascade if family == "zxampm" else pkg.IqAmPmCsdCascade
    for n in (32, 8192, 1000, 0):
        with pytest.raises(pkg.PsdError) as e:
            bank(n, 1)
        assert e.value.code == pkg.ERR_ARG and pre + f"create: n = {n} is not supported" in str(e.value)  # the zoom cross kind's text
        with pytest.raises(pkg.PsdError) as e:
            single(n, f0=0.2)
        assert e.value.code == pkg.ERR_ARG
        w = np.ones(max(n, 1), np.float32)
        assert not f("create_window")(n, pkg._fptr(w), 1.0, 1.0, 0, 1, 0)
        assert pre + f"create_window: n = {n} is not supported" in f("last_error")(None).decode()
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not f("create_window")(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in f("last_error")(None).decode()
    assert not f("create_window")(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in f("last_error")(None).decode()
    assert not f("create")(256, 7, 1, 0)
    assert "window_kind" in f("last_error")(None).decode()
    for npairs in (0, 65537):
        assert not f("create")(256, 1, npairs, 0)
        assert "n_pairs must be in [1, 65536]" in f("last_error")(None).decode()
    with pytest.raises(pkg.PsdError) as e:
        bank(256, 1, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG
    # a null handle: every call, the carrier's included
    assert f("set_carrier")(None, 0, 0, 1, 2) == pkg.ERR_ARG
    assert pre + "set_carrier: null handle" in f("last_error")(None).decode()
    feeds = ([f("process")(None, 0, None, None, 4), f("process_device")(None, 0, None, None, 4, None)] if family == "zxampm" else
             [f("process")(None, 0, None, None, None, None, 4), f("process_device")(None, 0, None, None, None, None, 4, None),
              f("process_interleaved")(None, 0, None, None, 4), f("process_interleaved_device")(None, 0, None, None, 4, None)])
    for rc in feeds + [f("sync")(None), f("reset")(None), f("set_detrend")(None, 0), f("set_avg")(None, 1, 1), f("num_stages")(None, 0),
                       f("stage_rows")(None, 0, 0, None, None), f("sidebands")(None, 0, 0, 1, 0, None, 0, None, None, 0, None),
                       f("stats_read")(None, C.byref(C.c_uint64()), None, 0)]:
        assert rc == pkg.ERR_ARG
    f("destroy")(None)
    one = np.ones(3, complex)
    for bad in ((0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 0.0)):
        with pytest.raises(pkg.PsdError) as e:
            pkg.am_pm_cross_from_sidebands(one, one, one, one, *bad)
        assert e.value.code == pkg.ERR_ARG
    for bad in ((64, 0.25, 0, 1.0, 1.0, 1.0, 1.0, 1.0), (64, 0.25, 5, 1.0, 1.0, 1.0, 0.0, 1.0), (64, 0.25, 5, 1.0, 1.0, 1.0, 1.0, 0.0)):
        with pytest.raises(pkg.PsdError) as e:
            pkg.carriers_from_rows(*bad)
        assert e.value.code == pkg.ERR_ARG


@pytest.mark.parametrize("family", ["zxampm", "iqxampm"])
def test_zoom_ampm_cross_no_gpu_fails_loudly(pkg, family):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    make = (lambda: pkg.ZoomAmPmCsdCascade(1024, f0=0.2)) if family == "zxampm" else (lambda: pkg.IqAmPmCsdCascade(1024))
    if has_gpu():
        make().close()
        return
    with pytest.raises(pkg.PsdError) as e:
        make()
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value) and "psdc_" + family + "_create" in str(e.value)


# ---- the restatement is anchored ----

@pytest.mark.parametrize("n,window,detrend,avg,length", [
    (64, "hann", "none", None, 40_000),
    (128, "rect", "mean", None, 30_000),
    (256, "hann", "span", (U32_MAX, 500), 60_000),
    (64, "custom", "midpoint", (40, U32_MAX), 30_000),
])
def test_restatement_is_anchored(pkg, ora, emul, n, window, detrend, avg, length):  # noqa: F811
    """(1) rows 0 ... 7 are restate_zoom_cross' rows bit for bit, with a carrier a side, in f64 and in the f32 sibling given the
    same I and Q; (2) counts, averages, pendings and the stitched Breaks are equal; (3) cab == cba at k = 0 and N/2, and
    |cab| <= sqrt(saa_up sbb_lo), |cba| <= sqrt(saa_lo sbb_up) everywhere (Cauchy-Schwarz).  A check of the yardstick, not of the
    library."""
    a, b = pair_input(length, 11 * n)
    pwin, owin = windows_of(pkg, n, window)
    avg = avg or (U32_MAX, U32_MAX)
    ftw = (pkg.zoom_ftw(0.2345678901234567)[0], pkg.zoom_ftw(0.7131313131313131)[0])
    ph = (0x0123456789ABCDEF, 1 << 63)
    for prec in ("f64", "f32"):
        iq = None if prec == "f64" else (mix_f32(emul, a, ftw[0], ph[0]), mix_f32(emul, b, ftw[1], ph[1]))
        st = restate_zoom_ampm_cross(ora, a, b, n, ftw, ph, owin, detrend, avg, prec, iq=iq)
        rz = restate_zoom_cross(ora, a, b, n, ftw, ph, owin, detrend, avg, prec, iq=iq)
        assert len(st) == len(rz)
        for k, (s, r) in enumerate(zip(st, rz)):
            assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
            assert s["rows"].dtype == r["rows"].dtype and s["rows"].tobytes() == r["rows"].tobytes(), (prec, k)
            assert s["cab"].dtype == s["cba"].dtype == (np.complex128 if prec == "f64" else np.complex64)
            r64 = s["rows"].astype(np.float64)
            assert np.all(np.abs(s["cab"]) <= np.sqrt(r64[0] * r64[3]) * (1 + 1e-5) + 1e-30), k
            assert np.all(np.abs(s["cba"]) <= np.sqrt(r64[1] * r64[2]) * (1 + 1e-5) + 1e-30), k
            for bin_ in (0, n // 2):
                assert s["cab"][bin_] == s["cba"][bin_], (k, bin_)
        assert stitch_zoom_cross(pkg, n, pwin, st)[6] == stitch_zoom_cross(pkg, n, pwin, rz)[6]
    one = restate_zoom_ampm_cross(ora, a, b, n, ftw, ph, owin, detrend, avg, max_stages=1)
    assert twelve(one[0]).tobytes() == twelve(restate_zoom_ampm_cross(ora, a, b, n, ftw, ph, owin, detrend, avg)[0]).tobytes()


# ---- what am_pm_cross() and carriers() read on the f64 restatement ----

def xrows_of(s):
    return s["count"], twelve(s)


@pytest.mark.parametrize("case", ["common", "common_real"])
def test_restatement_common_phase_noise(pkg, ora, case):
    """(a): a common phi_c (sigma 3e-3) plus an independent phi of the same sigma and an independent AM on each channel, complex
    carriers and real ones at f0 = 0.2: s_pm is the common density.  The figure printed here is K_MEASURED."""
    k = check_common(pkg, *xrows_of(xprop_restatement(pkg, ora, case)), case, case)
    assert k >= K_MEASURED[case] / K_FACTOR  # the recorded figure is this restatement's, not a loose guess


@pytest.mark.parametrize("case", ["delay", "delay_real"])
def test_restatement_delay_fixes_the_sign(pkg, ora, case):
    """(b)"""
    k = check_delay(pkg, *xrows_of(xprop_restatement(pkg, ora, case)), case, case)
    assert k >= K_MEASURED[case] / K_FACTOR


@pytest.mark.parametrize("case", ["indep", "indep_real"])
def test_restatement_same_stream_is_the_ampm_object(pkg, ora, case):
    """(c): fed (x, x) with one carrier, (s_am, s_pm, s_am_pm, s_pm_am) are the AM/PM restatement's (s_am, s_pm, s_ampm,
    conj s_ampm) of x, to 1e-9 of S_am + S_pm: these two facts -- this one and the delay -- fix every sign.  Both sides are given
    ONE carrier, the AM/PM restatement's (power, u), as p_ab = power, w = 1, q = u: the pair's own read-out takes P from
    sab_up[0] = sum |Z_0|^2 where the AM/PM object takes it from |comp[0]| = |sum Z_0^2|, and the two differ by 1 - lock_q (5e-8
    on this modulated carrier), which is a property of the two carrier read-outs and not of the split."""
    kind, v = prop_input(pkg, case)
    s = restate_pair_stage0(pkg, ora, kind, (v, v))
    one = prop_restatement(pkg, ora, case)
    r_am, r_pm, r_x, (power, u, _) = stage_am_pm(pkg, PROP_N, one["count"], one["upper"], one["lower"], one["comp"])
    s_am, s_pm, s_ap, s_pa, _ = stage_am_pm_cross(pkg, PROP_N, *xrows_of(s), carriers=(power, 1.0, u))
    car = stage_carriers(pkg, PROP_N, *xrows_of(s))
    assert abs(car[0] / power - 1) <= 2 * (1 - car[4]) + 1e-12 and abs(car[2] - u) <= 1e-12  # the own read-out: q = u, P to 1 - lock_q
    tot = (r_am + r_pm)[PROP_BINS]
    errs = [float(np.max(np.abs(got[PROP_BINS] - want[PROP_BINS]) / tot))
            for got, want in ((s_am, r_am), (s_pm, r_pm), (s_ap, r_x), (s_pa, np.conj(r_x)))]
    print(f"(x, x) {case}: worst error / (S_am + S_pm) of s_am, s_pm, s_am_pm, s_pm_am {errs}; locks {car[3]:.12f} {car[4]:.12f}")
    assert s["count"] == one["count"] and max(errs) <= 1e-9, errs
    assert abs(car[1] - 1) <= 1e-12 and abs(car[3] - 1) <= 1e-12  # w = 1 and lock_w = 1: the channels are one


def test_restatement_constant_carriers(pkg, ora):
    """(d): p_ab within 1e-12 relative, arg w and arg q within 1e-12 rad, both locks within 1e-12 of 1"""
    check_const(pkg, *xrows_of(xprop_restatement(pkg, ora, "const")), "const", 1e-12)


def test_restatement_detuned_carrier_loses_lock(pkg, ora):
    """(e): carrier b detuned by 1e-5 fs turns 21 times against carrier a during the average: lock_w < 0.01"""
    count, rows = xrows_of(xprop_restatement(pkg, ora, "detuned"))
    car = stage_carriers(pkg, PROP_N, count, rows)
    print(f"b detuned by {DETUNE} fs: lock_w {car[3]:.3g} lock_q {car[4]:.3g}")
    assert car[3] < 0.01


def test_am_pm_cross_from_sidebands_is_pure(pkg):
    """the relations written out on made-up spectra: the carriers' phases turn the rows and nothing else"""
    rng = np.random.default_rng(7)
    cplx = lambda: rng.standard_normal(9) + 1j * rng.standard_normal(9)  # noqa: E731
    aa, pp, ap, pa = cplx(), cplx(), cplx(), cplx()  # conj(a_a) a_b, conj(phi_a) phi_b, conj(a_a) phi_b, conj(phi_a) a_b at +f
    aan, ppn, apn, pan = cplx(), cplx(), cplx(), cplx()  # the same at -f: x real, so x(-f) = conj x(f)
    for A, B in ((1.0, 1.0), (0.5 * np.exp(0.9j), -2.0j), AMP):
        P, w, q = abs(A) * abs(B), np.conj(A) * B / (abs(A) * abs(B)), A * B / (abs(A) * abs(B))
        # Z_x[k] = A_x (a_x[k] + i phi_x[k]), Z_x[kn] = A_x conj(a_x[k] - i phi_x[k]) for real modulations:
        #   conj(Z_a[k]) Z_b[k]   = P w (aa + pp + i ap - i pa)          conj(Z_a[kn]) Z_b[kn] = P w conj(aa + pp - i ap + i pa)
        #   Z_a[k] Z_b[kn]        = P q conj(aa - pp - i ap - i pa)      Z_a[kn] Z_b[k]        = P q (aa - pp + i ap + i pa)
        U = P * w * (aa + pp + 1j * ap - 1j * pa)
        Lo = P * w * np.conj(aa + pp - 1j * ap + 1j * pa)
        cab = P * q * np.conj(aa - pp - 1j * ap - 1j * pa)
        cba = P * q * (aa - pp + 1j * ap + 1j * pa)
        got = pkg.am_pm_cross_from_sidebands(U, Lo, cab, cba, P, w, q)
        for g, want in zip(got, (aa, pp, ap, pa)):
            assert g.dtype == np.complex128 and np.allclose(g, want, rtol=1e-12, atol=1e-12)
    del aan, ppn, apn, pan
