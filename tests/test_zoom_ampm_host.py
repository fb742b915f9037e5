"""AM/PM cascades (psdc_zampm_*, psdc_iqampm_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "AM/PM
cascades".

restate_zoom_ampm below is the yardstick of tests/test_gpu_zoom_ampm.py: restate_zoom of tests/test_zoom_host.py with the
complementary row comp = sum w Z_k Z_(N-k) kept beside upper and lower.  It is anchored: its rows 0 and 1 are restate_zoom's rows bit
for bit (f64, and the f32 sibling given the same I and Q), and counts, averages, pendings and Breaks are equal.  What the GPU tests
assert of am_pm() and carrier() -- S_am and S_pm of independent modulations, the sign of the AM-PM cross spectrum, AM only, PM only,
the carrier read-out, the lock of a detuned carrier -- is checked on the f64 restatement first, so that the reference itself is
inside the bounds the GPU is held to.

The per-bin arithmetic of the kernel (csrc/zoom_ampm_fft.h) runs on the host in tests/host/zoom_ampm_emul.cpp, which this file
compiles itself: once plainly and once under the address and undefined-behaviour sanitizers (a stand-alone program; nothing is
loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, U32_MAX, _window
from test_iq_host import mix_c_f64
from test_zoom_host import emul, mix_f32, mix_f64, noise, phases, restate_zoom, stitch_zoom, windows_of  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = ["supported", "create", "create_window", "destroy", "reset", "set_detrend", "set_avg", "set_carrier", "sync", "num_stages",
           "stage_rows", "psd", "sidebands", "stats_read", "last_error"]
ZAMPM_SYMBOLS = ["psdc_zampm_" + s for s in _COMMON + ["process", "process_device"]]
IQAMPM_SYMBOLS = ["psdc_iqampm_" + s for s in _COMMON + ["process", "process_device", "process_interleaved", "process_interleaved_device"]]


def restate_zoom_ampm(ora, x, n, ftw, phase0=0, window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64", iq=None,
                      max_stages=None, schedule=None):
    """AM/PM cascade of the stream x: per stage dict(count, avg, pending, upper, lower, comp), stage 0 first; upper / lower are
    computed as restate_zoom computes them, comp[k] = sum w Z[k] Z[(N - k) mod N] is complex.  prec, iq and schedule as restate_zoom
    takes them.  max_stages: stop after that many stages (the property tests look at stage 0 only)."""
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
    while si.size and (max_stages is None or k < max_stages):
        nseg = 0 if si.size < n else 1 + (si.size - n) // hop
        sh = 3 * k
        a = min((avg[1] >> sh) if sh < 32 else 0, avg[0])
        upper, lower, comp = np.zeros(h, ft), np.zeros(h, ft), np.zeros(h, ct)
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
            c = (Z[:h] * Z[lower_idx]).astype(ct)
            g = 1.0
            if count > a:
                g = float(np.float32(a) / np.float32(count))  # src/psd.rs:220: defined in f32
                count = a
            count += 1
            upper = ft(g) * upper + p[:h]
            lower = ft(g) * lower + p[lower_idx]
            comp = (ft(g) * comp + c).astype(ct)
        pending = si.size if nseg == 0 else si.size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, upper=upper, lower=lower, comp=comp))
        p = nseg * hop + overlap if nseg else 0
        si = ora.hbf_dec8(si[:p], prec)[DRAIN:].astype(ft)
        sq = ora.hbf_dec8(sq[:p], prec)[DRAIN:].astype(ft)
        k += 1
    return stages


def stage_psd_scale(pkg, n, count, window=None):
    """1 / PsdStage::gain of a stage-0 row: what psd() multiplies a raw accumulator by (decimation 1)"""
    wt = window if isinstance(window, pkg.WindowTable) else pkg.WindowTable.hann(n)
    return 1.0 / ((n // 2) * count * float(wt.nenbw) * float(wt.power))


def stage_am_pm(pkg, n, count, upper, lower, comp, carrier=None):
    """(s_am, s_pm, s_ampm, (power, u, lock)) of one stage 0 from its raw rows (a restated stage's or stage_rows()'s), Hann: the
    carrier from bin 0 unless it is given, the rows in the normalisation of psd()"""
    power, u, lock = pkg.carrier_from_rows(n, pkg.WindowTable.hann(n).power, count, upper[0], lower[0], comp[0])
    if carrier is None:
        carrier = np.sqrt(power) * np.sqrt(complex(u))
    g = stage_psd_scale(pkg, n, count)
    return (*pkg.am_pm_from_sidebands(upper * g, lower * g, comp * g, carrier), (power, u, lock))


# ---- the inputs of the properties, shared with tests/test_gpu_zoom_ampm.py (each restatement is computed once a session) ----

PROP_N = 512
PROP_LEN = 1 << 21
PROP_SEED = 20261019  # fixed; if a restatement missed a bound below, the seed or the input would change, never the bound
PROP_F0 = 0.2
PROP_BAND = 0.1       # the modulations are white, band-limited to 0.1 fs
PROP_BINS = slice(4, 46)  # the in-band bins 4 ... 45 of stage 0 the properties are judged at
SIGMA_A, SIGMA_PHI = 1e-3, 3e-3
A0, THETA = 0.8, 0.7
DETUNE = 1e-5


def band_noise(sigma, seed, length=PROP_LEN):
    """white Gaussian noise of standard deviation sigma (one-sided density 2 sigma^2), everything at and above PROP_BAND removed"""
    v = np.random.default_rng(seed).standard_normal(length) * sigma
    V = np.fft.rfft(v)
    V[int(PROP_BAND * length):] = 0.0
    return np.fft.irfft(V, length)


def prop_modulation(case):
    """(a, phi) in f64"""
    zero = np.zeros(PROP_LEN)
    if case in ("indep", "indep_real"):  # (a)
        return band_noise(SIGMA_A, PROP_SEED), band_noise(SIGMA_PHI, PROP_SEED + 1)
    if case == "delay":  # (b): phi[n] = 2 a[n - 3]
        a = band_noise(SIGMA_A, PROP_SEED + 2)
        return a, 2.0 * np.roll(a, 3)
    if case == "am":  # (c)
        return band_noise(SIGMA_A, PROP_SEED + 3), zero
    if case == "pm":  # (d)
        return zero, band_noise(SIGMA_PHI, PROP_SEED + 4)
    if case in ("const", "detuned"):  # (e), (f)
        return zero, zero
    raise KeyError(case)


def prop_input(pkg, case):
    """("iq", (i, q)) f32 of a complex carrier z = A (1 + a) exp(i phi), A = A0 exp(i THETA) (A0 real for "am": Q is exactly 0
    then); ("real", x) f32 of the real carrier 2 Re(z exp(2 pi i f0 j)) at the tuning word of PROP_F0 for "indep_real"."""
    a, phi = prop_modulation(case)
    theta = 0.0 if case == "am" else THETA
    if case == "detuned":
        phi = 2.0 * np.pi * ((DETUNE * np.arange(PROP_LEN)) % 1.0)
    z = A0 * (1.0 + a) * np.exp(1j * (phi + theta))
    if case == "indep_real":
        ftw = pkg.zoom_ftw(PROP_F0)[0]
        w = 2.0 * np.pi * (phases(PROP_LEN, ftw).astype(np.float64) / 18446744073709551616.0)
        return "real", (2.0 * (z * np.exp(1j * w)).real).astype(np.float32)
    return "iq", (z.real.astype(np.float32), z.imag.astype(np.float32))


_PROP = {}


def prop_restatement(pkg, ora, case):
    """stage 0 of the f64 restatement of a property input"""
    if case not in _PROP:
        kind, v = prop_input(pkg, case)
        if kind == "real":
            _PROP[case] = restate_zoom_ampm(ora, v, PROP_N, pkg.zoom_ftw(PROP_F0)[0], max_stages=1)[0]
        else:
            _PROP[case] = restate_zoom_ampm(ora, v[0], PROP_N, 0, iq=mix_c_f64(v[0], v[1], 0), max_stages=1)[0]
    return _PROP[case]


def check_indep(pkg, count, upper, lower, comp, what):
    """(a): S_am and S_pm within 8 / sqrt(count) of 2 sigma^2 at every in-band bin"""
    s_am, s_pm, _, car = stage_am_pm(pkg, PROP_N, count, upper, lower, comp)
    ra, rp = s_am[PROP_BINS] / (2 * SIGMA_A ** 2), s_pm[PROP_BINS] / (2 * SIGMA_PHI ** 2)
    da, dp = float(np.max(np.abs(ra - 1))), float(np.max(np.abs(rp - 1)))
    print(f"{what}: count {count}, median S_am / 2 sigma_a^2 {np.median(ra):.4f} worst {da * np.sqrt(count):.2f} / sqrt(count); "
          f"median S_pm / 2 sigma_phi^2 {np.median(rp):.4f} worst {dp * np.sqrt(count):.2f} / sqrt(count); lock {car[2]:.9f}")
    assert count >= 8000
    assert da < 8.0 / np.sqrt(count) and dp < 8.0 / np.sqrt(count), (what, da, dp)


def check_delay(pkg, count, upper, lower, comp, what):
    """(b): phi[n] = 2 a[n - 3]: s_ampm / s_am within 5e-3 of 2 exp(-2 pi i 3 k / N): the sign convention S_a,phi = conj(a_k) phi_k"""
    s_am, _, s_x, _ = stage_am_pm(pkg, PROP_N, count, upper, lower, comp)
    k = np.arange(PROP_N // 2 + 1)[PROP_BINS]
    d = float(np.max(np.abs(s_x[PROP_BINS] / s_am[PROP_BINS] - 2.0 * np.exp(-2j * np.pi * 3 * k / PROP_N))))
    print(f"{what}: worst |s_ampm / s_am - 2 exp(-2 pi i 3 k / N)| {d:.3g}")
    assert d < 5e-3, (what, d)


def check_am_only(pkg, count, upper, lower, comp, what):
    """(c): S_pm <= 1e-9 S_am"""
    s_am, s_pm, _, _ = stage_am_pm(pkg, PROP_N, count, upper, lower, comp)
    r = float(np.max(np.abs(s_pm[PROP_BINS]) / s_am[PROP_BINS]))
    print(f"{what}: AM only, worst |S_pm| / S_am {r:.3g}")
    assert r <= 1e-9, (what, r)


def check_pm_only(pkg, count, upper, lower, comp, what):
    """(d): S_am <= 1e-5 S_pm (what is left is the second-order term -phi^2 / 2, which IS amplitude)"""
    s_am, s_pm, _, _ = stage_am_pm(pkg, PROP_N, count, upper, lower, comp)
    r = float(np.max(np.abs(s_am[PROP_BINS]) / s_pm[PROP_BINS]))
    print(f"{what}: PM only, worst |S_am| / S_pm {r:.3g}")
    assert r <= 1e-5, (what, r)


def const_truth(pkg):
    """(|A|^2, angle of A) of the constant input as the f32 samples hold it"""
    _, (i, q) = prop_input(pkg, "const")
    a = complex(float(i[0]), float(q[0]))
    return abs(a) ** 2, float(np.angle(a))


def check_const(pkg, count, upper, lower, comp, what, tol_power, tol_theta, tol_lock):
    """(e): a constant z = A0 exp(i THETA): |A|^2, the angle (u = A^2 / |A|^2: half its angle) and lock"""
    power, u, lock = pkg.carrier_from_rows(PROP_N, pkg.WindowTable.hann(PROP_N).power, count, upper[0], lower[0], comp[0])
    p0, th0 = const_truth(pkg)
    dth = abs(0.5 * float(np.angle(u * np.exp(-2j * th0))))
    print(f"{what}: |A|^2 relative error {abs(power / p0 - 1):.3g}, angle error {dth:.3g} rad, 1 - lock {1 - lock:.3g}")
    assert abs(power / p0 - 1) <= tol_power and dth <= tol_theta and abs(1 - lock) <= tol_lock, what
    return power, u, lock


# ---- the kernel's per-bin arithmetic on the host ----

_EMUL = {}


def zoom_ampm_emul_exe(tmp_dir, sanitize):
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "zoom_ampm_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "zoom_ampm_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def zoom_ampm_emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("zoom_ampm_emul")


def run_zoom_ampm_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    got = re.findall(r"zoom_ampm N=(\d+) worst ([0-9.e+-]+) bound ([0-9.e+-]+) \((power|comp)\)", r.stdout)
    assert sorted((int(n), row) for n, _, _, row in got) == [(64, "comp"), (64, "power"), (1024, "comp"), (1024, "power")]
    for n, worst, bound, row in got:
        # rows 0 and 1 within 2e-6 nx^2 (cross_emul's bound), rows 2 and 3 within 4e-6 nx^2
        assert float(bound) == (2e-6 if row == "power" else 4e-6) and float(worst) <= float(bound), (n, row, worst, bound)
    assert "WRONG" not in r.stdout and "FAIL" not in r.stdout
    # amplitude 1 at three scales, the EWMA amplitudes down to 2^-50, an inactive team
    for text in ("amp=1 ", "scale=0.001", "scale=1000", "amp=0.707 ", "amp=8.88e-16", "active=0"):
        assert text in r.stdout, text


def test_zoom_ampm_bin_emulation(zoom_ampm_emul_dir):
    """csrc/zoom_ampm_fft.h for every lane against an f64 DFT at N = 64 and 1024: the four products of the bins the team transform
    leaves in its frame, every (row, bin) written once, the complementary row from FFT indices k and (N - k) mod N
    (tests/host/zoom_ampm_emul.cpp; the program asserts, the figures it prints are checked again here)"""
    run_zoom_ampm_emul(zoom_ampm_emul_exe(zoom_ampm_emul_dir, sanitize=False))


def test_zoom_ampm_bin_emulation_under_sanitizers(zoom_ampm_emul_dir):
    """the same program built with -fsanitize=address,undefined: the team's frame and the partial rows have their exact sizes"""
    run_zoom_ampm_emul(zoom_ampm_emul_exe(zoom_ampm_emul_dir, sanitize=True))


# ---- exports, arguments ----

def test_zoom_ampm_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    L = pkg.lib()
    for prefix, symbols in (("psdc_zampm_", ZAMPM_SYMBOLS), ("psdc_iqampm_", IQAMPM_SYMBOLS)):
        declared = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr))
        assert declared == set(symbols)
        assert set(re.findall(r" T (" + prefix + r"[a-z0-9_]+)", out)) == declared
        assert declared <= set(pkg.EXPORTS)
        for name in symbols:  # mirrored in lib(): a prototype, not ctypes' default
            assert getattr(L, name).argtypes is not None, name
    assert L.psdc_abi_version() == 3
    # the f32 sample routes only: no frames, Loss or integer feeds for the new handles, in the header or in the library
    for text in (hdr, out):
        assert not re.search(r"psdc_(zampm|iqampm)_process_frames|psdc_(zampm|iqampm)_loss_read|psdc_s?int_(zampm|iqampm)", text)
    for cls in ("ZoomAmPmCascadeBank", "ZoomAmPmCascade", "IqAmPmCascadeBank", "IqAmPmCascade"):
        for m in ("set_carrier", "process", "process_device", "set_detrend", "set_avg", "num_stages", "stage_rows", "psd", "sidebands",
                  "carrier", "am_pm", "sync", "reset", "stats_read", "close"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)
        for m in ("process_frames", "process_frames_device", "loss", "process_int", "process_int_device", "sk", "stage_moments"):
            assert not hasattr(getattr(pkg, cls), m), (cls, m)
        assert callable(getattr(getattr(pkg, cls), "process_device_planar", None)) == cls.startswith("Iq")
        doc = " ".join((getattr(pkg, cls).__doc__ + pkg.ZoomAmPmCascadeBank.__doc__).split())
        for text in ("small-modulation", "second order", "lock", "bins 0 and 1", "-2 f0"):
            assert text in doc, (cls, text)
    assert callable(pkg.am_pm_from_sidebands) and callable(pkg.zoom_ampm_supported)
    # the definition is written down: rows, the relations, the limits
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "AM/PM cascades" in hdr
    for text in ("comp_re[k] = sum_j w_j Re(Z_j[k] Z_j[(N - k) mod N])", "WITHOUT a conjugate", "upper - lower = -4 |A|^2 Im S_a,phi",
                 "phi^2 reads as AM at second order", "stream frames, the loss record and the integer feeds are not offered yet"):
        assert text in flat, text


def test_zoom_ampm_supported(pkg):
    L = pkg.lib()
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        assert pkg.zoom_ampm_supported(n) and L.psdc_iqampm_supported(n) == 1 and L.psdc_zampm_supported(n) == 1, n
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.zoom_ampm_supported(n) and L.psdc_iqampm_supported(n) == 0, n
    assert not pkg.zoom_ampm_supported(-1) and not pkg.zoom_ampm_supported(1 << 32)


@pytest.mark.parametrize("family", ["zampm", "iqampm"])
def test_zoom_ampm_argument_errors(pkg, family):
    """what is refused before any device is touched: sizes, windows, channel counts, null handles"""
    import ctypes as C
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    f = lambda name: getattr(L, pre + name)  # noqa: E731
    bank = pkg.ZoomAmPmCascadeBank if family == "zampm" else pkg.IqAmPmCascadeBank
    single = pkg.ZoomAmPmCascade if family == "zampm" else pkg.IqAmPmCascade
    for n in (32, 8192, 1000, 0):
        with pytest.raises(pkg.PsdError) as e:
            bank(n, 1)
        assert e.value.code == pkg.ERR_ARG and pre + "create: n must be a power of two in [64, 4096]" in str(e.value)
        with pytest.raises(pkg.PsdError) as e:
            single(n, f0=0.2)
        assert e.value.code == pkg.ERR_ARG
        w = np.ones(max(n, 1), np.float32)
        assert not f("create_window")(n, pkg._fptr(w), 1.0, 1.0, 0, 1, 0)
        assert pre + "create_window: n must be a power of two in [64, 4096]" in f("last_error")(None).decode()
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not f("create_window")(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in f("last_error")(None).decode()
    assert not f("create_window")(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in f("last_error")(None).decode()
    assert not f("create")(256, 7, 1, 0)
    assert "window_kind" in f("last_error")(None).decode()
    for nch in (0, 65537):
        assert not f("create")(256, 1, nch, 0)
        assert "n_channels must be in [1, 65536]" in f("last_error")(None).decode()
    with pytest.raises(pkg.PsdError) as e:
        bank(256, 1, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG
    # a null handle: every call, the carrier's included
    assert f("set_carrier")(None, 0, 1, 2) == pkg.ERR_ARG
    assert pre + "set_carrier: null handle" in f("last_error")(None).decode()
    feeds = ([f("process")(None, 0, None, 4), f("process_device")(None, 0, None, 4, None)] if family == "zampm" else
             [f("process")(None, 0, None, None, 4), f("process_device")(None, 0, None, None, 4, None),
              f("process_interleaved")(None, 0, None, 4), f("process_interleaved_device")(None, 0, None, 4, None)])
    for rc in feeds + [f("sync")(None), f("reset")(None), f("set_detrend")(None, 0), f("set_avg")(None, 1, 1), f("num_stages")(None, 0),
                       f("stage_rows")(None, 0, 0, None, None, None, None, None),
                       f("psd")(None, 0, 0, 1, 0, None, None, 0, None, None, 0, None),
                       f("sidebands")(None, 0, 0, 1, 0, None, None, None, None, 0, None, None, 0, None),
                       f("stats_read")(None, C.byref(C.c_uint64()), None, 0)]:
        assert rc == pkg.ERR_ARG
    f("destroy")(None)
    with pytest.raises(pkg.PsdError) as e:
        pkg.am_pm_from_sidebands(np.ones(3), np.ones(3), np.ones(3, complex), 0.0)
    assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.PsdError) as e:
        pkg.carrier_from_rows(64, 0.25, 0, 1.0, 1.0, 1.0)
    assert e.value.code == pkg.ERR_ARG


@pytest.mark.parametrize("family", ["zampm", "iqampm"])
def test_zoom_ampm_no_gpu_fails_loudly(pkg, family):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    make = (lambda: pkg.ZoomAmPmCascade(1024, f0=0.2)) if family == "zampm" else (lambda: pkg.IqAmPmCascade(1024))
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
    """(1) rows 0 and 1 are restate_zoom's upper / lower bit for bit, at a carrier, in f64 and in the f32 sibling given the same I
    and Q; (2) counts, averages, pendings and the stitched Breaks are equal; (3) comp at k = 0 and N/2 is sum Z_k^2, so with one
    average |comp| there equals both power rows; |comp| <= sqrt(upper lower) everywhere (Cauchy-Schwarz).  A check of the
    yardstick, not of the library."""
    x = noise(length, n)
    pwin, owin = windows_of(pkg, n, window)
    avg = avg or (U32_MAX, U32_MAX)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    for prec, iq in (("f64", None), ("f32", mix_f32(emul, x, ftw))):
        st = restate_zoom_ampm(ora, x, n, ftw, 0, owin, detrend, avg, prec, iq=iq)
        rz = restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg, prec, iq=iq)
        assert len(st) == len(rz)
        for k, (s, r) in enumerate(zip(st, rz)):
            assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
            for row in ("upper", "lower"):
                assert s[row].dtype == r[row].dtype and s[row].tobytes() == r[row].tobytes(), (prec, k, row)
            assert s["comp"].dtype == (np.complex128 if prec == "f64" else np.complex64)
            assert np.all(np.abs(s["comp"]) <= np.sqrt(s["upper"].astype(np.float64) * s["lower"]) * (1 + 1e-5) + 1e-30), k
            if s["count"] == 1:
                for b in (0, n // 2):
                    assert abs(abs(s["comp"][b]) - s["upper"][b]) <= 1e-5 * s["upper"][b] + 1e-30, (k, b)
        assert stitch_zoom(pkg, n, pwin, st)[2] == stitch_zoom(pkg, n, pwin, rz)[2]
    one = restate_zoom_ampm(ora, x, n, ftw, 0, owin, detrend, avg, max_stages=1)
    assert one[0]["comp"].tobytes() == restate_zoom_ampm(ora, x, n, ftw, 0, owin, detrend, avg)[0]["comp"].tobytes()


# ---- what am_pm() and carrier() read on the f64 restatement ----

def rows_of(s):
    return s["count"], s["upper"], s["lower"], s["comp"]


@pytest.mark.parametrize("case", ["indep", "indep_real"])
def test_restatement_independent_modulations(pkg, ora, case):
    """(a): sigma_a = 1e-3, sigma_phi = 3e-3 on a complex carrier and on a real one at f0 = 0.2"""
    check_indep(pkg, *rows_of(prop_restatement(pkg, ora, case)), case)


def test_restatement_delayed_pm_fixes_the_sign(pkg, ora):
    check_delay(pkg, *rows_of(prop_restatement(pkg, ora, "delay")), "delay")


def test_restatement_am_only(pkg, ora):
    check_am_only(pkg, *rows_of(prop_restatement(pkg, ora, "am")), "am")


def test_restatement_pm_only(pkg, ora):
    check_pm_only(pkg, *rows_of(prop_restatement(pkg, ora, "pm")), "pm")


def test_restatement_constant_carrier(pkg, ora):
    """(e): |A|^2 within 1e-12 relative, the angle within 1e-12 rad, lock within 1e-12 of 1"""
    check_const(pkg, *rows_of(prop_restatement(pkg, ora, "const")), "const", 1e-12, 1e-12, 1e-12)


def test_restatement_detuned_carrier_loses_lock(pkg, ora):
    """(f): a carrier detuned by 1e-5 fs turns 21 times during the average: lock < 0.01"""
    count, up, lo, comp = rows_of(prop_restatement(pkg, ora, "detuned"))
    lock = pkg.carrier_from_rows(PROP_N, pkg.WindowTable.hann(PROP_N).power, count, up[0], lo[0], comp[0])[2]
    print(f"detuned by {DETUNE} fs: lock {lock:.3g}")
    assert lock < 0.01


def test_am_pm_from_sidebands_is_pure(pkg):
    """the relations written out on made-up rows: a carrier phase turns comp and nothing else; the sign of A does not matter"""
    rng = np.random.default_rng(5)
    s_a, s_p = rng.uniform(1, 2, 9), rng.uniform(1, 2, 9)
    s_x = 0.3 * (rng.standard_normal(9) + 1j * rng.standard_normal(9))
    for A in (1.0, 0.5 * np.exp(0.9j), -2.0j):
        P, u = abs(A) ** 2, A * A / abs(A) ** 2
        mean, dif = P * (s_a + s_p), -4 * P * s_x.imag  # (U + L) / 2, U - L
        U, L = mean + dif / 2, mean - dif / 2
        comp = P * (s_a - s_p + 2j * s_x.real) * u
        for carrier in (A, -A):
            a, p, x = pkg.am_pm_from_sidebands(U, L, comp, carrier)
            assert a.dtype == p.dtype == np.float64 and x.dtype == np.complex128
            assert np.allclose(a, s_a, rtol=1e-13) and np.allclose(p, s_p, rtol=1e-13) and np.allclose(x, s_x, rtol=1e-12)
