"""Zoom and IQ spectral kurtosis cascades (psdc_zsk_*, psdc_iqsk_*): the parts that run without a GPU.  Semantics:
include/psdcascade.h, "zoom and IQ spectral kurtosis cascades".

restate_zoom_sk below is the yardstick of tests/test_gpu_zoom_sk.py: restate_zoom of tests/test_zoom_host.py with the S2 rows
sum w |Z|^4 kept beside the S1 rows.  It is anchored three ways: its S1 rows are restate_zoom's rows bit for bit (f64, and the f32
sibling given the same I and Q), with ftw = 0 on a real stream both S2 rows are restate_sk's S2 (tests/test_sk_host.py), and counts
and pendings are equal.  The statistical properties the GPU tests assert (circular Gaussian noise reads 1 at EVERY bin, a real
stream mixed from f0 rises towards 2 where its own DC and Nyquist fall, a complex tone reads 0 on its side only) are checked on the
f64 restatement first, so that the reference itself is inside the bounds the GPU is held to.

The per-slot arithmetic and the row map of the kernel (csrc/zoom_sk_fft.h) run on the host in tests/host/zoom_sk_emul.cpp, which
this file compiles itself: once plainly and once under the address and undefined-behaviour sanitizers (a stand-alone program;
nothing is loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, U32_MAX, _window
from test_iq_host import mix_c_f64
from test_sk_host import gaussian, restate_sk
from test_zoom_host import emul, mix_f32, mix_f64, noise, restate_zoom, windows_of  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = ["supported", "create", "create_window", "destroy", "reset", "set_detrend", "set_avg", "set_carrier", "sync", "num_stages",
           "stage_moments", "psd", "sk", "stats_read", "last_error"]
ZSK_SYMBOLS = ["psdc_zsk_" + s for s in _COMMON + ["process", "process_device"]]
IQSK_SYMBOLS = ["psdc_iqsk_" + s for s in _COMMON + ["process", "process_device", "process_interleaved", "process_interleaved_device"]]


def restate_zoom_sk(ora, x, n, ftw, phase0=0, window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64", iq=None,
                    max_stages=None, schedule=None):
    """Zoom spectral kurtosis cascade of the stream x: per stage dict(count, avg, pending, upper, lower, s2_upper, s2_lower), stage 0
    first; upper / lower are the S1 rows, computed as restate_zoom computes them.  prec, iq and schedule as restate_zoom takes them.
    max_stages: stop after that many stages (the property tests look at the first ones only)."""
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
        upper, lower = np.zeros(h, ft), np.zeros(h, ft)
        u2, l2 = np.zeros(h, ft), np.zeros(h, ft)
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
            p2 = (p * p).astype(ft)
            g = 1.0
            if count > a:
                g = float(np.float32(a) / np.float32(count))  # src/psd.rs:220: defined in f32
                count = a
            count += 1
            upper = ft(g) * upper + p[:h]
            lower = ft(g) * lower + p[lower_idx]
            u2 = ft(g) * u2 + p2[:h]
            l2 = ft(g) * l2 + p2[lower_idx]
        pending = si.size if nseg == 0 else si.size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, upper=upper, lower=lower, s2_upper=u2, s2_lower=l2))
        p = nseg * hop + overlap if nseg else 0
        si = ora.hbf_dec8(si[:p], prec)[DRAIN:].astype(ft)
        sq = ora.hbf_dec8(sq[:p], prec)[DRAIN:].astype(ft)
        k += 1
    return stages


def sk_rows(pkg, s):
    """(sk_upper, sk_lower) of one restated stage"""
    return (pkg.sk_from_moments(s["count"], s["upper"], s["s2_upper"]), pkg.sk_from_moments(s["count"], s["lower"], s["s2_lower"]))


# ---- the inputs of the statistical properties, shared with tests/test_gpu_zoom_sk.py (each restatement is computed once a session) ----

PROP_N = 512
PROP_SEED = 20261019  # fixed; if a restatement missed a bound below, the seed or the input would change, never the bound
PROP_F0 = 0.2
TONE_BIN = 37


def prop_input(case):
    """(i, q) f32 of "circular" and "tone" (complex streams, ftw = 0); x f32 of "real" (mixed from PROP_F0)"""
    n = PROP_N
    if case == "circular":  # (a): I and Q independent
        return gaussian(1 << 21, PROP_SEED), gaussian(1 << 21, PROP_SEED + 1)
    if case == "real":  # (b)
        return gaussian(1 << 21, PROP_SEED + 2)
    if case == "tone":  # (c): exp(2 pi i (37.37 / N) j) + 1e-3 (circular Gaussian)
        m = 1 << 19
        a = 2 * np.pi * (((TONE_BIN + 0.37) / n) * np.arange(m, dtype=np.float64) % 1.0)
        return ((np.cos(a) + 1e-3 * gaussian(m, PROP_SEED + 3)).astype(np.float32),
                (np.sin(a) + 1e-3 * gaussian(m, PROP_SEED + 4)).astype(np.float32))
    raise KeyError(case)


_PROP = {}


def prop_restatement(pkg, ora, case):
    if case not in _PROP:
        v = prop_input(case)
        if case == "real":
            _PROP[case] = restate_zoom_sk(ora, v, PROP_N, pkg.zoom_ftw(PROP_F0)[0], max_stages=1)
        else:
            _PROP[case] = restate_zoom_sk(ora, v[0], PROP_N, 0, iq=mix_c_f64(v[0], v[1], 0), max_stages=None if case == "circular" else 1)
    return _PROP[case]


def check_circular(sk_of_stage, counts):
    """(a): every stage with count >= 255, both rows, ALL bins 0 ... N/2 within 16 / sqrt(count) of 1 (every bin of a complex stream
    is complex: offset 0 and Nyquist read 1 too), median within 0.05 of 1; at least two such stages"""
    seen = 0
    for k, count in enumerate(counts):
        if count < 255:
            continue
        seen += 1
        for name, sk in zip(("upper", "lower"), sk_of_stage(k)):
            dev = float(np.max(np.abs(sk - 1.0)))
            print(f"circular stage {k} count {count} {name}: worst |SK - 1| {dev:.4f} = {dev * np.sqrt(count):.2f} / sqrt(count), "
                  f"median {np.median(sk):.4f}, bin 0 {sk[0]:.3f}, bin N/2 {sk[-1]:.3f}")
            assert sk.size == PROP_N // 2 + 1
            assert dev < 16.0 / np.sqrt(count), (k, name, count, dev)
            assert abs(float(np.median(sk)) - 1.0) < 0.05, (k, name, np.median(sk))
    assert seen >= 2
    return seen


REAL_UPPER, REAL_LOWER = (153, 154), (102, 103)  # where the stream's own Nyquist (0.5 - f0) and DC (f0) fall at f0 = 0.2, N = 512


def check_real(sk_up, sk_lo, count):
    """(b): upper bins 153 and 154 and lower bins 102 and 103 each above 1.2; every bin of a row further than 3 bins from that
    row's two within 16 / sqrt(count) of 1"""
    print(f"real stream from f0 = {PROP_F0}, count {count}: upper 153, 154: {sk_up[153]:.3f}, {sk_up[154]:.3f}; "
          f"lower 102, 103: {sk_lo[102]:.3f}, {sk_lo[103]:.3f}")
    k = np.arange(PROP_N // 2 + 1)
    for name, sk, marked in (("upper", sk_up, REAL_UPPER), ("lower", sk_lo, REAL_LOWER)):
        for b in marked:
            assert sk[b] > 1.2, (name, b, sk[b])
        far = np.min(np.abs(k[:, None] - np.array(marked)[None, :]), axis=1) > 3
        dev = float(np.max(np.abs(sk[far] - 1.0)))
        print(f"  {name}: worst |SK - 1| of the other bins {dev:.4f} = {dev * np.sqrt(count):.2f} / sqrt(count)")
        assert dev < 16.0 / np.sqrt(count), (name, dev)


def check_tone(sk_up, sk_lo):
    """(c): the tone is at +37.37 / N: upper bin 37 reads 0, lower bin 37 holds noise (the row orientation)"""
    med = float(np.median(sk_lo[20:61]))
    print(f"tone: upper bin {TONE_BIN} {sk_up[TONE_BIN]:.3g}, lower bin {TONE_BIN} {sk_lo[TONE_BIN]:.3f}, median of lower 20 ... 60 {med:.4f}")
    assert sk_up[TONE_BIN] < 1e-3
    assert sk_lo[TONE_BIN] > 0.5
    assert abs(med - 1.0) < 0.1


# ---- the kernel's per-slot arithmetic and row map on the host ----

_EMUL = {}


def zoom_sk_emul_exe(tmp_dir, sanitize):
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "zoom_sk_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "zoom_sk_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def zoom_sk_emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("zoom_sk_emul")


def run_zoom_sk_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    got = re.findall(r"zoom_sk N=(\d+) worst ([0-9.e+-]+) bound ([0-9.e+-]+) \((P2?)\)", r.stdout)
    assert sorted((int(n), row) for n, _, _, row in got) == [(64, "P"), (64, "P2"), (1024, "P"), (1024, "P2")]
    for n, worst, bound, row in got:
        # the bounds tests/host/sk_emul.cpp holds: P within 2e-6 of w nx^2, P^2 within 4e-6 of w nx^4
        assert float(bound) == (2e-6 if row == "P" else 4e-6) and float(worst) <= float(bound), (n, row, worst, bound)
    assert "WRONG" not in r.stdout and "FAIL" not in r.stdout
    # weight 1 at three scales, the EWMA weights down to 2^-100, an inactive team
    for text in ("w=1 ", "scale=0.001", "scale=1000", "w=0.5 ", "w=7.89e-31", "active=0"):
        assert text in r.stdout, text


def test_zoom_sk_slot_emulation(zoom_sk_emul_dir):
    """csrc/zoom_sk_fft.h for every lane against an f64 DFT at N = 64 and 1024: P and P^2 of the bins the team transform yields,
    the weights, and every (row, bin) of the four rows written once from the right FFT index (tests/host/zoom_sk_emul.cpp; the
    program asserts, the figures it prints are checked again here)"""
    run_zoom_sk_emul(zoom_sk_emul_exe(zoom_sk_emul_dir, sanitize=False))


def test_zoom_sk_slot_emulation_under_sanitizers(zoom_sk_emul_dir):
    """the same program built with -fsanitize=address,undefined: the team's LDS region and the partial rows have their exact sizes"""
    run_zoom_sk_emul(zoom_sk_emul_exe(zoom_sk_emul_dir, sanitize=True))


# ---- exports, arguments ----

def test_zoom_sk_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    L = pkg.lib()
    for prefix, symbols in (("psdc_zsk_", ZSK_SYMBOLS), ("psdc_iqsk_", IQSK_SYMBOLS)):
        declared = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr))
        assert declared == set(symbols)
        assert set(re.findall(r" T (" + prefix + r"[a-z0-9_]+)", out)) == declared
        assert declared <= set(pkg.EXPORTS)
        for name in symbols:  # mirrored in lib(): a prototype, not ctypes' default
            assert getattr(L, name).argtypes is not None, name
    assert L.psdc_abi_version() == 3
    # the f32 sample routes only: no frames, Loss or integer feeds for the new handles, in the header or in the library
    for text in (hdr, out):
        assert not re.search(r"psdc_(zsk|iqsk)_process_frames|psdc_(zsk|iqsk)_loss_read|psdc_s?int_(zsk|iqsk)", text)
        assert not re.search(r"psdc_(zoomsk|iqsk)cascade_", text)
    for cls in ("ZoomSkCascadeBank", "ZoomSkCascade", "IqSkCascadeBank", "IqSkCascade"):
        for m in ("set_carrier", "process", "process_device", "set_detrend", "set_avg", "num_stages", "stage_moments", "psd", "sk",
                  "sync", "reset", "stats_read", "close"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)
        for m in ("process_frames", "process_frames_device", "loss", "process_int", "process_int_device"):
            assert not hasattr(getattr(pkg, cls), m), (cls, m)
        assert callable(getattr(getattr(pkg, cls), "process_device_planar", None)) == cls.startswith("Iq")
    # the definition is written down: rows, estimator, what SK reads on complex bins
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "zoom and IQ spectral kurtosis cascades" in hdr
    for text in ("s2_upper[k] = sum_j w_j |Z_j[k]|^4", "s2_lower[k] = sum_j w_j |Z_j[(N - k) mod N]|^4",
                 "reads 1 at every bin, offset 0 and Nyquist included", "SK rises towards 2", "never divided by"):
        assert text in flat, text


def test_zoom_sk_supported(pkg):
    L = pkg.lib()
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        assert pkg.zoom_sk_supported(n) and L.psdc_iqsk_supported(n) == 1 and pkg.sk_supported(n), n
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.zoom_sk_supported(n) and L.psdc_iqsk_supported(n) == 0, n
    assert not pkg.zoom_sk_supported(-1) and not pkg.zoom_sk_supported(1 << 32)


@pytest.mark.parametrize("family", ["zsk", "iqsk"])
def test_zoom_sk_argument_errors(pkg, family):
    """what is refused before any device is touched: sizes, windows, channel counts, null handles"""
    import ctypes as C
    L = pkg.lib()
    pre = "psdc_" + family + "_"
    f = lambda name: getattr(L, pre + name)  # noqa: E731
    bank = pkg.ZoomSkCascadeBank if family == "zsk" else pkg.IqSkCascadeBank
    single = pkg.ZoomSkCascade if family == "zsk" else pkg.IqSkCascade
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
    feeds = ([f("process")(None, 0, None, 4), f("process_device")(None, 0, None, 4, None)] if family == "zsk" else
             [f("process")(None, 0, None, None, 4), f("process_device")(None, 0, None, None, 4, None),
              f("process_interleaved")(None, 0, None, 4), f("process_interleaved_device")(None, 0, None, 4, None)])
    for rc in feeds + [f("sync")(None), f("reset")(None), f("set_detrend")(None, 0), f("set_avg")(None, 1, 1), f("num_stages")(None, 0),
                       f("stage_moments")(None, 0, 0, None, None, None, None, None),
                       f("psd")(None, 0, 0, 1, 0, None, None, 0, None, None, 0, None),
                       f("sk")(None, 0, 0, 1, 0, None, None, 0, None, None, 0, None),
                       f("stats_read")(None, C.byref(C.c_uint64()), None, 0)]:
        assert rc == pkg.ERR_ARG
    f("destroy")(None)


@pytest.mark.parametrize("family", ["zsk", "iqsk"])
def test_zoom_sk_no_gpu_fails_loudly(pkg, family):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    make = (lambda: pkg.ZoomSkCascade(1024, f0=0.2)) if family == "zsk" else (lambda: pkg.IqSkCascade(1024))
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
    """(1) the S1 rows are restate_zoom's upper / lower bit for bit, at a carrier, in f64 and in the f32 sibling given the same I and
    Q; (2) with ftw = 0 on a real stream both S2 rows are restate_sk's s2 to 1e-9 relative (under a detrend plus 1e-9 of the row's
    mean: the bins a detrend nulls); (3) counts, averages and pendings are equal in both.  The four cases of
    test_restatement_ftw0_is_the_oracle_cascade (tests/test_zoom_host.py).  A check of the yardstick, not of the library."""
    x = noise(length, n)
    _, owin = windows_of(pkg, n, window)
    avg = avg or (U32_MAX, U32_MAX)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    for prec, iq in (("f64", None), ("f32", mix_f32(emul, x, ftw))):
        st = restate_zoom_sk(ora, x, n, ftw, 0, owin, detrend, avg, prec, iq=iq)
        rz = restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg, prec, iq=iq)
        assert len(st) == len(rz)
        for k, (s, r) in enumerate(zip(st, rz)):
            assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
            for row in ("upper", "lower"):
                assert s[row].dtype == r[row].dtype and s[row].tobytes() == r[row].tobytes(), (prec, k, row)
                assert s["s2_" + row].dtype == s[row].dtype
            if s["count"] == 1:
                assert np.array_equal(s["s2_upper"], s["upper"] * s["upper"]) and np.array_equal(s["s2_lower"], s["lower"] * s["lower"]), k
    st = restate_zoom_sk(ora, x, n, 0, 0, owin, detrend, avg)
    rs = restate_sk(ora, x, n, owin, detrend, avg, "f64")
    assert len(st) == len(rs)
    worst = 0.0
    for k, (s, r) in enumerate(zip(st, rs)):
        assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
        floor = 1e-9 * np.mean(r["s2"]) if detrend != "none" else 0.0
        for row in ("s2_upper", "s2_lower"):
            assert np.all(np.abs(s[row] - r["s2"]) <= 1e-9 * r["s2"] + floor), (row, k)
            if s["count"]:
                worst = max(worst, float(np.max(np.abs(s[row] - r["s2"]) / np.maximum(r["s2"], floor + 1e-300))))
    print(f"ftw = 0: S2 rows against restate_sk, worst relative difference {worst:.3g}")
    assert restate_zoom_sk(ora, x, n, 0, 0, owin, detrend, avg, max_stages=1)[0]["s2_upper"].tobytes() == st[0]["s2_upper"].tobytes()


# ---- statistical properties of the f64 restatement ----

def test_restatement_circular_noise_reads_one_at_every_bin(pkg, ora):
    st = prop_restatement(pkg, ora, "circular")
    check_circular(lambda k: sk_rows(pkg, st[k]), [s["count"] for s in st])


def test_restatement_real_stream_rises_at_its_dc_and_nyquist(pkg, ora):
    s = prop_restatement(pkg, ora, "real")[0]
    check_real(*sk_rows(pkg, s), s["count"])


def test_restatement_complex_tone_reads_zero_on_its_side(pkg, ora):
    s = prop_restatement(pkg, ora, "tone")[0]
    check_tone(*sk_rows(pkg, s))
