"""Spectral kurtosis cascade (psdc_sk_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "spectral kurtosis
cascade".

restate_sk below is the yardstick of tests/test_gpu_sk.py: the restatement of tests/test_cross_host.py on one stream, with
S2 = sum w P^2 kept beside S1 = sum w P.  It is anchored here: its S1 is restate(...)["sxx"] bit for bit and the oracle's f64
PsdCascade to 1e-12.  The statistical properties the GPU tests assert (Gaussian noise reads 1, a line reads 0, gated noise reads
above 2) are checked on the f64 restatement first, so that the reference itself is inside the bounds the GPU is held to.

The per-bin arithmetic of the kernel (csrc/sk_fft.h) runs on the host in tests/host/sk_emul.cpp, which this file compiles itself:
once plainly and once under the address and undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, U32_MAX, _window, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SK_SYMBOLS = ["psdc_sk_supported", "psdc_sk_create", "psdc_sk_create_window", "psdc_sk_destroy", "psdc_sk_reset",
              "psdc_sk_set_detrend", "psdc_sk_set_avg", "psdc_sk_process", "psdc_sk_process_device", "psdc_sk_sync",
              "psdc_sk_num_stages", "psdc_sk_stage_moments", "psdc_sk_psd", "psdc_sk_sk", "psdc_sk_stats_read",
              "psdc_sk_last_error"]


def restate_sk(ora, x, n, window="hann", detrend="none", avg=(U32_MAX, U32_MAX), prec="f64", max_stages=None, schedule=None):
    """Spectral kurtosis cascade of the stream x: per stage dict(count, avg, pending, s1, s2), stage 0 first.
    prec "f64": truth; "f32": the reference's arithmetic (f32 detrend / FFT / decimator, f32 accumulation).
    max_stages: stop after that many stages (the property tests look at the first ones only).
    schedule: a settings_schedule.Schedule of mid-stream set_detrend / set_avg calls; it then replaces detrend and avg."""
    win, _, _, overlap, kind = _window(ora, n, window)
    hop = n - overlap
    h = n // 2 + 1
    ft = np.float64 if prec == "f64" else np.float32
    ct = np.complex128 if prec == "f64" else np.complex64
    xs = np.asarray(x, np.float32)
    stages = []
    k = 0
    while xs.size and (max_stages is None or k < max_stages):
        nseg = 0 if xs.size < n else 1 + (xs.size - n) // hop
        sh = 3 * k
        a = min((avg[1] >> sh) if sh < 32 else 0, avg[0])
        s1, s2 = np.zeros(h, ft), np.zeros(h, ft)
        count = 0

        def spec(seg):
            if kind is not None:
                c = ora.detrend_apply(seg, detrend, kind, prec)
            else:
                c = ora.detrend_apply(seg, detrend, "rect", prec) * win.astype(ft)
            return ora.fft_forward(c.astype(ct), prec)[:h].astype(ct)

        for j in range(nseg):
            if schedule is not None:  # the settings in force when segment j of stage k completed
                detrend, a = schedule.stage(k, j)
            X = spec(xs[j * hop:j * hop + n])
            g = 1.0
            if count > a:
                g = float(np.float32(a) / np.float32(count))  # src/psd.rs:220: defined in f32
                count = a
            count += 1
            p = (X.real * X.real + X.imag * X.imag).astype(ft)
            s1 = ft(g) * s1 + p
            s2 = ft(g) * s2 + (p * p).astype(ft)
        pending = xs.size if nseg == 0 else xs.size - nseg * hop
        if schedule is not None:
            a = schedule.final_avg(k)  # the stitchers take the value in force at the end
        stages.append(dict(count=count, avg=a, pending=pending, s1=s1, s2=s2))
        p = nseg * hop + overlap if nseg else 0
        xs = ora.hbf_dec8(xs[:p], prec)[DRAIN:].astype(ft)  # (the f64 oracle carries its stages in f64)
        k += 1
    return stages


# ---- the inputs of the statistical properties, shared with tests/test_gpu_sk.py (each restatement is computed once a session) ----

PROP_N = 512
PROP_SEED = 20261018  # fixed; if its restatement missed a bound below, the seed would change, never the bound


def gaussian(length, seed=PROP_SEED):
    """Gaussian noise.  (pkg.noise_host is uniform: at N = 64 uniform noise reads a mean SK of 0.96, so it is no Gaussian test
    signal at small N.)"""
    return np.random.default_rng(seed).standard_normal(length).astype(np.float32)


def prop_input(case):
    n = PROP_N
    if case == "gauss":
        return gaussian(1 << 21)
    if case == "tone":  # a line at bin 100.37 of stage 0, 60 dB above the noise floor's amplitude
        m = 1 << 19
        return (np.cos(2 * np.pi * ((100.37 / n) * np.arange(m, dtype=np.float64) % 1.0)) + 1e-3 * gaussian(m)).astype(np.float32)
    if case == "gated":  # on for 8 N samples, off for 8 N
        m = 1 << 19
        gate = ((np.arange(m) // (8 * n)) % 2 == 0).astype(np.float32)
        return (gaussian(m) * gate).astype(np.float32)
    raise KeyError(case)


_PROP = {}


def prop_restatement(ora, case):
    if case not in _PROP:
        _PROP[case] = restate_sk(ora, prop_input(case), PROP_N, max_stages=None if case == "gauss" else 1)
    return _PROP[case]


def check_gauss(sk_of_stage, counts):
    """(a): every stage with count >= 255: bins 2 ... N/2 - 2 within 16 / sqrt(count) of 1 (8 sigma of sk_sigma; a numpy model of
    the estimator over 32 draws at counts 255 ... 16383 read 9.2 / sqrt(count) at its worst bin), median within 0.05 of 1"""
    n = PROP_N
    seen = 0
    for k, count in enumerate(counts):
        if count < 255:
            continue
        seen += 1
        sk = sk_of_stage(k)[2:n // 2 - 1]
        dev = float(np.max(np.abs(sk - 1.0)))
        print(f"gauss stage {k} count {count}: worst |SK - 1| {dev:.4f} = {dev * np.sqrt(count):.2f} / sqrt(count), "
              f"median {np.median(sk):.4f}")
        assert dev < 16.0 / np.sqrt(count), (k, count, dev)
        assert abs(float(np.median(sk)) - 1.0) < 0.05, (k, np.median(sk))
    assert seen >= 2
    return seen


def check_tone(sk0):
    print(f"tone: SK at bin 100 {sk0[100]:.3g}, median of bins 150 ... 250 {np.median(sk0[150:251]):.4f}")
    assert sk0[100] < 1e-3
    assert abs(float(np.median(sk0[150:251])) - 1.0) < 0.1


def check_gated(sk0):
    med = float(np.median(sk0[2:PROP_N // 2 - 1]))
    print(f"gated: median SK of stage-0 bins 2 ... N/2 - 2 {med:.4f}")
    assert med > 2.0
    return med


# ---- exports, arguments ----

def test_sk_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_sk_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SK_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_sk_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert pkg.lib().psdc_abi_version() == 3
    # the definition is written down: rows, estimator, its limits
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "spectral kurtosis cascade" in hdr
    assert "SK[k] = (M + 1) / (M - 1) * (M S2[k] / S1[k]^2 - 1)" in hdr
    for text in ("about 2 count - 1", "read 2 for Gaussian noise", "must stay below f32 max", "never divided by"):
        assert text in flat, text
    for cls in ("SkCascadeBank", "SkCascade"):
        for m in ("process", "process_device", "set_detrend", "set_avg", "num_stages", "stage_moments", "psd", "sk", "sync", "reset",
                  "stats"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)


def test_sk_supported(pkg):
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        assert pkg.sk_supported(n), n
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.sk_supported(n), n


def test_sk_from_moments(pkg):
    """the pure formula: constant P reads 0, exponentially distributed P reads 1, P on one segment in four reads about 7 (2 / d - 1);
    NaN below two averages and without power"""
    m = 1000
    ones = np.ones(5)
    assert np.all(pkg.sk_from_moments(m, m * ones, m * ones) == 0.0)
    rng = np.random.default_rng(1)
    p = rng.exponential(3.0, (m, 4000))
    sk = pkg.sk_from_moments(m, p.sum(0), (p * p).sum(0))
    assert sk.dtype == np.float64 and abs(sk.mean() - 1.0) < 0.01 and abs(sk.std() - pkg.sk_sigma(m)) < 0.1 * pkg.sk_sigma(m)
    p[np.arange(m) % 4 != 0] = 0.0
    assert abs(np.median(pkg.sk_from_moments(m, p.sum(0), (p * p).sum(0))) - 7.0) < 0.5  # 2 / d - 1 with d = 1/4
    assert np.all(np.isnan(pkg.sk_from_moments(1, ones, ones))) and np.all(np.isnan(pkg.sk_from_moments(0, ones, ones)))
    got = pkg.sk_from_moments(10, np.array([0.0, 1.0]), np.array([0.0, 1.0]))
    assert np.isnan(got[0]) and got[1] == 11.0 / 9.0 * 9.0
    assert pkg.sk_sigma(400) == 0.1


def object_argument_errors(pkg):
    """What needs an object (so a device): Detrend::Linear, a channel out of range, a null sample pointer.  Called from here when a
    device is visible, and from tests/test_gpu_sk.py."""
    L = pkg.lib()
    b = pkg.SkCascadeBank(256, 2)
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED and "psdc_sk_set_detrend" in str(e.value)  # as everywhere
    with pytest.raises(pkg.PsdError) as e:
        b.set_detrend(9)
    assert e.value.code == pkg.ERR_ARG
    x = np.zeros(1000, np.float32)
    for call in (lambda: b.process(2, x), lambda: b.process_device(7, 4096, 10), lambda: b.num_stages(2), lambda: b.psd(2),
                 lambda: b.sk(5), lambda: b.stage_moments(2, 0)):
        with pytest.raises(pkg.PsdError) as e:
            call()
        assert e.value.code == pkg.ERR_ARG and "out of range (n_channels 2)" in str(e.value) and "psdc_sk" in str(e.value)
    assert L.psdc_sk_process(b._h, 0, None, 4) == pkg.ERR_ARG
    assert "psdc_sk_process: null sample pointer" in L.psdc_sk_last_error(b._h).decode()
    assert L.psdc_sk_process_device(b._h, 0, None, 4, None) == pkg.ERR_ARG
    assert "psdc_sk_process_device: null sample pointer" in L.psdc_sk_last_error(b._h).decode()
    assert L.psdc_sk_process(b._h, 0, None, 0) == 0  # nothing to read
    with pytest.raises(pkg.PsdError) as e:
        b.stage_moments(0, 0)  # no sample yet: no stage
    assert e.value.code == pkg.ERR_ARG and "psdc_sk_stage_moments: stage 0 out of range" in str(e.value)
    p, br = b.psd(0)
    s, br2 = b.sk(0)
    assert p.size == 0 and s.size == 0 and br == br2 == []
    b.close()


def test_sk_argument_errors(pkg):
    import ctypes as C
    from conftest import has_gpu
    L = pkg.lib()
    for n in (32, 8192, 1000, 0):
        with pytest.raises(pkg.PsdError) as e:
            pkg.SkCascadeBank(n, 1)
        assert e.value.code == pkg.ERR_ARG and "psdc_sk_create: n must be a power of two in [64, 4096]" in str(e.value)
        w = np.ones(max(n, 1), np.float32)
        assert not L.psdc_sk_create_window(n, pkg._fptr(w), 1.0, 1.0, 0, 1, 0)
        assert "psdc_sk_create_window: n must be a power of two in [64, 4096]" in L.psdc_sk_last_error(None).decode()
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not L.psdc_sk_create_window(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in L.psdc_sk_last_error(None).decode()
    assert not L.psdc_sk_create_window(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in L.psdc_sk_last_error(None).decode()
    assert not L.psdc_sk_create(256, 7, 1, 0)
    assert "window_kind" in L.psdc_sk_last_error(None).decode()
    assert not L.psdc_sk_create(256, 1, 0, 0)
    assert "n_channels" in L.psdc_sk_last_error(None).decode()
    assert L.psdc_sk_process(None, 0, None, 4) == pkg.ERR_ARG
    assert "psdc_sk_process: null handle" in L.psdc_sk_last_error(None).decode()
    for rc in (L.psdc_sk_process_device(None, 0, None, 4, None), L.psdc_sk_sync(None), L.psdc_sk_reset(None),
               L.psdc_sk_set_detrend(None, 0), L.psdc_sk_set_avg(None, 1, 1), L.psdc_sk_num_stages(None, 0),
               L.psdc_sk_stage_moments(None, 0, 0, None, None, None),
               L.psdc_sk_psd(None, 0, 0, 1, 0, None, 0, None, None, 0, None),
               L.psdc_sk_sk(None, 0, 0, 1, 0, None, 0, None, None, 0, None),
               L.psdc_sk_stats_read(None, C.byref(C.c_uint64()), None, 0)):
        assert rc == pkg.ERR_ARG
    L.psdc_sk_destroy(None)
    with pytest.raises(pkg.PsdError) as e:
        pkg.SkCascadeBank(256, 1, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG
    if has_gpu():
        object_argument_errors(pkg)


def test_sk_no_gpu_fails_loudly(pkg):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    if has_gpu():
        pkg.SkCascade(1024).close()
        return
    with pytest.raises(pkg.PsdError) as e:
        pkg.SkCascade(1024)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)


# ---- the restatement is anchored ----

def _custom(pkg, n):
    wt = pkg.WindowTable.hann(n)
    return (np.sqrt(wt.win).astype(np.float32), 0.5, 1.2, n // 4)


@pytest.mark.parametrize("n,window,detrend,avg,length", [
    (64, "hann", "none", None, 40_000),
    (128, "rect", "mean", None, 30_000),
    (256, "hann", "span", (U32_MAX, 500), 60_000),
    (64, "custom", "midpoint", (40, U32_MAX), 30_000),
])
def test_restatement_s1_is_sxx_and_the_oracle(pkg, ora, n, window, detrend, avg, length):
    """restate_sk's S1 is restate's Sxx bit for bit in both precisions (counts, averages and pendings equal), and the oracle's f64
    PsdCascade to 1e-12 at every stage.  S2 of a stage with one segment is S1 squared.  (A check of the yardstick, not of the
    library: it uses the oracle alone.)"""
    x = gaussian(length, n)
    win = _custom(pkg, n) if window == "custom" else window
    avg = avg or (U32_MAX, U32_MAX)
    for prec in ("f64", "f32"):
        st = restate_sk(ora, x, n, win, detrend, avg, prec)
        rs = restate(ora, x, x, n, win, detrend, avg, prec)
        assert len(st) == len(rs)
        for k, (s, r) in enumerate(zip(st, rs)):
            assert (s["count"], s["avg"], s["pending"]) == (r["count"], r["avg"], r["pending"]), k
            assert s["s1"].dtype == r["sxx"].dtype and s["s1"].tobytes() == r["sxx"].tobytes(), (prec, k)
            assert s["s2"].dtype == s["s1"].dtype
            if s["count"] == 1:
                assert np.array_equal(s["s2"], s["s1"] * s["s1"]), k
    st = restate_sk(ora, x, n, win, detrend, avg, "f64")
    ref = ora.PsdCascade(n, "f64", window=win)
    ref.set_detrend(detrend)
    ref.set_avg(*avg)
    ref.process(x)
    assert ref.num_stages == len(st)
    for k, s in enumerate(st):
        info = ref.stage_info(k)
        assert (info["count"], info["pending"]) == (s["count"], s["pending"]), k
        r = ref.stage_spectrum(k)
        assert np.max(np.abs(s["s1"] - r) / np.maximum(r, 1e-300)) <= 1e-12, k
    assert restate_sk(ora, x, n, win, detrend, avg, "f64", max_stages=1)[0]["s2"].tobytes() == st[0]["s2"].tobytes()


# ---- the kernel's per-bin arithmetic on the host ----

_EMUL = {}


def sk_emul_exe(tmp_dir, sanitize):
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "sk_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "sk_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def sk_emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sk_emul")


def run_sk_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    got = re.findall(r"sk N=(\d+) worst ([0-9.e+-]+) bound ([0-9.e+-]+) \((P2?)\)", r.stdout)
    assert sorted((int(n), row) for n, _, _, row in got) == [(64, "P"), (64, "P2"), (1024, "P"), (1024, "P2")]
    for n, worst, bound, row in got:
        # P: the bound tests/host/cross_emul.cpp asserts for |X|^2; P^2: twice that (squaring doubles a relative error)
        assert float(bound) == (2e-6 if row == "P" else 4e-6) and float(worst) <= float(bound), (n, row, worst, bound)
    assert "WRONG" not in r.stdout and "FAIL" not in r.stdout
    # with and without EWMA weights, among them one whose square is 0 in f32, and the odd last segment
    assert "wa=1 " in r.stdout and "wa=7.89e-31" in r.stdout and "b_live=0" in r.stdout


def test_sk_bin_emulation(sk_emul_dir):
    """csrc/sk_fft.h for every lane against an f64 DFT at N = 64 and 1024: separation, P and P^2 of both segments, weights and the
    row layout (tests/host/sk_emul.cpp; the program asserts, the figures it prints are checked again here)"""
    run_sk_emul(sk_emul_exe(sk_emul_dir, sanitize=False))


def test_sk_bin_emulation_under_sanitizers(sk_emul_dir):
    """the same program built with -fsanitize=address,undefined: the frame and the partial rows have their exact sizes"""
    run_sk_emul(sk_emul_exe(sk_emul_dir, sanitize=True))


# ---- statistical properties of the f64 restatement ----

def test_restatement_gaussian_noise_reads_one(pkg, ora):
    st = prop_restatement(ora, "gauss")
    check_gauss(lambda k: pkg.sk_from_moments(st[k]["count"], st[k]["s1"], st[k]["s2"]), [s["count"] for s in st])
    # the two real-valued bins read 2 (one degree of freedom); a loose bound, their scatter at this count is below 0.1
    s = st[0]
    sk = pkg.sk_from_moments(s["count"], s["s1"], s["s2"])
    print(f"gauss stage 0: SK at bin 0 {sk[0]:.3f}, at bin N/2 {sk[-1]:.3f}")
    assert abs(sk[0] - 2.0) < 0.5 and abs(sk[-1] - 2.0) < 0.5


def test_restatement_tone_reads_zero(pkg, ora):
    s = prop_restatement(ora, "tone")[0]
    check_tone(pkg.sk_from_moments(s["count"], s["s1"], s["s2"]))


def test_restatement_gated_noise_reads_above_two(pkg, ora):
    s = prop_restatement(ora, "gated")[0]
    check_gated(pkg.sk_from_moments(s["count"], s["s1"], s["s2"]))
