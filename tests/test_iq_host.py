"""IQ cascade (psdc_iq_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "IQ cascade".

The yardstick of tests/test_gpu_iq.py is restate_zoom of tests/test_zoom_host.py fed iq = mix_c_f64(...): the zoom restatement
with the complex f64 mix from exact integer phases in front of it.  It is anchored to the oracle here through restate_zoom's own
anchors: a complex stream z = x exp(+2 pi i f0 j) retuned by the same f0 is x again.  The mixer itself (csrc/iq_lo.h) runs on the
host in tests/host/iq_emul.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_zoom_host import M64, ROOT, emul, mix_f32, noise, phases, restate_zoom  # noqa: F401

IQ_SYMBOLS = ["psdc_iq_create", "psdc_iq_create_window", "psdc_iq_destroy", "psdc_iq_reset", "psdc_iq_set_detrend", "psdc_iq_set_avg",
              "psdc_iq_set_carrier", "psdc_iq_process", "psdc_iq_process_device", "psdc_iq_process_interleaved",
              "psdc_iq_process_interleaved_device", "psdc_iq_process_frames", "psdc_iq_process_frames_device", "psdc_iq_loss_read",
              "psdc_iq_sync", "psdc_iq_num_stages", "psdc_iq_stage_spectra", "psdc_iq_psd", "psdc_iq_stats_read", "psdc_iq_last_error"]

_EMUL = {}


def iq_emul_exe(tmp_dir):
    """tests/host/iq_emul.cpp compiled once a session (-ffp-contract=off: iq_lo.h leaves nothing to contract anyway)."""
    if "exe" not in _EMUL:
        exe = os.path.join(str(tmp_dir), "iq_emul")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "iq_emul.cpp"), "-o", exe], check=True)
        _EMUL["exe"] = exe
    return _EMUL["exe"]


@pytest.fixture(scope="session")
def iq_emul(tmp_path_factory):
    return iq_emul_exe(tmp_path_factory.mktemp("iq_emul"))


def mix_c_f64(i, q, ftw, phase0=0):
    """(I', Q') = z exp(-2 pi i phi_j / 2^64) in f64 from the exact integer phases (the full 64 bits, rounded once to f64's 53);
    i and q are taken as they are (f32 samples convert exactly)"""
    i, q = np.asarray(i, np.float64), np.asarray(q, np.float64)
    a = 2.0 * np.pi * (phases(i.size, ftw, phase0).astype(np.float64) / 18446744073709551616.0)
    c, s = np.cos(a), np.sin(a)
    return i * c + q * s, q * c - i * s


def mix_c_f32(iq_emul, i, q, ftw, phase0=0):
    """(I', Q') as iq_mix_kernel stores them: csrc/iq_lo.h run on the host"""
    d = os.path.dirname(iq_emul)
    fi, fq, fout = (os.path.join(d, f) for f in ("mix_i.f32", "mix_q.f32", "mix_out.f32"))
    np.asarray(i, np.float32).tofile(fi)
    np.asarray(q, np.float32).tofile(fq)
    subprocess.run([iq_emul, "mix", str(ftw & M64), str(phase0 & M64), fi, fq, fout], check=True)
    out = np.fromfile(fout, np.float32)
    m = np.asarray(i).size
    return out[:m].copy(), out[m:].copy()


def test_iq_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_iq_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(IQ_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_iq_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert pkg.lib().psdc_abi_version() == 3
    assert "I' = fmaf(Q, s,  I * c)" in hdr and "Q' = fmaf(Q, c, -(I * s))" in hdr  # the mix formula is written down
    for cls in ("IqCascadeBank", "IqCascade", "iq_map"):
        assert hasattr(pkg, cls)


def test_iq_mix_matches_f64(iq_emul):
    """The emulated mixer against the f64 complex mix on 50 000 random samples with a start phase: I' and Q' within
    (2^-23 + 2 pi 2^-32 + 2 2^-24) (|I| + |Q|) -- the LO's error, the phase truncation and the two roundings of the formula."""
    i, q = noise(50_000, 19), noise(50_000, 23)
    ftw, ph0 = 0x3C6EF372FE94F82B, 0x9E3779B97F4A7C15
    i32, q32 = mix_c_f32(iq_emul, i, q, ftw, ph0)
    i64, q64 = mix_c_f64(i, q, ftw, ph0)
    tol = (2.0 ** -23 + 2 * np.pi * 2.0 ** -32 + 2 * 2.0 ** -24) * (np.abs(i.astype(np.float64)) + np.abs(q.astype(np.float64)))
    ei, eq = np.abs(i32 - i64), np.abs(q32 - q64)
    print(f"worst error / bound: I' {float(np.max(ei / tol)):.3g}, Q' {float(np.max(eq / tol)):.3g}")
    assert np.all(ei <= tol) and np.all(eq <= tol)


def test_iq_mix_with_q_zero_is_zoom_mix(iq_emul, emul):  # noqa: F811
    """Q = 0: fmaf(0, s, I c) and fmaf(0, c, -(I s)) are zoom_mix's x c and -(x s), bit for bit up to the sign of a zero (== on floats)"""
    x = noise(50_000, 29)
    x[::97] = 0.0
    ftw, ph0 = 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9
    zi, zq = mix_f32(emul, x, ftw, ph0)
    ci, cq = mix_c_f32(iq_emul, x, np.zeros_like(x), ftw, ph0)
    assert np.all(ci == zi) and np.all(cq == zq)
    assert not np.any(np.isnan(ci)) and not np.any(np.isnan(cq))


def test_iq_mix_without_a_carrier_is_the_identity(iq_emul):
    """ftw = phase0 = 0: c = 1 and s = 0 exactly, and the formula returns (I, Q) for finite input"""
    i, q = noise(50_000, 31), noise(50_000, 37)
    i[:4] = [0.0, -0.0, np.float32(3.4e38), np.float32(1e-45)]
    q[:4] = [-0.0, 1.0, np.float32(-3.4e38), 0.0]
    oi, oq = mix_c_f32(iq_emul, i, q, 0, 0)
    assert np.all(oi == i) and np.all(oq == q)


def test_iq_restatement_retuned_is_the_real_restatement(pkg, ora):
    """The yardstick anchored without a GPU: z = x exp(+2 pi i f0 j) built in f64 with f0 on a bin, retuned by the same ftw, is x
    again, so restate_zoom(iq = mix_c_f64(z)) reproduces restate_zoom of the real x at ftw = 0 (which test_zoom_host.py anchors to
    the oracle's cascade): every stage's counts, and both rows within 1e-9 relative.  N = 64, 2^15 samples."""
    n, j, length = 64, 5, 1 << 15
    x = noise(length, 41)
    ftw = (j << 64) // n
    a = 2.0 * np.pi * (phases(length, ftw).astype(np.float64) / 18446744073709551616.0)
    xd = x.astype(np.float64)
    zi, zq = xd * np.cos(a), xd * np.sin(a)
    got = restate_zoom(ora, x, n, ftw, iq=mix_c_f64(zi, zq, ftw))
    want = restate_zoom(ora, x, n, 0)
    assert len(got) == len(want) >= 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["count"], g["avg"], g["pending"]) == (w["count"], w["avg"], w["pending"]), k
        for row in ("upper", "lower"):
            rel = float(np.max(np.abs(g[row] - w[row]) / w[row])) if g["count"] else 0.0
            assert rel <= 1e-9, (k, row, rel)


def test_iq_map(pkg):
    NONE = pkg.TRACE_NONE
    assert pkg.iq_map([("BI", "BQ")], 2).tolist() == [2, 3, NONE, NONE]
    assert pkg.iq_map([None, (0, 1), (3, 3)], 3).tolist() == [NONE, NONE, 0, 1, 3, 3]
    for bad in ([(0, 1)] * 3, [None, None], [(0, None)], [(0, 4)], [(0, "nonesuch")], [2], ["BI"]):
        with pytest.raises(pkg.PsdError) as e:
            pkg.iq_map(bad, 2)
        assert e.value.code == pkg.ERR_ARG, bad


def test_iq_argument_errors(pkg):
    L = pkg.lib()
    for n in (1000, 32, 8192, 0):
        with pytest.raises(pkg.PsdError) as e:
            pkg.IqCascadeBank(n, 1)
        assert e.value.code == pkg.ERR_ARG and "power of two in [64, 4096]" in str(e.value)
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not L.psdc_iq_create_window(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in L.psdc_iq_last_error(None).decode()
    assert not L.psdc_iq_create_window(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in L.psdc_iq_last_error(None).decode()
    assert not L.psdc_iq_create(256, 7, 1, 0)
    assert "window_kind" in L.psdc_iq_last_error(None).decode()
    assert not L.psdc_iq_create(256, 1, 0, 0)
    assert "n_channels" in L.psdc_iq_last_error(None).decode()
    assert L.psdc_iq_process(None, 0, None, None, 4) == pkg.ERR_ARG
    assert "null handle" in L.psdc_iq_last_error(None).decode()
    ok = C.c_size_t(5)
    for rc in (L.psdc_iq_process_device(None, 0, None, None, 4, None), L.psdc_iq_process_interleaved(None, 0, None, 4),
               L.psdc_iq_process_interleaved_device(None, 0, None, 4, None), L.psdc_iq_sync(None), L.psdc_iq_reset(None),
               L.psdc_iq_set_carrier(None, 0, 1, 2), L.psdc_iq_set_detrend(None, 0), L.psdc_iq_set_avg(None, 1, 1),
               L.psdc_iq_num_stages(None, 0), L.psdc_iq_stage_spectra(None, 0, 0, None, None, None),
               L.psdc_iq_psd(None, 0, 0, 1, 0, None, None, 0, None, None, 0, None),
               L.psdc_iq_stats_read(None, C.byref(C.c_uint64()), None, 0), L.psdc_iq_loss_read(None, None, 0),
               L.psdc_iq_process_frames(None, None, None, 200, 1, C.byref(ok)),
               L.psdc_iq_process_frames_device(None, None, None, 200, 1, C.byref(ok), None)):
        assert rc == pkg.ERR_ARG
    assert ok.value == 0
    L.psdc_iq_destroy(None)


def test_iq_no_gpu_fails_loudly(pkg):
    from conftest import has_gpu
    if has_gpu():
        pytest.skip("a HIP device is visible")
    with pytest.raises(pkg.PsdError) as e:
        pkg.IqCascade(1024, f0=0.2)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)
