"""IQ cross cascade (psdc_iqcsd_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "IQ cross cascade".

The yardstick of tests/test_gpu_iq_cross.py is restate_zoom_cross of tests/test_zoom_cross_host.py fed
iq = (mix_c_f64(side a), mix_c_f64(side b)): the zoom cross restatement with the complex f64 mix of tests/test_iq_host.py in front
of it.  It is anchored here to the restatement of real streams: with Q = 0 the complex mix is the real one."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_iq_host import mix_c_f64
from test_zoom_cross_host import pair_input, restate_zoom_cross
from test_zoom_host import ROOT

IQCSD_SYMBOLS = ["psdc_iqcsd_supported", "psdc_iqcsd_create", "psdc_iqcsd_create_window", "psdc_iqcsd_destroy", "psdc_iqcsd_reset",
                 "psdc_iqcsd_set_detrend", "psdc_iqcsd_set_avg", "psdc_iqcsd_set_carrier", "psdc_iqcsd_process",
                 "psdc_iqcsd_process_device", "psdc_iqcsd_process_interleaved", "psdc_iqcsd_process_interleaved_device",
                 "psdc_iqcsd_process_frames", "psdc_iqcsd_process_frames_device", "psdc_iqcsd_loss_read", "psdc_iqcsd_sync",
                 "psdc_iqcsd_num_stages", "psdc_iqcsd_stats_read", "psdc_iqcsd_last_error", "psdc_iqcsd_stage_spectra",
                 "psdc_iqcsd_csd"]


def test_iqcsd_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_iqcsd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(IQCSD_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_iqcsd_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert pkg.lib().psdc_abi_version() == 3
    m = re.search(r"#define PSDC_IQCSD_STEADY_LAUNCHES (\d+)", hdr)
    assert m and int(m.group(1)) == pkg.IQCSD_STEADY_LAUNCHES == 4  # 1 + 3
    for name in ("IqCsdCascadeBank", "IqCsdCascade", "iq_pair_map", "iqcsd_supported"):
        assert hasattr(pkg, name)


def test_iqcsd_supported(pkg):
    for n in (0, *(32 << k for k in range(8)), 1000, 8192):  # 0, 32, 64 ... 4096, 1000, 8192
        assert pkg.iqcsd_supported(n) == pkg.zcsd_supported(n), n
    assert pkg.iqcsd_supported(64) and pkg.iqcsd_supported(2048) and not pkg.iqcsd_supported(32)


def test_iq_pair_map(pkg):
    NONE = pkg.TRACE_NONE
    assert pkg.iq_pair_map([(("BI", "BQ"), ("AR", "AP"))], 2).tolist() == [2, 3, pkg.trace_index("AR"), pkg.trace_index("AP")] + [NONE] * 4
    assert pkg.iq_pair_map([None, ((0, 1), (2, 2)), ((3, 1), (0, 2))], 3).tolist() == [NONE] * 4 + [0, 1, 2, 2, 3, 1, 0, 2]
    # a pair with all four entries None is accepted: it is not fed
    assert pkg.iq_pair_map([((None, None), (None, None)), ((0, 1), (2, 3))], 2).tolist() == [NONE] * 4 + [0, 1, 2, 3]
    bad = [[((0, 1), (2, 3))] * 3,               # more entries than pairs
           [None, None],                         # feeds nothing
           [((None, None), (None, None))],       # feeds nothing
           [((0, None), (2, 3))], [((0, 1), (None, 3))], [((None, None), (2, 3))], [((0, None), (None, None))],  # 1 ... 3 None
           [((0, 1), (2, 4))], [((0, 1), (2, "nonesuch"))], [(0, 1)], [(0, 1, 2, 3)], [2], ["BI"]]
    for b in bad:
        with pytest.raises(pkg.PsdError) as e:
            pkg.iq_pair_map(b, 2)
        assert e.value.code == pkg.ERR_ARG, b


def test_iqcsd_argument_errors(pkg):
    """What can be refused without a device: sizes, windows, pair counts, NULL handles.  (Pair and side out of range,
    Detrend::Linear and the pointer checks need an object: tests/test_gpu_iq_cross.py.)"""
    L = pkg.lib()
    for n in (1000, 32, 8192, 0):
        with pytest.raises(pkg.PsdError) as e:
            pkg.IqCsdCascadeBank(n, 1)
        assert e.value.code == pkg.ERR_ARG and f"n = {n} is not supported" in str(e.value)
        w = np.ones(max(n, 1), np.float32)
        assert not L.psdc_iqcsd_create_window(n, pkg._fptr(w), 1.0, 1.0, 0, 1, 0)
        assert f"n = {n} is not supported" in L.psdc_iqcsd_last_error(None).decode()
    w = np.ones(256, np.float32)
    for ov in (4, 256):
        assert not L.psdc_iqcsd_create_window(256, pkg._fptr(w), 1.0, 1.0, ov, 1, 0)
        assert "overlap" in L.psdc_iqcsd_last_error(None).decode()
    assert not L.psdc_iqcsd_create_window(256, None, 1.0, 1.0, 0, 1, 0)
    assert "null window" in L.psdc_iqcsd_last_error(None).decode()
    assert not L.psdc_iqcsd_create(256, 7, 1, 0)
    assert "window_kind" in L.psdc_iqcsd_last_error(None).decode()
    assert not L.psdc_iqcsd_create(256, 1, 0, 0)
    assert "n_pairs" in L.psdc_iqcsd_last_error(None).decode()
    assert L.psdc_iqcsd_process(None, 0, None, None, None, None, 4) == pkg.ERR_ARG
    assert "null handle" in L.psdc_iqcsd_last_error(None).decode()
    ok = C.c_size_t(5)
    for rc in (L.psdc_iqcsd_process_device(None, 0, None, None, None, None, 4, None),
               L.psdc_iqcsd_process_interleaved(None, 0, None, None, 4),
               L.psdc_iqcsd_process_interleaved_device(None, 0, None, None, 4, None), L.psdc_iqcsd_sync(None),
               L.psdc_iqcsd_reset(None), L.psdc_iqcsd_set_carrier(None, 0, 0, 1, 2), L.psdc_iqcsd_set_detrend(None, 0),
               L.psdc_iqcsd_set_avg(None, 1, 1), L.psdc_iqcsd_num_stages(None, 0),
               L.psdc_iqcsd_stage_spectra(None, 0, 0, None, None),
               L.psdc_iqcsd_csd(None, 0, 0, 1, 0, None, None, None, None, None, None, 0, None, None, 0, None),
               L.psdc_iqcsd_stats_read(None, C.byref(C.c_uint64()), None, 0), L.psdc_iqcsd_loss_read(None, None, 0),
               L.psdc_iqcsd_process_frames(None, None, None, 200, 1, C.byref(ok)),
               L.psdc_iqcsd_process_frames_device(None, None, None, 200, 1, C.byref(ok), None)):
        assert rc == pkg.ERR_ARG
    assert ok.value == 0
    L.psdc_iqcsd_destroy(None)
    with pytest.raises(pkg.PsdError) as e:
        pkg.IqCsdCascadeBank(256, 1, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG


def test_iqcsd_no_gpu_fails_loudly(pkg):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    if has_gpu():
        pkg.IqCsdCascade(1024, f0=0.2).close()
        return
    with pytest.raises(pkg.PsdError) as e:
        pkg.IqCsdCascade(1024, f0=0.2)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)


def test_restatement_with_q_zero_is_the_real_restatement(pkg, ora):
    """A check of the yardstick (it passes without the library's new code): with Q_a = Q_b = 0 the f64 complex mix is the f64
    real mix, so restate_zoom_cross(iq = (mix_c_f64(a, 0), mix_c_f64(b, 0))) equals restate_zoom_cross of the real streams with
    the same carriers: stages, counts and pendings equal, the auto rows within 1e-12 relative and the cross rows within 1e-12
    of sqrt(S_aa S_bb).  N = 64, two different carriers with start phases."""
    n = 64
    a, b = pair_input(30_000, 1234)
    ftw = (pkg.zoom_ftw(0.2345678901234567)[0], pkg.zoom_ftw(0.7131313131313131)[0])
    ph = (0x0123456789ABCDEF, 1 << 63)
    zero = np.zeros_like(a)
    got = restate_zoom_cross(ora, None, None, n, ftw, ph, iq=(mix_c_f64(a, zero, ftw[0], ph[0]), mix_c_f64(b, zero, ftw[1], ph[1])))
    want = restate_zoom_cross(ora, a, b, n, ftw, ph)
    assert len(got) == len(want) >= 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["count"], g["avg"], g["pending"]) == (w["count"], w["avg"], w["pending"]), k
        for r in range(4):
            assert np.all(np.abs(g["rows"][r] - w["rows"][r]) <= 1e-12 * np.abs(w["rows"][r])), (k, r)
        for r in range(4, 8):
            scale = np.sqrt(w["rows"][r % 2] * w["rows"][2 + r % 2])
            assert np.all(np.abs(g["rows"][r] - w["rows"][r]) <= 1e-12 * scale), (k, r)
