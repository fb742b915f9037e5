"""Stream frames into cross objects (psdc_csd_*): the parts that run without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSD_SYMBOLS = {"psdc_csd_process_frames", "psdc_csd_process_frames_device", "psdc_csd_loss_read"}


def test_csd_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_csd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == CSD_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_csd_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert "#define PSDC_TRACE_NONE 0xFFFFFFFFu" in hdr
    assert "H1 from DAC0 to ADC0" in hdr


def test_null_handle(pkg):
    L = pkg.lib()
    m = np.array([0, 2], np.uint32)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint32))
    frame = np.zeros(72, np.uint8)
    ok = C.c_size_t(99)
    calls = {
        "psdc_csd_process_frames": lambda: L.psdc_csd_process_frames(None, mp, frame.ctypes.data_as(C.c_void_p), 72, 1, C.byref(ok)),
        "psdc_csd_process_frames_device": lambda: L.psdc_csd_process_frames_device(None, mp, None, 72, 1, C.byref(ok), None),
        "psdc_csd_loss_read": lambda: L.psdc_csd_loss_read(None, C.byref(pkg._CLoss()), 0),
    }
    for name, call in calls.items():
        ok.value = 99
        assert call() == pkg.ERR_ARG, name
        assert L.psdc_cross_last_error(None).decode() == f"{name}: null handle"
        if name != "psdc_csd_loss_read":
            assert ok.value == 0, name


def test_pair_map(pkg):
    NONE = pkg.TRACE_NONE
    m = pkg.pair_map([("ADC0", "DAC0"), None, (3, "ADC1"), ("AR", "BQ"), ("phase (rad)", "amplitude (V/G10)")], 6)
    assert m.dtype == np.uint32
    assert m.tolist() == [0, 2, NONE, NONE, 3, 1, 0, 3, 0, 2, NONE, NONE]
    for bad in ([("ADC0", "nope")], [(0, 1)] * 3):
        try:
            pkg.pair_map(bad, 2)
        except pkg.PsdError as e:
            assert e.code == pkg.ERR_ARG
        else:
            raise AssertionError(bad)
