"""Stream frames into zoom cross objects (psdc_zoomcsdcascade_process_frames[_device], psdc_zoomcsdcascade_loss_read): the parts that
run without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZCSD_FRAMES_SYMBOLS = {"psdc_zoomcsdcascade_process_frames", "psdc_zoomcsdcascade_process_frames_device",
                       "psdc_zoomcsdcascade_loss_read"}


def test_zoom_cross_frames_symbols_declared(pkg):
    """declared in the header, exported by the library and mirrored; the prefix collides with no other object's closed set"""
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_zoomcsdcascade_[a-z0-9_]+)\s*\(", hdr))
    assert declared == ZCSD_FRAMES_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_zoomcsdcascade_[a-z0-9_]+)", out)) == ZCSD_FRAMES_SYMBOLS
    assert ZCSD_FRAMES_SYMBOLS <= set(pkg.EXPORTS)
    L = pkg.lib()
    for name in ZCSD_FRAMES_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
        for other in ("psdc_zcsd_", "psdc_zoomcascade_", "psdc_zoom_", "psdc_csd_", "psdc_cross_", "psdc_csm_"):
            assert not re.search(r"\b" + other, name), (name, other)
    # each call cites what it mirrors, the invariants are written down, and the old sentence is gone
    sec = hdr[hdr.index("Stream frames into zoom cross pairs (mirrors"):hdr.index("int psdc_zcsd_sync")]
    for text in ("mirrors psdc_csd_process_frames)", "mirrors psdc_csd_process_frames_device)", "mirrors psdc_csd_loss_read)",
                 "Invariants:", "(a) a call that is one piece", "(b) the same frames in host and in device memory",
                 "(c) sample and frame calls may be mixed on one pair", "(d) a steady-state call of one piece", "Memory:"):
        assert text in sec, text
    assert "Stream frames do not feed this object" not in hdr
    assert "#define PSDC_ABI_VERSION 3" in hdr  # additive: the version stays
    assert L.psdc_abi_version() == 3


def test_null_handle(pkg):
    L = pkg.lib()
    m = np.array([0, 1], np.uint32)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint32))
    frame = np.zeros(72, np.uint8)
    ok = C.c_size_t(99)
    calls = {
        "psdc_zoomcsdcascade_process_frames":
            lambda: L.psdc_zoomcsdcascade_process_frames(None, mp, frame.ctypes.data_as(C.c_void_p), 72, 1, C.byref(ok)),
        "psdc_zoomcsdcascade_process_frames_device":
            lambda: L.psdc_zoomcsdcascade_process_frames_device(None, mp, None, 72, 1, C.byref(ok), None),
        "psdc_zoomcsdcascade_loss_read": lambda: L.psdc_zoomcsdcascade_loss_read(None, C.byref(pkg._CLoss()), 0),
    }
    for name, call in calls.items():
        ok.value = 99
        assert call() == pkg.ERR_ARG, name
        assert L.psdc_zcsd_last_error(None).decode() == f"{name}: null handle"
        if name != "psdc_zoomcsdcascade_loss_read":
            assert ok.value == 0, name


def test_methods_exist(pkg):
    for cls in (pkg.ZoomCsdCascadeBank, pkg.ZoomCsdCascade):
        for name in ("process_frames", "process_frames_device", "loss"):
            assert callable(getattr(cls, name)), (cls, name)


def test_pair_map_indices_labels_none(pkg):
    """the map the zoom cross frames calls take is pair_map's: a regression anchor"""
    NONE = pkg.TRACE_NONE
    m = pkg.pair_map([(0, 1), None, ("DAC0", 3), (2, 2)], 6)
    assert m.dtype == np.uint32
    assert m.tolist() == [0, 1, NONE, NONE, 2, 3, 2, 2] + [NONE] * 4
    assert pkg.pair_map([("ADC1", "ADC1")] * 9, 9).tolist() == [1] * 18
    assert pkg.pair_map([(np.int64(2), np.int32(0))], 1).tolist() == [2, 0]
    assert pkg.pair_map([], 2).tolist() == [NONE] * 4


@pytest.mark.parametrize("fmt", [1, 2, 3, 4])
def test_pair_map_labels_of_every_format(pkg, fmt):
    names = pkg.TRACE_NAMES[pkg.Format(fmt)]
    pairs = [(a, b) for a in names for b in names]
    want = [i for a in range(len(names)) for b in range(len(names)) for i in (a, b)]
    assert pkg.pair_map(pairs, len(pairs)).tolist() == want


@pytest.mark.parametrize("bad,n", [
    ([("nope", 0)], 1),                  # unknown label
    ([(0, "nope")], 1),
    ([(0, 1), (1, 0), (2, 3)], 2),       # more pairs than the bank has
])
def test_pair_map_errors(pkg, bad, n):
    with pytest.raises(pkg.PsdError) as e:
        pkg.pair_map(bad, n)
    assert e.value.code == pkg.ERR_ARG
