"""Stream frames into zoom objects (psdc_zoomcascade_process_frames[_device], psdc_zoomcascade_loss_read): the parts that run without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOOM_FRAMES_SYMBOLS = {"psdc_zoomcascade_process_frames", "psdc_zoomcascade_process_frames_device", "psdc_zoomcascade_loss_read"}


def test_zoom_frames_symbols_declared(pkg):
    """declared in the header and mirrored (tests/test_host_logic.py then holds the library to every declared symbol)"""
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_zoomcascade_[a-z0-9_]+)\s*\(", hdr))
    assert declared == ZOOM_FRAMES_SYMBOLS
    assert ZOOM_FRAMES_SYMBOLS <= set(pkg.EXPORTS)
    L = pkg.lib()
    for name in ZOOM_FRAMES_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
    # each call cites what it mirrors, and the invariants are written down
    for text in ("mirrors psdc_csd_process_frames)", "mirrors psdc_csd_process_frames_device)", "mirrors psdc_csd_loss_read)",
                 "Invariants:", "(a) a call that is one piece", "(d) a steady-state call of one piece"):
        assert text in hdr, text
    assert "#define PSDC_ABI_VERSION 3" in hdr  # additive: the version stays
    assert L.psdc_abi_version() == 3


def test_null_handle(pkg):
    L = pkg.lib()
    m = np.array([0], np.uint32)
    mp = m.ctypes.data_as(C.POINTER(C.c_uint32))
    frame = np.zeros(72, np.uint8)
    ok = C.c_size_t(99)
    calls = {
        "psdc_zoomcascade_process_frames": lambda: L.psdc_zoomcascade_process_frames(None, mp, frame.ctypes.data_as(C.c_void_p), 72, 1, C.byref(ok)),
        "psdc_zoomcascade_process_frames_device": lambda: L.psdc_zoomcascade_process_frames_device(None, mp, None, 72, 1, C.byref(ok), None),
        "psdc_zoomcascade_loss_read": lambda: L.psdc_zoomcascade_loss_read(None, C.byref(pkg._CLoss()), 0),
    }
    for name, call in calls.items():
        ok.value = 99
        assert call() == pkg.ERR_ARG, name
        assert L.psdc_zoom_last_error(None).decode() == f"{name}: null handle"
        if name != "psdc_zoomcascade_loss_read":
            assert ok.value == 0, name


def test_channel_map_indices_labels_none(pkg):
    NONE = pkg.TRACE_NONE
    m = pkg.channel_map([0, None, 3, "DAC0", 1], 7)
    assert m.dtype == np.uint32
    assert m.tolist() == [0, NONE, 3, 2, 1, NONE, NONE]
    # one trace may feed every channel
    assert pkg.channel_map(["ADC1"] * 17, 17).tolist() == [1] * 17
    # numpy integers are indices too
    assert pkg.channel_map([np.int64(2)], 1).tolist() == [2]


@pytest.mark.parametrize("fmt", [1, 2, 3, 4])
def test_channel_map_labels_of_every_format(pkg, fmt):
    names = pkg.TRACE_NAMES[pkg.Format(fmt)]
    assert pkg.channel_map(list(names), 4).tolist() == list(range(len(names))) + [pkg.TRACE_NONE] * (4 - len(names))


@pytest.mark.parametrize("bad,n", [
    (["nope"], 1),            # unknown label
    ([4], 1),                 # index >= 4
    ([0, 7], 2),
    ([-1], 1),
    ([], 2),                  # empty map: no fed channel
    ([None, None], 2),
    ([0, 1, 2], 2),           # more entries than channels
])
def test_channel_map_errors(pkg, bad, n):
    with pytest.raises(pkg.PsdError) as e:
        pkg.channel_map(bad, n)
    assert e.value.code == pkg.ERR_ARG
