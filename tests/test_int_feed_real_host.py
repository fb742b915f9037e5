"""Integer sample feeds of the real-input objects (psdc_sint_*: PSD, pair, matrix): the parts that run without a GPU.  Semantics:
include/psdcascade.h, "integer sample feeds of the real-input objects".

The converter's thread function (sint_cvt_thread of csrc/sample_int.h, what sample_cvt_int_kernel runs) runs on the host in
tests/host/sample_cvt_emul.cpp, which this file compiles itself: once plainly and once under the address and undefined-behaviour
sanitizers (a stand-alone program; nothing is loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_zoom_host import ROOT

SINT_SYMBOLS = ["psdc_sint_process", "psdc_sint_process_device", "psdc_sint_cross_process", "psdc_sint_cross_process_device",
                "psdc_sint_csm_process", "psdc_sint_csm_process_device"]
CLASSES = ("PsdCascadeBank", "PsdCascade", "CsdCascadeBank", "CsdCascade", "CsmCascadeBank", "CsmCascade")

_EMUL = {}


def sample_cvt_emul_exe(tmp_dir, sanitize):
    """tests/host/sample_cvt_emul.cpp compiled once a session and flavour (-ffp-contract=off, as the other emulation builds)"""
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "sample_cvt_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "sample_cvt_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def cvt_emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sample_cvt_emul")


def run_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "sample_cvt: all checks hold" in out
    # every value of the type four times over (once at every position of a group) and a partial tail, on 2 channels, 4 destination
    # phases and 3 scales
    assert int(re.search(r"values s16: (\d+) conversions", out).group(1)) == 3 * 4 * 2 * (4 * 65536 + 7)
    assert int(re.search(r"values s8: (\d+) conversions", out).group(1)) == 3 * 4 * 2 * (4 * 256 + 7)
    # 3 scales x nch 1 ... 4 x 4 destination phases x 8 source misalignments x (lengths 0 ... 40 and 12 around 4 * 256)
    lengths = list(range(41)) + list(range(4 * 256 - 5, 4 * 256 + 7))
    for kind in ("s16", "s8"):
        m = re.search(rf"launch {kind}: (\d+) launches, (\d+) outputs", out)
        assert int(m.group(1)) == 3 * 4 * 4 * 8 * len(lengths)
        assert int(m.group(2)) == 3 * 4 * 8 * sum(lengths) * (1 + 2 + 3 + 4)


def test_sint_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_sint_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SINT_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_sint_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert pkg.lib().psdc_abi_version() == 3
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "integer sample feeds of the real-input objects" in flat
    assert "except the integer feeds below" in flat  # (the wording of the existing section stays)
    for cls in CLASSES:
        for m in ("process_int", "process_int_device"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)


def test_sample_cvt_on_the_host(cvt_emul_dir):
    """sint_cvt_thread for every thread of a launch: every value of both types, three scales, nch 1 ... 4, every destination
    phase, per-channel source misalignments, lengths 0 ... 40 and around 4 * 256: equal bits with (float)v * scale, every element
    written once, the guard words intact"""
    run_emul(sample_cvt_emul_exe(cvt_emul_dir, sanitize=False))


def test_sample_cvt_under_sanitizers(cvt_emul_dir):
    """the same program built with -fsanitize=address,undefined: its buffers have the exact size, so a byte read or written
    outside a source or a destination stops it"""
    run_emul(sample_cvt_emul_exe(cvt_emul_dir, sanitize=True))


def test_sint_argument_handling_without_a_device(pkg):
    """Bad dtype, shape, contiguity, unequal sides or a wrong channel count raise ValueError before any library call: the objects
    were never created (no handle exists), so a library call would raise something else."""
    x16 = np.arange(12, dtype=np.int16)
    bad_real = [x16.astype(np.float32), x16.astype(np.int32), x16.astype(np.uint16), x16[::2], x16.reshape(6, 2), list(x16)]
    psd = object.__new__(pkg.PsdCascadeBank)
    for bad in bad_real:
        with pytest.raises(ValueError):
            psd.process_int(0, bad)
    pair = object.__new__(pkg.CsdCascadeBank)
    for bad in bad_real:
        with pytest.raises(ValueError):
            pair.process_int(0, x16, bad)
        with pytest.raises(ValueError):
            pair.process_int(0, bad, x16)
    with pytest.raises(ValueError):  # the sides differ in dtype, and in length
        pair.process_int(0, x16, x16.astype(np.int8))
    with pytest.raises(ValueError):
        pair.process_int(0, x16, x16[:-1])
    mat = object.__new__(pkg.CsmCascadeBank)
    mat.m = 3
    for bad in bad_real:
        with pytest.raises(ValueError):
            mat.process_int(0, [x16, bad, x16])
    for xs in ([x16, x16], [x16] * 4, np.stack([x16] * 3), [x16, x16, x16[:-1]], [x16, x16.astype(np.int8), x16]):
        with pytest.raises(ValueError):  # a wrong number of channels, one array for all, unequal lengths, unequal dtypes
            mat.process_int(0, xs)
    with pytest.raises(ValueError):
        mat.process_int_device(0, [0, 0], 4, pkg.SampleKind.S16)
