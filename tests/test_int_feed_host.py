"""Integer sample feeds (psdc_int_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "integer sample feeds".

The index map, the unpack-and-scale and the three integer mixers of csrc/sample_int.h run on the host in
tests/host/sample_int_emul.cpp, which this file compiles itself: once plainly and once under the address and undefined-behaviour
sanitizers (a stand-alone program; nothing is loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_zoom_host import ROOT

INT_SYMBOLS = ["psdc_int_zoom_process", "psdc_int_zoom_process_device", "psdc_int_zcsd_process", "psdc_int_zcsd_process_device",
               "psdc_int_iq_process", "psdc_int_iq_process_device", "psdc_int_iqcsd_process", "psdc_int_iqcsd_process_device"]

_EMUL = {}


def sample_int_emul_exe(tmp_dir, sanitize):
    """tests/host/sample_int_emul.cpp compiled once a session and flavour (-ffp-contract=off, as the other emulation builds)"""
    key = "san" if sanitize else "plain"
    if key not in _EMUL:
        exe = os.path.join(str(tmp_dir), "sample_int_emul_" + key)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "sample_int_emul.cpp"), "-o", exe], check=True)
        _EMUL[key] = exe
    return _EMUL[key]


@pytest.fixture(scope="session")
def emul_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sample_int_emul")


def run_emul(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert "sample_int: all checks hold" in out
    # every part ran, and on every kind
    for part in ("unpack s16:", "unpack s8:", "map:", "mix s16:", "mix s8:"):
        assert part in out, part
    # every int16 value, 3 scales, (2 lanes x 3 surroundings + load1 + 2 x 2 load1c + 4 + 8 group positions)
    assert int(re.search(r"unpack s16: (\d+) conversions", out).group(1)) == 65536 * 3 * (2 * 3 + 4 + 4 + 8)
    assert int(re.search(r"unpack s8: (\d+) conversions", out).group(1)) == 256 * 3 * (4 * 3 + 4 + 4 + 8)


def test_int_feed_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_int_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(INT_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert set(re.findall(r" T (psdc_int_[a-z0-9_]+)", out)) == declared
    assert declared <= set(pkg.EXPORTS)
    assert pkg.lib().psdc_abi_version() == 3
    # the conversion rule and the defining property are written down
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "the f32 sample the mixer sees is (float)v * scale" in hdr
    assert "one stand-alone f32 product rounded to nearest" in flat
    assert "except the integer feeds below" in flat
    assert re.search(r"#define PSDC_SAMPLE_S16 1\b", hdr) and re.search(r"#define PSDC_SAMPLE_S8 2\b", hdr)
    assert int(pkg.SampleKind.S16) == 1 and int(pkg.SampleKind.S8) == 2
    for cls in ("ZoomCascadeBank", "ZoomCascade", "ZoomCsdCascadeBank", "ZoomCsdCascade", "IqCascadeBank", "IqCascade",
                "IqCsdCascadeBank", "IqCsdCascade"):
        for m in ("process_int", "process_int_device"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)


def test_sample_int_header_on_the_host(emul_dir):
    """unpack (all 65536 + 256 values in every lane position, three scales), index map (every kind, head, misalignment and
    length) and mixer parity (equal bits with zoom_mix / iq_mix, without and with carriers, shared and distinct on a pair)"""
    run_emul(sample_int_emul_exe(emul_dir, sanitize=False))


def test_sample_int_header_under_sanitizers(emul_dir):
    """the same program built with -fsanitize=address,undefined: its buffers have the exact size, so a byte read or written
    outside a source or a destination stops it"""
    run_emul(sample_int_emul_exe(emul_dir, sanitize=True))


def test_sample_kind(pkg):
    assert pkg.sample_kind(np.int16) == (pkg.SampleKind.S16, 2.0 ** -15)
    assert pkg.sample_kind(np.dtype("int8")) == (pkg.SampleKind.S8, 2.0 ** -7)
    assert pkg.sample_kind(np.zeros(3, np.int16).dtype)[0] is pkg.SampleKind.S16
    for bad in (np.float32, np.int32, np.uint8, np.uint16, np.complex64, np.int64):
        with pytest.raises(ValueError):
            pkg.sample_kind(bad)
    # full scale maps into [-1, 1)
    for dt in (np.int16, np.int8):
        info, (_, scale) = np.iinfo(dt), pkg.sample_kind(dt)
        assert info.min * scale == -1.0 and info.max * scale < 1.0


def test_int_argument_handling_without_a_device(pkg):
    """Bad dtype, shape or contiguity raises ValueError before any library call: on the module's checks, and through the objects'
    methods on an object that was never created (its handle does not exist, so a library call would raise something else)."""
    x16, x8 = np.arange(12, dtype=np.int16), np.arange(12, dtype=np.int8)
    a, kind, scale = pkg.int_samples(x16)
    assert a is x16 and kind == pkg.SampleKind.S16 and scale == 2.0 ** -15
    a, kind, scale = pkg.int_samples(x8[3:])
    assert a.ctypes.data == x8.ctypes.data + 3 and kind == pkg.SampleKind.S8 and scale == 2.0 ** -7
    z = x16.reshape(6, 2)
    a, kind, scale = pkg.int_pairs(z)
    assert a is z and kind == pkg.SampleKind.S16
    assert pkg.int_pairs(x8.reshape(6, 2)[1:])[1] == pkg.SampleKind.S8
    bad_real = [x16.astype(np.float32), x16.astype(np.int32), x16.astype(np.uint16), x16[::2], x16.reshape(6, 2), list(x16), x16.reshape(12, 1)]
    bad_pairs = [z.astype(np.float32), z.astype(np.complex64), z.astype(np.uint8), x16, x16.reshape(4, 3), x16.reshape(2, 6).T,
                 x16.reshape(2, 3, 2), z[::2], np.asfortranarray(z), z.tolist()]
    for bad in bad_real:
        with pytest.raises(ValueError):
            pkg.int_samples(bad)
    for bad in bad_pairs:
        with pytest.raises(ValueError):
            pkg.int_pairs(bad)
    for cls, complex_ in ((pkg.ZoomCascadeBank, False), (pkg.IqCascadeBank, True)):
        obj = object.__new__(cls)  # no handle, no library: only the argument checks can run
        for bad in (bad_pairs if complex_ else bad_real):
            with pytest.raises(ValueError):
                obj.process_int(0, bad)
    for cls, complex_ in ((pkg.ZoomCsdCascadeBank, False), (pkg.IqCsdCascadeBank, True)):
        obj = object.__new__(cls)
        good = z if complex_ else x16
        for bad in (bad_pairs if complex_ else bad_real):
            with pytest.raises(ValueError):
                obj.process_int(0, good, bad)
            with pytest.raises(ValueError):
                obj.process_int(0, bad, good)
        with pytest.raises(ValueError):  # the sides differ in dtype, and in length
            obj.process_int(0, good, good.astype(np.int8))
        with pytest.raises(ValueError):
            obj.process_int(0, good, good[:-1])
