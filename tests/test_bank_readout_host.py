"""Bank read-out (include/psdcascade_readout.h, psdcr_*; stabilizer-stream_amd/bankread.py): the parts that run without a GPU.

csrc/bank_readout.h -- the job table made from Break lists, what one thread of bank_stitch_kernel computes for one element and
what bank_band_kernel adds up for one row -- runs on the host in tests/host/bank_readout_check.cpp, which this file compiles itself:
once plainly and once under the address and undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python).
The Breaks come from the library's host-only stitch (pkg.stitch, which needs no device); the program's rows must equal that
stitch's and Break.frequencies byte for byte, its band sums numpy's f64 sum of the same trapezoids within the summation bound."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdcr_bank_layout", "psdcr_bank_psd_device", "psdcr_bank_psd", "psdcr_release"]
BANDS = [(0.0, 0.5), (1e-3, 1e-2), (0.01, 0.2), (0.25, 0.25), (0.30001, 0.30002), (3e-7, 0.4)]  # whole, a decade, wide, one bin, none


@pytest.fixture(scope="session")
def bank_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bank_readout_host")


def cases(pkg):
    """[(what, n, counts (stage 0 first, 64 bits), MergeOpts)]"""
    out = []
    for n, ns in ((64, 1), (64, 3), (1024, 3), (64, 16), (1024, 16)):
        counts = [max(1, 40000 >> (3 * k)) + k for k in range(ns)]
        for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 1)):
            out.append((f"n={n} stages={ns} keep_overlap={ko} keep_transition_band={ktb} min_count={mc}", n, counts,
                        pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)))
    for n, ns in ((64, 3), (1024, 16)):
        deep = [900 - k for k in range(ns - 1)] + [3]
        mid = [900 - k for k in range(ns)]
        mid[ns // 2] = 3
        for ko in (False, True):
            out.append((f"n={n} stages={ns} keep_overlap={ko}: the deepest excluded", n, deep, pkg.MergeOpts(keep_overlap=ko, min_count=10)))
            out.append((f"n={n} stages={ns} keep_overlap={ko}: a middle stage excluded", n, mid, pkg.MergeOpts(keep_overlap=ko, min_count=10)))
            out.append((f"n={n} stages={ns} keep_overlap={ko}: every stage excluded", n, mid, pkg.MergeOpts(keep_overlap=ko, min_count=10 ** 6)))
    out.append(("counts at and above 2^32", 64, [2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 1, 7], pkg.MergeOpts()))
    out.append(("count 2^32 alone", 1024, [2 ** 32], pkg.MergeOpts(min_count=0)))
    out.append(("no stage", 64, [], pkg.MergeOpts()))
    return out


@pytest.fixture(scope="session")
def dump(pkg, bank_host_dir):
    """every case through the plain program once: [(what, psd, frequencies, bands f64, want psd, breaks)]"""
    rng = np.random.default_rng(20261020)
    wt = pkg.WindowTable.hann(64)
    blob, want = [], []
    cs = cases(pkg)
    for what, n, counts, opts in cs:
        ns = len(counts)
        spectra = np.exp(rng.normal(0.0, 3.0, (ns, n // 2 + 1))).astype(np.float32)
        psd, breaks = pkg.stitch(n, counts, [pkg.U32_MAX] * ns, [0] * ns, spectra, opts)
        assert len(breaks) == ns
        blob.append(struct.pack("<4I2f", n, ns, len(breaks), len(BANDS), wt.nenbw, wt.power))
        blob.append(np.asarray(counts, np.uint64).tobytes())
        blob += [bytes(b._c()) for b in breaks]
        blob.append(spectra.tobytes())
        blob.append(np.asarray(BANDS, np.float32).tobytes())
        want.append((psd, breaks))
    src, dst = (os.path.join(str(bank_host_dir), name) for name in ("cases.bin", "rows.bin"))
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cs)) + b"".join(blob))
    exe = host_exe(bank_host_dir, "bank_readout_check", False)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
    raw, pos, out = open(dst, "rb").read(), 0, []
    for (what, _, _, _), (psd, breaks) in zip(cs, want):
        L = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        got = [np.frombuffer(raw, np.float32, L, pos + 8), np.frombuffer(raw, np.float32, L, pos + 8 + 4 * L),
               np.frombuffer(raw, np.float64, len(BANDS), pos + 8 + 8 * L)]
        pos += 8 + 8 * L + 8 * len(BANDS)
        out.append((what, *got, psd, breaks))
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_bank_readout_check(pkg, bank_host_dir, dump, sanitize):
    """the program's own checks (every element of a row written exactly once, nothing else written, an excluded middle stage, an
    empty row), plainly and under ASan + UBSan; the sanitized program also runs every case of this file"""
    exe = host_exe(bank_host_dir, "bank_readout_check", sanitize)
    out = run_host(exe)
    assert int(re.search(r"bank_readout_check: (\d+) checks", out).group(1)) > 100
    if sanitize:
        src = os.path.join(str(bank_host_dir), "cases.bin")
        r = subprocess.run([exe, src, os.path.join(str(bank_host_dir), "rows_san.bin")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        assert open(os.path.join(str(bank_host_dir), "rows_san.bin"), "rb").read() == open(os.path.join(str(bank_host_dir), "rows.bin"), "rb").read()


def test_rows_and_frequencies_equal_the_stitch(pkg, dump):
    """byte for byte: 1, 3 and 16 stages, the three merge options on and off, a min_count that excludes the deepest, a middle and
    every stage, counts at and above 2^32"""
    seen = dict(empty=0, excluded=0, big=0)
    for what, psd, freq, _, want, breaks in dump:
        assert psd.tobytes() == want.tobytes(), what
        assert freq.tobytes() == pkg.Break.frequencies(breaks).tobytes(), what
        assert len(psd) == sum(len(b.bins) for b in breaks if b.include), what
        seen["empty"] += int(len(psd) == 0)
        seen["excluded"] += int(any(not b.include for b in breaks) and len(psd) > 0)
        seen["big"] += int("2^32" in what)
    assert all(seen.values()), seen


def band_reference(psd, freq, bands):
    """numpy's f64 sum of the trapezoids t_k of include/psdcascade_readout.h per band, and L * 2^-52 * sum |t_k| over the band"""
    p, f = psd.astype(np.float64), freq.astype(np.float64)
    t = 0.5 * (p + np.concatenate(([0.0], p[:-1]))) * (f - np.concatenate(([0.0], f[:-1])))
    out = []
    for lo, hi in np.asarray(bands, np.float32):
        m = (freq >= lo) & (freq <= hi)  # compared in f32
        out.append((float(np.sum(t[m])), len(psd) * 2.0 ** -52 * float(np.sum(np.abs(t[m]))), int(m.sum())))
    return out


def test_band_sums(pkg, dump):
    """each band within L * 2^-52 * sum |t_k| of numpy's f64 sum of the same t_k (both sums carry at most L * 2^-53 of sum |t_k|)"""
    held = np.zeros(len(BANDS), int)
    for what, psd, freq, bands, _, _ in dump:
        for b, (want, tol, count) in enumerate(band_reference(psd, freq, BANDS)):
            assert abs(bands[b] - want) <= tol, (what, b, bands[b], want, tol)
            if count == 0:
                assert bands[b] == 0.0
            held[b] = max(held[b], count)
    assert held[3] == 1 and held[4] == 0 and held[0] > 1000, held  # one bin, none, the whole range


def test_exports(pkg):
    """include/psdcascade_readout.h declares exactly the psdcr_ entry points and the library exports exactly those; each returns
    ERR_ARG with a text on a NULL handle; psdcascade.h and its ABI version are unchanged"""
    hdr = open(os.path.join(ROOT, "include", "psdcascade_readout.h")).read()
    assert set(re.findall(r"\b(psdcr_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdcr_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdcr_")]
    assert '#include "psdcascade.h"' in hdr and re.search(r"#define\s+PSDCR_MAX_BANDS\s+8u", hdr)
    assert "psdcr_" not in open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    assert pkg.lib().psdc_abi_version() == 3
    from stabilizer_stream_amd import bankread
    L = bankread._lib()
    lens = np.full(4, 77, np.uintp)
    buf = np.zeros(64, np.float32)
    info = bankread._CInfo()
    tail = (lens.ctypes.data, None, None, 0, C.byref(info))
    calls = {"psdcr_bank_layout": (None, None, 0, 0, 1, 0, *tail),
             "psdcr_bank_psd_device": (None, None, 0, 0, 1, 0, buf.ctypes.data, None, 64, None, 0, None, None, *tail),
             "psdcr_bank_psd": (None, None, 0, 0, 1, 0, buf.ctypes.data, None, 64, None, 0, None, *tail),
             "psdcr_release": (None,)}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == pkg.ERR_ARG, name
        assert pkg.lib().psdc_last_error(None).decode() == name + ": null handle"
    assert np.all(lens == 77) and np.all(buf == 0)
    assert bankread.MAX_BANDS == 8
    for cls in ("PsdCascadeBank", "PsdCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "bank_psd" in m or "layout" in m]
    with pytest.raises(pkg.PsdError) as e:
        bankread.layout(object())
    assert e.value.code == pkg.ERR_ARG
