"""Bank read-out of the pair and matrix objects (include/psdcascade_crossread.h, psdcxr_*; stabilizer-stream_amd/crossread.py): the
parts that run without a GPU.

csrc/cross_readout.h -- the job table made from Break lists, what one thread of cross_stitch_kernel computes for one bin (the pair
form with coherence and H1, the matrix form with m * m rows), what cross_band_kernel adds up for one pair and the argument rules
that need no object -- runs on the host in tests/host/cross_readout_check.cpp, which this file compiles itself: once plainly and
once under the address and undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python).  The Breaks come
from the library's host-only stitch (pkg.stitch, which needs no device) of the f32-cast accumulator rows; the program's rows must
equal that stitch's and Break.frequencies byte for byte, coherence and H1 a numpy f64 restatement byte for byte, its band sums
numpy's f64 sum of the same trapezoids within the summation bound of tests/test_bank_readout_host.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_bank_readout_host import BANDS, band_reference, cases
from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdcxr_cross_layout", "psdcxr_cross_csd_device", "psdcxr_cross_csd", "psdcxr_cross_release",
           "psdcxr_csm_layout", "psdcxr_csm_rows_device", "psdcxr_csm_rows", "psdcxr_csm_release"]
ROWS = (4, 9, 16)  # a pair (and m = 2), m = 3, m = 4


@pytest.fixture(scope="session")
def cross_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("cross_readout_host")


def accumulators(rng, ns, rows, bins):
    """f64 accumulators [ns][rows][bins] that do not fit f32; of a pair (rows == 4): xx, yy > 0, re and im of either sign, with a
    zero xx, a zero yy and a zero of both in every stage"""
    acc = np.exp(rng.normal(0.0, 3.0, (ns, rows, bins)))
    if rows == 4:
        acc[:, 2:] = rng.normal(0.0, 1.0, (ns, 2, bins)) * np.sqrt(acc[:, 0:1] * acc[:, 1:2])
        acc[:, 0, 5::11] = 0.0
        acc[:, 1, 7::13] = 0.0
        acc[:, :2, 9::17] = 0.0
    else:
        acc *= rng.choice([-1.0, 1.0], acc.shape)
    return acc


@pytest.fixture(scope="session")
def dump(pkg, cross_host_dir):
    """every case of tests/test_bank_readout_host.py with 4, 9 and 16 rows through the plain program once:
    [dict(what, rows, acc, want rows, breaks, got rows, frequencies, and for a pair coherence, transfer, bands)]"""
    rng = np.random.default_rng(20261021)
    wt = pkg.WindowTable.hann(64)
    blob, out = [], []
    for what, n, counts, opts in cases(pkg):
        for rows in ROWS:
            ns, bins = len(counts), n // 2 + 1
            acc = accumulators(rng, ns, rows, bins)
            f32 = acc.astype(np.float32)
            stitched = [pkg.stitch(n, counts, [pkg.U32_MAX] * ns, [0] * ns, np.ascontiguousarray(f32[:, r]), opts) for r in range(rows)]
            breaks = stitched[0][1]
            assert len(breaks) == ns and all(br == breaks for _, br in stitched)
            blob.append(struct.pack("<5I2f", n, ns, len(breaks), len(BANDS), rows, wt.nenbw, wt.power))
            blob.append(np.asarray(counts, np.uint64).tobytes())
            blob += [bytes(b._c()) for b in breaks]
            blob.append(acc.tobytes())
            blob.append(np.asarray(BANDS, np.float32).tobytes())
            out.append(dict(what=f"{what} rows={rows}", rows=rows, acc=acc, want=[p for p, _ in stitched], breaks=breaks))
    src, dst = (os.path.join(str(cross_host_dir), name) for name in ("cases.bin", "rows.bin"))
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(blob))
    exe = host_exe(cross_host_dir, "cross_readout_check", False)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
    raw, pos = open(dst, "rb").read(), 0
    for d in out:
        L = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        pos += 8
        d["got"] = np.frombuffer(raw, np.float32, d["rows"] * L, pos).reshape(d["rows"], L)
        d["freq"] = np.frombuffer(raw, np.float32, L, pos + 4 * d["rows"] * L)
        pos += 4 * (d["rows"] + 1) * L
        if d["rows"] == 4:
            d["coherence"] = np.frombuffer(raw, np.float64, L, pos)
            d["transfer"] = np.frombuffer(raw, np.float64, 2 * L, pos + 8 * L).reshape(L, 2)
            d["bands"] = np.frombuffer(raw, np.float64, 4 * len(BANDS), pos + 24 * L).reshape(len(BANDS), 4)
            pos += 24 * L + 32 * len(BANDS)
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_cross_readout_check(pkg, cross_host_dir, dump, sanitize):
    """the program's own checks (every element of every output written exactly once and nothing else, y = 2 x with its NaN paths,
    an excluded middle stage, an empty unit, m = 2, 3, 4, the argument rules), plainly and under ASan + UBSan; the sanitized
    program also runs every case of this file and must write the same bytes, band sums included"""
    exe = host_exe(cross_host_dir, "cross_readout_check", sanitize)
    out = run_host(exe)
    assert int(re.search(r"cross_readout_check: (\d+) checks", out).group(1)) > 1000
    if sanitize:
        src, dst = (os.path.join(str(cross_host_dir), name) for name in ("cases.bin", "rows_san.bin"))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        assert open(dst, "rb").read() == open(os.path.join(str(cross_host_dir), "rows.bin"), "rb").read()


def test_rows_and_frequencies_equal_the_stitch(pkg, dump):
    """byte for byte, four rows of a pair and m * m rows for m = 2, 3, 4: 1, 3 and 16 stages, the three merge options on and off, a
    min_count that excludes the deepest, a middle and every stage, counts at and above 2^32, no stage"""
    seen = dict(empty=0, excluded=0, big=0, none=0)
    for d in dump:
        for r in range(d["rows"]):
            assert d["got"][r].tobytes() == d["want"][r].tobytes(), (d["what"], r)
        assert d["freq"].tobytes() == pkg.Break.frequencies(d["breaks"]).tobytes(), d["what"]
        assert len(d["freq"]) == sum(len(b.bins) for b in d["breaks"] if b.include), d["what"]
        seen["empty"] += int(len(d["freq"]) == 0)
        seen["excluded"] += int(any(not b.include for b in d["breaks"]) and len(d["freq"]) > 0)
        seen["big"] += int("2^32" in d["what"])
        seen["none"] += int(not d["breaks"])
    assert all(seen.values()), seen


def placed(acc, breaks):
    """the f64 accumulators [ns][rows][bins] laid along the stitched row by the Breaks (deepest stage first): [rows][L]"""
    parts = [acc[len(breaks) - 1 - i][:, b.bins.start:b.bins.stop] for i, b in enumerate(breaks) if b.include]
    return np.concatenate(parts, axis=1) if parts else np.zeros((acc.shape[1], 0))


def test_coherence_and_h1_equal_the_f64_restatement(pkg, dump):
    """den = xx yy; coherence = den != 0 ? (re re + im im) / den : NaN; transfer = xx != 0 ? (re / xx, im / xx) : NaN, in numpy
    f64 on the same accumulators, byte for byte; NaN at the zeros of xx and of xx yy"""
    nans = np.zeros(2, int)
    for d in dump:
        if d["rows"] != 4:
            continue
        xx, yy, re_, im = placed(d["acc"], d["breaks"])
        den = xx * yy
        with np.errstate(divide="ignore", invalid="ignore"):
            coh = np.where(den != 0, (re_ * re_ + im * im) / den, np.nan)
            tr = np.stack([np.where(xx != 0, re_ / xx, np.nan), np.where(xx != 0, im / xx, np.nan)], axis=1)
        assert d["coherence"].tobytes() == coh.tobytes(), d["what"]
        assert d["transfer"].tobytes() == tr.tobytes(), d["what"]
        assert np.array_equal(np.isnan(d["coherence"]), (xx == 0) | (yy == 0)) and np.array_equal(np.isnan(d["transfer"][:, 0]), xx == 0)
        nans += [int(np.sum((yy == 0) & (xx != 0))), int(np.sum(xx == 0))]
    assert np.all(nans > 10), nans  # coherence NaN with H1 finite, and both NaN


def test_band_sums(pkg, dump):
    """each of the four sums of a band within L * 2^-52 * sum |t_k| of numpy's f64 sum of the same t_k on the stitched f32 row
    (p negative for re / im)"""
    held = np.zeros(len(BANDS), int)
    negative = 0
    for d in dump:
        if d["rows"] != 4:
            continue
        for r in range(4):
            for b, (want, tol, count) in enumerate(band_reference(d["got"][r], d["freq"], BANDS)):
                assert abs(d["bands"][b, r] - want) <= tol, (d["what"], r, b, d["bands"][b, r], want, tol)
                if count == 0:
                    assert d["bands"][b, r] == 0.0
                held[b] = max(held[b], count)
                negative += int(want < 0)
    assert held[3] == 1 and held[4] == 0 and held[0] > 1000 and negative > 10, (held, negative)


def test_exports(pkg):
    """include/psdcascade_crossread.h declares exactly the eight psdcxr_ entry points, compiles as plain C, and the library
    exports exactly those; each returns ERR_ARG with a text on a NULL handle; the other headers, EXPORTS and the ABI version are
    unchanged; crossread adds nothing to the classes"""
    inc = os.path.join(ROOT, "include")
    hdr = open(os.path.join(inc, "psdcascade_crossread.h")).read()
    assert sorted(set(re.findall(r"\b(psdcxr_[a-z0-9_]+)\s*\(", hdr))) == sorted(SYMBOLS)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "psdcascade_crossread.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdcxr_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdcxr_")]
    assert '#include "psdcascade.h"' in hdr and re.search(r"#define\s+PSDCXR_MAX_BANDS\s+8u", hdr) and re.search(r"#define\s+PSDCXR_MAX_ROWS\s+65536u", hdr)
    for other in ("psdcascade.h", "psdcascade_readout.h", "psdcascade_robust.h"):
        assert "psdcxr_" not in open(os.path.join(inc, other)).read()
    assert pkg.lib().psdc_abi_version() == 3
    from stabilizer_stream_amd import crossread
    L = crossread._lib()
    lens = np.full(4, 77, np.uintp)
    buf = np.zeros(64, np.float32)
    info = crossread._CInfo()
    tail = (lens.ctypes.data, None, None, 0, C.byref(info))
    head = (None, None, 0, 0, 1, 0)
    calls = {"psdcxr_cross_layout": (*head, *tail),
             "psdcxr_cross_csd_device": (*head, buf.ctypes.data, None, None, None, None, None, 64, None, 0, None, None, *tail),
             "psdcxr_cross_csd": (*head, buf.ctypes.data, None, None, None, None, None, 64, None, 0, None, *tail),
             "psdcxr_cross_release": (None,),
             "psdcxr_csm_layout": (*head, *tail),
             "psdcxr_csm_rows_device": (*head, buf.ctypes.data, None, 64, None, *tail),
             "psdcxr_csm_rows": (*head, buf.ctypes.data, None, 64, *tail),
             "psdcxr_csm_release": (None,)}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == pkg.ERR_ARG, name
        assert pkg.lib().psdc_cross_last_error(None).decode() == name + ": null handle"
    assert np.all(lens == 77) and np.all(buf == 0)
    assert crossread.MAX_BANDS == 8
    for cls in ("CsdCascadeBank", "CsdCascade", "CsmCascadeBank", "CsmCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "bank_" in m or "layout" in m]
    for fn in (crossread.layout, crossread.bank_csd, crossread.bank_rows, crossread.release):
        with pytest.raises(pkg.PsdError) as e:
            fn(object())
        assert e.value.code == pkg.ERR_ARG


def test_band_coherence_and_transfer():
    """the two formulas on the four sums of a band"""
    from stabilizer_stream_amd import crossread
    s = np.array([[[2.0, 8.0, 4.0, 0.0], [2.0, 4.0, 0.0, -2.0]], [[0.0, 1.0, 0.0, 0.0], [3.0, 0.0, 1.0, 1.0]]])
    coh, tr = crossread.band_coherence(s), crossread.band_transfer(s)
    assert coh.shape == (2, 2) and coh[0, 0] == 1.0 and coh[0, 1] == 0.5 and np.isnan(coh[1, 0]) and np.isnan(coh[1, 1])
    assert tr[0, 0] == 2.0 and tr[0, 1] == -1.0j and np.isnan(tr[1, 0]) and tr[1, 1] == (1.0 + 1.0j) / 3.0
