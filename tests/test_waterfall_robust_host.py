"""Robust waterfall read-outs (include/psdcascade_robust.h, psdcx_*; stabilizer-stream_amd/robust.py): the parts that run without
a GPU.

csrc/waterfall_robust.h -- what one thread of wf_robust_kernel computes for one (side, bin) -- runs on the host in
tests/host/waterfall_robust_emul.cpp, which this file compiles itself: once plainly and once under the address and
undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python).  The program compares every output bit for
bit with a sort-based restatement and dumps the considered rows and the outputs; the dump is compared with numpy here."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdcx_wf_robust", "psdcx_wf_robust_device", "psdcx_zwf_robust", "psdcx_zwf_robust_device"]


@pytest.fixture(scope="session")
def robust(pkg):
    from stabilizer_stream_amd import robust as mod
    return mod


@pytest.fixture(scope="session")
def robust_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("waterfall_robust_host")


CASES = (["unwrapped partial", "unwrapped complete", "wrapped partial", "wrapped complete", "max_rows 5 of 12", "max_rows 6 of 11",
          "max_rows 0", "first block partial", "nothing yet", "depth 1 partial", "depth 1 complete", "all equal odd", "all equal even",
          "all zero", "nan row odd", "nan row even", "inf row odd", "inf row even", "inf row R=2", "limits -inf..1", "limits 1..inf",
          "limits -inf..inf", "limits empty", "past 2^32 blocks"] +
         [f"R={r} {what}" for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64) for what in ("unwrapped", "wrapped partial", "ties")])


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_robust_emulation(robust_host_dir, sanitize):
    """csrc/waterfall_robust.h against the sort-based restatement of tests/host/waterfall_robust_emul.cpp, bit for bit: R = 1 ... 9
    and 64, a ring before and after it wraps with the partial newest block present and absent, ties, zeros, a NaN row, a +inf row,
    infinite limits (the program asserts)"""
    out = run_host(host_exe(robust_host_dir, "waterfall_robust_emul", sanitize))
    for name in CASES:
        assert f"case {name}: " in out, name
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"case (.*?): .* -> R=(\d+)", out)}
    for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64):
        for what in ("unwrapped", "wrapped partial", "ties"):
            assert rows[f"R={r} {what}"] == r
    assert rows["unwrapped partial"] == 6 and rows["unwrapped complete"] == 7      # the partial newest block is left out
    assert rows["wrapped partial"] == 11 and rows["wrapped complete"] == 12
    assert rows["max_rows 5 of 12"] == 5 and rows["max_rows 6 of 11"] == 6 and rows["max_rows 0"] == 0
    assert rows["first block partial"] == 0 and rows["nothing yet"] == 0 and rows["depth 1 partial"] == 0 and rows["depth 1 complete"] == 1
    assert int(re.search(r"waterfall_robust_emul: (\d+) checks", out).group(1)) > 10_000


def read_dump(path):
    """the records of waterfall_robust_emul's dump: dict(R, B, g, lo, hi, V, W [R][elements] f64, and with R > 0 median, min, max,
    excised f32 and kept u32 [elements])"""
    raw = open(path, "rb").read()
    pos, out = 0, []

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count, pos)
        pos += a.nbytes
        return a

    while pos < len(raw):
        R, ne, B, _ = (int(v) for v in take(np.uint32, 4))
        g, lo, hi = (float(v) for v in take(np.float64, 3))
        rec = dict(R=R, B=B, g=g, lo=lo, hi=hi, V=take(np.float64, R * ne).reshape(R, ne), W=take(np.float64, R * ne).reshape(R, ne))
        if R:
            for name in ("median", "min", "max", "excised"):
                rec[name] = take(np.float32, ne)
            rec["kept"] = take(np.uint32, ne)
        out.append(rec)
    assert pos == len(raw)
    return out


def same_f32(got, want):
    """equal bytes, a NaN equal to any NaN"""
    want = np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def numpy_robust(pkg, V, W, B, g, lo, hi):
    """the semantics of include/psdcascade_robust.h in numpy over rows V, W [R][...]: (median, min, max, excised, kept)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = np.float64(g)
        med, mn, mx = (f(V, axis=0) for f in (np.median, np.min, np.max))  # (each is NaN where a row is)
        sk = pkg.sk_from_moments(B, V, W)
        keep = ~np.isnan(sk) & (sk >= lo) & (sk <= hi)
        acc, kept = np.zeros(V.shape[1:], np.float64), np.zeros(V.shape[1:], np.uint32)
        for r in range(V.shape[0]):  # oldest first, one add a row
            acc = np.where(keep[r], acc + np.where(keep[r], V[r], 0.0), acc)
            kept += keep[r].astype(np.uint32)
        exc = np.where(kept > 0, acc / np.maximum(kept, 1).astype(np.float64) * g, np.nan)
        return (med * g).astype(np.float32), (mn * g).astype(np.float32), (mx * g).astype(np.float32), exc.astype(np.float32), kept


def test_emulation_dump_against_numpy(pkg, robust_host_dir):
    """the arrays the program dumps, against numpy: np.median, np.min, np.max of the considered rows times g, rounded to f32 once;
    the excised mean from a row-by-row acc += row over the kept rows; byte for byte"""
    exe = host_exe(robust_host_dir, "waterfall_robust_emul", False)
    path = os.path.join(str(robust_host_dir), "dump.bin")
    subprocess.run([exe, path], check=True, capture_output=True, timeout=600)
    recs = read_dump(path)
    assert len(recs) == len(CASES)
    seen = dict(nan=0, inf=0, zero=0, excised_nan=0, even=0, odd=0)
    for i, rec in enumerate(recs):
        if not rec["R"]:
            continue
        med, mn, mx, exc, kept = numpy_robust(pkg, rec["V"], rec["W"], rec["B"], rec["g"], rec["lo"], rec["hi"])
        for name, want in (("median", med), ("min", mn), ("max", mx), ("excised", exc)):
            assert same_f32(rec[name], want), (i, name)
        assert np.array_equal(rec["kept"], kept), i
        seen["nan"] += int(np.isnan(rec["V"]).any())
        seen["inf"] += int(np.isinf(rec["V"]).any())
        seen["zero"] += int(np.all(rec["V"] == 0))
        seen["excised_nan"] += int(np.isnan(rec["excised"]).any())
        seen["even" if rec["R"] % 2 == 0 else "odd"] += 1
    print(seen)
    assert all(seen.values()), seen


def test_robust_exports(pkg):
    """include/psdcascade_robust.h declares exactly the four psdcx_ functions and the library exports exactly those; psdcascade.h is
    the committed one; each returns ERR_ARG on a NULL handle with a text through last_error"""
    hdr = open(os.path.join(ROOT, "include", "psdcascade_robust.h")).read()
    assert set(re.findall(r"\b(psdcx_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdcx_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdcx_")]  # the recorded surface is psdcascade.h's
    assert '#include "psdcascade.h"' in hdr and re.search(r"#define\s+PSDCX_ROBUST_MAX_ROWS\s+4096u", hdr)
    flat = " ".join(hdr.replace(" * ", " ").split())
    for text in ("newest R COMPLETE blocks", "0.5 (v_(R/2-1) + v_(R/2))", "sk_lo <= sk_r <= sk_hi", "exactly one kernel launch",
                 "Out of scope: partial blocks", "no weights", "no other object", "more than PSDCX_ROBUST_MAX_ROWS = 4096 rows"):
        assert text in flat, text
    try:  # (where the tree is a git checkout that git will read)
        d = subprocess.run(["git", "-C", ROOT, "diff", "HEAD", "--", "include/psdcascade.h"], capture_output=True, text=True)
    except OSError:
        d = None
    if d is not None and d.returncode == 0:
        assert d.stdout == "", d.stdout[:500]
    assert pkg.lib().psdc_abi_version() == 3 and "psdcx_" not in open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    from stabilizer_stream_amd import robust as mod
    L = mod._lib()
    info = mod._CRobustInfo()
    buf = np.zeros(64, np.float32)
    for s in SYMBOLS:
        rc = getattr(L, s)(None, 0, 0, 4, 0.0, 2.0, buf.ctypes.data, None, None, None, None, C.byref(info))
        assert rc == pkg.ERR_ARG, s
        last = L.psdc_zwf_last_error if "zwf" in s else L.psdc_wf_last_error
        assert last(None).decode() == s + ": null handle"
    assert np.all(buf == 0)


def test_robust_helpers(pkg, robust):
    """robust.sk_limits and robust.median_to_mean against their formulas; the module adds no method to the classes"""
    for block in (2, 8, 64, 1000):
        s = 2.0 / math.sqrt(block)
        assert s == pkg.sk_sigma(block)
        assert robust.sk_limits(block) == (1.0 - 3.0 * s, 1.0 + 3.0 * s)
        assert robust.sk_limits(block, nsigma=4.5) == (1.0 - 4.5 * s, 1.0 + 4.5 * s)
        assert robust.median_to_mean(block) == 1.0 / (1.0 - 1.0 / (9.0 * block)) ** 3
    # Wilson-Hilferty against the asymptotic series of the gamma median, k - 1/3 + 8 / (405 k): the two differ in the 1 / k^2 terms
    # (3e-4 at k = 8, where the tabulated median of chi-square 16 gives 7.6692), so 5e-4 from k = 8 on
    for block in (8, 64, 1000):
        assert abs(robust.median_to_mean(block) - block / (block - 1.0 / 3.0 + 8.0 / (405.0 * block))) < 5e-4
        assert robust.median_to_mean(block) > 1.0
    assert "independent" in robust.median_to_mean.__doc__.lower() and "approximation" in robust.median_to_mean.__doc__
    assert robust.MAX_ROWS == 4096
    for cls in ("WaterfallCascadeBank", "WaterfallCascade", "ZoomWaterfallCascadeBank", "ZoomWaterfallCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "robust" in m]
    with pytest.raises(pkg.PsdError) as e:
        robust.stage_robust(object(), 0)
    assert e.value.code == pkg.ERR_ARG
