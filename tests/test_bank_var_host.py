"""Var read-out (include/psdcascade_var.h, psdcv_*; stabilizer-stream_amd/bankvar.py): the parts that run without a GPU.

csrc/bank_var.h -- the limit search, the exact fold, the terms and the sum in bank_var_kernel's order -- runs on the host in
tests/host/bank_var_check.cpp, which this file compiles itself: once plainly and once under the address and undefined-behaviour
sanitizers (a stand-alone program; nothing is loaded into Python).  The Breaks come from the library's host-only stitch
(pkg.stitch, which needs no device); the program's results are held to the numpy f64 restatement of the definition
(tests/bank_var_ref.py) within (L + 64) 2^-52 sum |t|."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bank_var_ref as ref
from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdcv_bank_var_device", "psdcv_bank_var", "psdcv_rows_var_device"]
TAUS = np.concatenate(([0.5, 2.7, 3e7], np.logspace(0, 6, 61))).astype(np.float32)  # lim = inf, every stage cut, no term at all
VARS = [ref.AVAR, ref.MVAR, ref.FVAR, dict(ref.AVAR, dc_cut=1)]


@pytest.fixture(scope="session")
def var_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bank_var_host")


def cases(pkg):
    """[(what, n, counts (stage 0 first), MergeOpts, vars)]; a dc_cut of ("L", k) stands for the row's length + k"""
    out = []
    for n, ns in ((64, 1), (64, 4), (64, 16), (1024, 3)):
        counts = [max(1, 40000 >> (3 * k)) + k for k in range(ns)]
        for ko, ktb in ((False, False), (True, False), (True, True)):
            out.append((f"n={n} stages={ns} keep_overlap={ko} keep_transition_band={ktb}", n, counts,
                        pkg.MergeOpts(keep_overlap=ko, min_count=1, keep_transition_band=ktb), VARS))
    mid = [900, 899, 3, 897]
    out.append(("a middle stage excluded", 64, mid, pkg.MergeOpts(min_count=10), VARS[:3]))
    out.append(("every stage excluded", 64, mid, pkg.MergeOpts(min_count=10 ** 6), VARS[:2]))
    out.append(("no stage", 64, [], pkg.MergeOpts(), VARS[:1]))
    out.append(("dc_cut 0, at and behind the end", 64, [500, 60], pkg.MergeOpts(),
                [dict(ref.AVAR, dc_cut=0), dict(ref.MVAR, dc_cut=("L", 0)), dict(ref.FVAR, dc_cut=("L", 5)), dict(ref.AVAR, dc_cut=("L", -1))]))
    return out


@pytest.fixture(scope="session")
def dump(pkg, var_host_dir):
    """every case through the plain program once: [(what, psd, frequencies, var f64 [V][T], vars, want psd, breaks)]"""
    rng = np.random.default_rng(20261021)
    wt = pkg.WindowTable.hann(64)
    blob, want = [], []
    cs = cases(pkg)
    for what, n, counts, opts, vs in cs:
        ns = len(counts)
        spectra = np.exp(rng.normal(0.0, 3.0, (ns, n // 2 + 1))).astype(np.float32)
        psd, breaks = pkg.stitch(n, counts, [pkg.U32_MAX] * ns, [0] * ns, spectra, opts)
        vs = [dict(v, dc_cut=len(psd) + v["dc_cut"][1]) if isinstance(v["dc_cut"], tuple) else v for v in vs]
        blob.append(struct.pack("<6I2f", n, ns, len(breaks), len(vs), len(TAUS), 0, wt.nenbw, wt.power))
        blob.append(np.asarray(counts, np.uint64).tobytes())
        blob += [bytes(b._c()) for b in breaks]
        blob.append(spectra.tobytes())
        blob += [struct.pack("<2ifI", v["x_exp"], v["sinx_exp"], v["clip"], v["dc_cut"]) for v in vs]
        blob.append(TAUS.tobytes())
        want.append((psd, breaks, vs))
    src, dst = (os.path.join(str(var_host_dir), name) for name in ("cases.bin", "vars.bin"))
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cs)) + b"".join(blob))
    exe = host_exe(var_host_dir, "bank_var_check", False)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
    raw, pos, out = open(dst, "rb").read(), 0, []
    for (what, _, _, _, _), (psd, breaks, vs) in zip(cs, want):
        L = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        count = len(vs) * len(TAUS)
        out.append((what, np.frombuffer(raw, np.float32, L, pos + 8), np.frombuffer(raw, np.float32, L, pos + 8 + 4 * L),
                    np.frombuffer(raw, np.float64, count, pos + 8 + 8 * L).reshape(len(vs), len(TAUS)), vs, psd, breaks))
        pos += 8 + 8 * L + 8 * count
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_bank_var_check(pkg, var_host_dir, dump, sanitize):
    """the program's own checks -- every element of [dc_cut, E) once for L below, at and beside multiples of 256 (exact sums); E at
    dc_cut, inside the first job, on a seam and at L; a keep_overlap row whose f steps back; dc_cut >= L; an empty row; the fold
    against fmod -- plainly and under ASan + UBSan; the sanitized program also runs every case of this file, with the same bytes"""
    exe = host_exe(var_host_dir, "bank_var_check", sanitize)
    out = run_host(exe)
    assert int(re.search(r"bank_var_check: (\d+) checks", out).group(1)) > 100000
    if sanitize:
        src = os.path.join(str(var_host_dir), "cases.bin")
        r = subprocess.run([exe, src, os.path.join(str(var_host_dir), "vars_san.bin")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        assert open(os.path.join(str(var_host_dir), "vars_san.bin"), "rb").read() == open(os.path.join(str(var_host_dir), "vars.bin"), "rb").read()


def test_restatement_on_the_reference_vector():
    """0.134782674 within 1e-9, and within 1e-5 of the reference's f32 result 0.13478442 (a condition on the restatement: the gap
    of 1.75e-6 is the f32 rounding of pi f tau = 76.3 at f = 9)"""
    got, sum_abs, E = ref.var_ref(ref.REF_P, ref.REF_F, ref.REF_TAU)
    assert E == 5 and abs(got - ref.REF_F64) <= 1e-9 and abs(got - ref.REF_F32) <= 1e-5, got
    assert ref.var_ref(ref.REF_P, ref.REF_F, ref.REF_TAU, **ref.FVAR)[2] == 2  # clip / tau = 0.37 < f[2]
    assert ref.var_ref(ref.REF_P, ref.REF_F, ref.REF_TAU, **dict(ref.AVAR, dc_cut=7)) == (0.0, 0.0, 5)
    assert np.isnan(ref.var_ref(ref.REF_P, ref.REF_F, ref.REF_TAU, **dict(ref.AVAR, dc_cut=0))[0])


def test_var_eval_is_the_f32_side(pkg):
    """psdc_var_eval is unchanged: the reference's f32 value on its own vector"""
    got = pkg.var_eval(np.asarray(ref.REF_P, np.float32), np.asarray(ref.REF_F, np.float32), ref.REF_TAU)
    assert abs(got - ref.REF_F32) <= 2e-7 * ref.REF_F32, got


def test_rows_equal_the_stitch(pkg, dump):
    for what, psd, freq, _, _, want, breaks in dump:
        assert psd.tobytes() == want.tobytes(), what
        assert freq.tobytes() == pkg.Break.frequencies(breaks).tobytes(), what


def test_results_against_the_restatement(dump):
    """every case, descriptor and tau within (L + 64) 2^-52 sum |t| of numpy's f64 sum; NaN exactly where numpy gives NaN"""
    seen = dict(nan=0, empty=0, cut=0, whole=0, stepped_back=0)
    worst = 0.0
    for what, psd, freq, got, vs, _, _ in dump:
        seen["stepped_back"] += int(len(freq) > 1 and bool(np.any(np.diff(freq) < 0)))
        for v, var in enumerate(vs):
            for j, tau in enumerate(TAUS):
                worst = max(worst, ref.check(got[v, j], psd, freq, tau, var, (what, var, float(tau))))
                E = ref.limit(freq, tau, var["clip"], var["dc_cut"])
                seen["nan"] += int(np.isnan(got[v, j]))
                if E <= var["dc_cut"] or len(psd) == 0:
                    assert got[v, j] == 0.0, (what, var, tau)
                    seen["empty"] += 1
                elif E < len(psd):
                    seen["cut"] += 1
                else:
                    seen["whole"] += 1
    print("largest |error| / tolerance", worst, seen)
    assert all(seen.values()), seen


def test_exports(pkg):
    """include/psdcascade_var.h declares exactly the psdcv_ entry points and the library exports exactly those; each returns ERR_ARG
    with a text on a NULL handle; psdcascade.h, its ABI version and the package's EXPORTS are unchanged"""
    hdr = open(os.path.join(ROOT, "include", "psdcascade_var.h")).read()
    assert set(re.findall(r"\b(psdcv_[a-z0-9_]+)\s*\(", hdr)) == set(SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdcv_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdcv_")]
    assert '#include "psdcascade_readout.h"' in hdr and re.search(r"#define\s+PSDCV_MAX_VARS\s+4u", hdr)
    assert re.search(r"#define\s+PSDCV_MAX_TAUS\s+4096u", hdr) and re.search(r"#define\s+PSDCV_MAX_EXP\s+16\b", hdr)
    assert "psdcv_" not in open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    assert "psdcascade_var.h" in open(os.path.join(ROOT, "include", "psdcascade_readout.h")).read()
    assert pkg.lib().psdc_abi_version() == 3
    from stabilizer_stream_amd import bankread, bankvar
    L = bankvar._lib()
    lens = np.full(4, 77, np.uintp)
    out64 = np.zeros(8, np.float64)
    rec, nv, taus, nt, single = bankvar._what(None, [1.0, 2.0])
    assert single and nv == 1 and nt == 2 and rec[0].tolist() == (-2, 4, np.float32(bankvar.FLT_MAX), 2)
    info = bankread._CInfo()
    what = (rec.ctypes.data, nv, taus.ctypes.data, nt)
    tail = (lens.ctypes.data, None, None, 0, C.byref(info))
    calls = {"psdcv_bank_var_device": (None, None, 0, 0, 1, 0, *what, out64.ctypes.data, None, *tail),
             "psdcv_bank_var": (None, None, 0, 0, 1, 0, *what, out64.ctypes.data, *tail),
             "psdcv_rows_var_device": (None, out64.ctypes.data, out64.ctypes.data, 4, lens.ctypes.data, 1, *what, out64.ctypes.data, None,
                                       C.byref(info))}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == pkg.ERR_ARG, name
        assert pkg.lib().psdc_last_error(None).decode() == name + ": null handle"
    assert np.all(lens == 77) and np.all(out64 == 0)
    assert (bankvar.MAX_VARS, bankvar.MAX_TAUS, bankvar.MAX_EXP) == (4, 4096, 16)
    assert bankvar.Var() == bankvar.Var.avar() == bankvar.Var(-2, 4, bankvar.FLT_MAX, 2)
    assert bankvar.Var.mvar() == bankvar.Var(-4, 6, bankvar.FLT_MAX, 2) and bankvar.Var.fvar(dc_cut=3) == bankvar.Var(-2, 4, 1.0, 3)
    with pytest.raises(Exception):
        bankvar.Var().dc_cut = 3  # frozen
    for cls in ("PsdCascadeBank", "PsdCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "bank_var" in m or "rows_var" in m]
    with pytest.raises(pkg.PsdError) as e:
        bankvar.bank_var(object(), [1.0])
    assert e.value.code == pkg.ERR_ARG


def test_verify_target_covers_the_kernel():
    mk = open(os.path.join(ROOT, "stabilizer-stream_amd", "csrc", "Makefile")).read()
    verify = re.search(r"^verify:.*$", mk, re.M).group(0)
    assert "bank_var.hip" in verify and re.search(r"\$\(VERIFY_DIR\)/bank_var\.vfy:.*\n.*\n.*\$\(BANK_FLAGS\)", mk)
    assert re.search(r"bank_var_k\.o:.*\n.*\$\(BANK_FLAGS\)", mk)
