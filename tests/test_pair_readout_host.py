"""Bank read-out of the zoom cross, IQ cross and zoom / IQ AM/PM cross objects (include/ext/psdcascade_pairread.h, psdcpr_*;
stabilizer-stream_amd/pairread.py): the parts that run without a GPU.

csrc/pair_readout.h -- the job and unit tables made from Break lists, what one thread of pair_stitch_kernel<MODE> computes for one
bin (the six f32 sides, coherence and H1 a side, cab / cba, the AM/PM cross split with the carriers from bin 0 of stage 0 or
given), the carrier records, what pair_band_kernel adds up for one pair and the argument rules that need no object -- runs on the
host in tests/host/pair_readout_check.cpp, which this file compiles itself: once plainly and once under the address and
undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python).  The cases are synthetic 8- and 12-row f64
accumulators of 1, 3 and 16 stages; the Breaks come from the library's host-only stitch (pkg.stitch).  Every output must equal
tests/pair_read_ref.py byte for byte (g++ on x86-64 without -march does not fuse); the f32 sides and the frequencies also equal that
stitch's and Break.frequencies; the band sums equal the restated order bit for bit and are close to np.trapz."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pair_read_ref as ref
from test_bank_readout_host import BANDS, band_reference, cases
from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdcpr_layout", "psdcpr_csd_device", "psdcpr_csd", "psdcpr_ampm_device", "psdcpr_ampm", "psdcpr_release"]
CSD, AMPM = 0, 1
GIVEN = (0.0137, 0.3 - 1.7j, -2.0 + 0.25j)  # p_ab, w, q: neither w nor q of magnitude 1
CSD_KEYS = ("saa_up", "saa_lo", "sbb_up", "sbb_lo", "sab_up", "sab_lo", "freq", "coh_up", "coh_lo", "h1_up", "h1_lo")
AMPM_KEYS = ("cab", "cba", "s_am", "s_pm", "s_am_pm", "s_pm_am")


@pytest.fixture(scope="session")
def pair_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pair_readout_host")


def accumulators(rng, rows, ns, bins):
    """f64 accumulators [ns][rows][bins] that do not fit f32: autos > 0 with a zero S_aa upper / S_bb lower here and there in every
    stage, crosses of either sign below the geometric mean of the autos"""
    acc = np.exp(rng.normal(0.0, 3.0, (ns, rows, bins)))
    scale = np.sqrt(acc[:, 0:1] * acc[:, 2:3])
    acc[:, 4:] = rng.normal(0.0, 0.5, (ns, rows - 4, bins)) * scale
    acc[:, 0, 5::11] = 0.0
    acc[:, 3, 7::13] = 0.0
    return acc


def variants(mode):
    """(tag, given, how stage 0 is prepared) of a case in a mode"""
    if mode != AMPM:
        return [("", 0, None)]
    return [("", 0, None), (" given", 1, None), (" cab[0]=0", 0, "zero_c"), (" sab_up[0]=0", 0, "zero_u"), (" no average", 0, "count0")]


@pytest.fixture(scope="session")
def dump(pkg, pair_host_dir):
    """every case of tests/test_bank_readout_host.py as 8-row CSD, 12-row CSD and 12-row AM/PM (the carriers from bin 0, given,
    cab[0] == 0, sab_up[0] == 0 and stage 0 without an average) through the plain program once"""
    rng = np.random.default_rng(20261023)
    wt = pkg.WindowTable.hann(64)
    blob, out = [], []
    few = [("a deepest stage without an average", 64, [70, 2, 0], pkg.MergeOpts(keep_overlap=True, min_count=0))]
    for what, n, counts, opts in cases(pkg) + few:
        for mode, rows in ((CSD, 8), (CSD, 12), (AMPM, 12)):
            for tag, given, prep in variants(mode):
                ns, bins = len(counts), n // 2 + 1
                acc = accumulators(rng, rows, ns, bins)
                if ns:
                    acc[0, :4, 0] = np.abs(acc[0, :4, 0]) + 1.0  # (the locks' denominators)
                if prep == "zero_c" and ns:
                    acc[0, 8:10, 0] = 0.0
                if prep == "zero_u" and ns:
                    acc[0, (4, 6), 0] = 0.0
                count0 = 0 if (prep == "count0" or not ns) else min(int(counts[0]), pkg.U32_MAX)
                f32 = acc.astype(np.float32)
                stitched = [pkg.stitch(n, counts, [pkg.U32_MAX] * ns, [0] * ns, np.ascontiguousarray(f32[:, r]), opts) for r in range(8)]
                breaks = stitched[0][1]
                assert len(breaks) == ns and all(s[1] == breaks for s in stitched)
                blob.append(struct.pack("<8I2f5d", n, ns, len(breaks), len(BANDS), mode, rows, given, count0, wt.nenbw, wt.power,
                                        GIVEN[0], GIVEN[1].real, GIVEN[1].imag, GIVEN[2].real, GIVEN[2].imag))
                blob.append(np.asarray(counts, np.uint64).tobytes())
                blob += [bytes(b._c()) for b in breaks]
                blob.append(acc.tobytes())
                blob.append(np.asarray(BANDS, np.float32).tobytes())
                out.append(dict(what=f"{what} mode={mode} rows={rows}{tag}", mode=mode, rows=rows, given=given, count0=count0, n=n,
                                counts=counts, acc=acc, want=[p for p, _ in stitched], breaks=breaks, nenbw=wt.nenbw, power=wt.power))
    src, dst = (os.path.join(str(pair_host_dir), name) for name in ("cases.bin", "rows.bin"))
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(blob))
    exe = host_exe(pair_host_dir, "pair_readout_check", False)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
    raw, pos = open(dst, "rb").read(), 0

    def take(dtype, count, width=1):
        nonlocal pos
        a = np.frombuffer(raw, dtype, count * width, pos)
        pos += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    for d in out:
        L = int(take(np.uint64, 1)[0])
        if d["mode"] == CSD:
            for k, w in zip(CSD_KEYS[:7], (1, 1, 1, 1, 2, 2, 1)):
                d[k] = take(np.float32, L, w)
            for k, w in zip(CSD_KEYS[7:], (1, 1, 2, 2)):
                d[k] = take(np.float64, L, w)
        else:
            d["freq"] = take(np.float32, L)
            for k in AMPM_KEYS:
                d[k] = take(np.float64, L, 2)
            d["carrier"] = take(np.float64, 7)
        d["bands"] = take(np.float64, len(BANDS), 8)
    assert pos == len(raw)
    return out


def same(a, b):
    """byte for byte, where NaN equals NaN of either sign"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())


def placed(d):
    return ref.placed(d["acc"], d["breaks"], d["n"], d["counts"], d["nenbw"], d["power"])[:2]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_pair_readout_check(pkg, pair_host_dir, dump, sanitize):
    """the program's own checks (every job covers its row exactly once; every element of every asked output written exactly once and
    nothing else, each output alone -- the rows a thread loads depend on what is asked -- and all together; exactly one write a
    carrier record; the known answers of coherence, H1, shared pure AM and shared pure PM; the NaN records; an excluded middle stage,
    an empty pair, 300 records in two blocks; two four-row band walks against one of eight; the argument rules), plainly and under
    ASan + UBSan; the sanitized program also runs every case of this file and must write the same bytes"""
    exe = host_exe(pair_host_dir, "pair_readout_check", sanitize)
    out = run_host(exe)
    assert int(re.search(r"pair_readout_check: (\d+) checks", out).group(1)) > 1000
    if sanitize:
        src, dst = (os.path.join(str(pair_host_dir), name) for name in ("cases.bin", "rows_san.bin"))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        assert open(dst, "rb").read() == open(os.path.join(str(pair_host_dir), "rows.bin"), "rb").read()


def test_host_makefile_target():
    """tests/host/pair_readout_check.mk builds the program plainly and under the sanitizers (targets pair_readout_check[_san])"""
    mk = open(os.path.join(ROOT, "tests", "host", "pair_readout_check.mk")).read()
    assert re.search(r"^pair_readout_check: pair_readout_check\.cpp", mk, re.M) and re.search(r"^pair_readout_check_san: .*\n\t.*\$\(SAN\)", mk, re.M)


def test_sides_and_frequencies_equal_the_stitch(pkg, dump):
    """the six f32 outputs and the frequencies, byte for byte, against the restatement and against the library's host stitch of the
    f32-cast rows: 1, 3 and 16 stages, the merge options on and off, a min_count that excludes the deepest, a middle and every stage,
    counts at and above 2^32, no stage; on 8 and on 12 rows"""
    seen = dict(empty=0, excluded=0, big=0, none=0, rows12=0)
    for d in dump:
        if d["mode"] != CSD:
            assert d["freq"].tobytes() == pkg.Break.frequencies(d["breaks"]).tobytes(), d["what"]
            continue
        rows, g = placed(d)
        want = ref.csd_sides(rows, g) if len(g) else None
        got6 = [d["saa_up"], d["saa_lo"], d["sbb_up"], d["sbb_lo"], d["sab_up"][:, 0], d["sab_lo"][:, 0], d["sab_up"][:, 1], d["sab_lo"][:, 1]]
        for r in range(8):
            assert got6[r].tobytes() == d["want"][r].tobytes(), (d["what"], r)
            if want:
                assert got6[r].tobytes() == want["f32"][r].tobytes(), (d["what"], r)
        assert d["freq"].tobytes() == pkg.Break.frequencies(d["breaks"]).tobytes(), d["what"]
        assert d["freq"].tobytes() == ref.frequencies(d["breaks"]).tobytes(), d["what"]
        assert len(d["freq"]) == sum(len(b.bins) for b in d["breaks"] if b.include), d["what"]
        seen["empty"] += int(len(d["freq"]) == 0)
        seen["excluded"] += int(any(not b.include for b in d["breaks"]) and len(d["freq"]) > 0)
        seen["big"] += int("2^32" in d["what"])
        seen["none"] += int(not d["breaks"])
        seen["rows12"] += int(d["rows"] == 12)
    assert all(seen.values()), seen


def test_coherence_and_h1_equal_the_restatement(pkg, dump):
    """coherence and H1 of both sides byte for byte; NaN exactly where the denominator is 0, which every stage has on either side"""
    nans = np.zeros(2, int)
    for d in dump:
        if d["mode"] != CSD or not len(d["freq"]):
            continue
        rows, g = placed(d)
        want = ref.csd_sides(rows, g)
        for k in ("coh_up", "coh_lo", "h1_up", "h1_lo"):
            assert same(d[k], want[k]), (d["what"], k)
        assert np.array_equal(np.isnan(d["coh_up"]), rows[0] * rows[2] == 0) and np.array_equal(np.isnan(d["h1_up"][:, 0]), rows[0] == 0)
        assert np.array_equal(np.isnan(d["coh_lo"]), rows[1] * rows[3] == 0) and not np.any(np.isnan(d["h1_lo"]))
        nans += [int(np.isnan(d["coh_up"]).sum()), int(np.isnan(d["coh_lo"]).sum())]
    assert np.all(nans > 10), nans


def carriers_of(d):
    if d["given"]:
        return ref.carriers_given(*GIVEN)
    if len(d["counts"]):
        return ref.carriers_from_bin0(d["n"], d["power"], d["count0"], d["acc"][0][:, 0])
    return ref.NO_CARRIER


def test_am_pm_cross_equals_the_restatement(pkg, dump):
    """cab, cba, the four AM/PM rows and the carrier record byte for byte: the carriers from bin 0 of stage 0 whatever the merge
    options include, given carriers (normalised on the host, locks NaN), and the record (0, NaN x 6) with NaN rows for cab[0] == 0,
    sab_up[0] == 0 and a stage 0 without an average, whose cab / cba stay"""
    seen = dict(bin0=0, given=0, nan=0, stage0_excluded=0)
    for d in dump:
        if d["mode"] != AMPM:
            continue
        rows, g = placed(d)
        car = carriers_of(d)
        assert same(d["carrier"], np.asarray(car, np.float64)), (d["what"], d["carrier"], car)
        no_carrier = bool(np.isnan(car[1]))
        assert no_carrier == (not d["given"] and ("]=0" in d["what"] or "no average" in d["what"] or not len(d["counts"]))), d["what"]
        if len(g):
            cab, cba = ref.cross_rows(rows, g)
            assert d["cab"].tobytes() == cab.tobytes() and d["cba"].tobytes() == cba.tobytes(), d["what"]
            s = ref.split(rows, g, car)
            for i, k in enumerate(AMPM_KEYS[2:]):
                assert same(d[k], s[:, 2 * i:2 * i + 2]), (d["what"], k)
                ok = np.isfinite(g)
                assert np.all(np.isnan(d[k])) if no_carrier else np.all(np.isfinite(d[k][ok])), (d["what"], k)
        if no_carrier:
            assert car[0] == 0.0
        seen["given"] += int(d["given"] and np.isnan(car[5]) and abs(np.hypot(car[1], car[2]) - 1) < 1e-15)
        seen["bin0"] += int(not d["given"] and not no_carrier and car[5] > 0 and car[6] > 0)
        seen["nan"] += int(no_carrier and len(g) > 0)
        seen["stage0_excluded"] += int(not d["given"] and not no_carrier and len(d["breaks"]) > 0 and not d["breaks"][-1].include)
    assert all(seen.values()), seen


def test_am_pm_cross_is_am_pm_cross_from_sidebands(pkg, dump):
    """the restated real arithmetic is the package's complex formula: within 16 * 2^-53 (|U| + |L| + |cab| + |cba|) / (4 P) a
    component (at most eight f64 roundings a side)"""
    worst = 0.0
    for d in dump:
        if d["mode"] != AMPM or not len(d["freq"]) or np.isnan(d["carrier"][1]):
            continue
        rows, g = placed(d)
        ok = np.isfinite(g)
        sc = rows[4:12, ok] * g[ok]
        U, L, cab, cba = sc[0] + 1j * sc[2], sc[1] + 1j * sc[3], sc[4] + 1j * sc[5], sc[6] + 1j * sc[7]
        P, w, q = d["carrier"][0], complex(*d["carrier"][1:3]), complex(*d["carrier"][3:5])
        want = pkg.am_pm_cross_from_sidebands(U, L, cab, cba, P, w, q)
        scale = (np.abs(U) + np.abs(L) + np.abs(cab) + np.abs(cba)) / (4.0 * P)
        for k, wv in zip(AMPM_KEYS[2:], want):
            got = d[k][ok, 0] + 1j * d[k][ok, 1]
            err = np.maximum(np.abs(got.real - wv.real), np.abs(got.imag - wv.imag)) / scale
            worst = max(worst, float(err.max()) * 2.0 ** 53)
            assert np.all(err <= 16 * 2.0 ** -53), (d["what"], k, float(err.max()) * 2.0 ** 53)
    print(f"largest deviation from am_pm_cross_from_sidebands: {worst:.2f} * 2^-53 of the scale")
    assert worst > 0.0


def band_values(d):
    """[8][L] f64: what the band sums of the case integrate"""
    if d["mode"] == CSD:
        return np.stack([d["saa_up"], d["saa_lo"], d["sbb_up"], d["sbb_lo"], d["sab_up"][:, 0], d["sab_lo"][:, 0], d["sab_up"][:, 1],
                         d["sab_lo"][:, 1]]).astype(np.float64)
    return np.concatenate([d[k].T for k in AMPM_KEYS[2:]])


def test_band_sums(pkg, dump):
    """bit-equal to bank_band_rows_host's order restated in numpy (thread stride 256, the shuffle tree, the wavefronts in order) on
    the values the program wrote -- the f32 rows 0 ... 7, or the f64 AM/PM components without an f32 cast -- and within
    L * 2^-52 * sum |t_k| of numpy's plain f64 sum of the same trapezoids (np.trapz with a leading zero)"""
    held = np.zeros(len(BANDS), int)
    f64_rows = trapz = 0
    for d in dump:
        vals = band_values(d)
        if len(d["freq"]) and np.all(np.isfinite(vals)):
            assert same(d["bands"], ref.band_sums(vals, d["freq"], BANDS)), d["what"]
        elif not len(d["freq"]):
            assert np.all(d["bands"] == 0.0)
        for r, row in enumerate(vals):
            if not np.all(np.isfinite(row)):  # (a stage without a segment stitches to NaN; a pair without carriers)
                continue
            for b, (want, tol, count) in enumerate(band_reference(row, d["freq"], BANDS)):
                assert abs(d["bands"][b, r] - want) <= tol, (d["what"], r, b, d["bands"][b, r], want, tol)
                if count == 0:
                    assert d["bands"][b, r] == 0.0
                held[b] = max(held[b], count)
                f64_rows += int(d["mode"] == AMPM and count > 1)
            if len(row) > 1 and BANDS[0] == (0.0, 0.5):
                whole = (getattr(np, "trapezoid", None) or np.trapz)(np.concatenate([[0.0], row]), np.concatenate([[0.0], d["freq"].astype(np.float64)]))
                assert abs(d["bands"][0, r] - whole) <= band_reference(row, d["freq"], BANDS)[0][1]
                trapz += 1
    assert held[3] == 1 and held[4] == 0 and held[0] > 1000 and f64_rows > 100 and trapz > 100, (held, f64_rows, trapz)


def test_exports(pkg):
    """include/ext/psdcascade_pairread.h declares exactly the six psdcpr_ entry points, compiles as plain C99 with -Wall -Wextra -Werror,
    and the library exports exactly those; each returns ERR_ARG with a text on a NULL handle and touches no output; the other
    headers, EXPORTS and the ABI version are unchanged; pairread adds nothing to the classes"""
    inc = os.path.join(ROOT, "include")
    path = os.path.join(inc, "ext", "psdcascade_pairread.h")
    hdr = open(path).read()
    code = hdr[hdr.index("#ifndef PSDCASCADE_PAIRREAD_H"):]
    assert sorted(set(re.findall(r"\b(psdcpr_[a-z0-9_]+)\s*\(", code))) == sorted(SYMBOLS)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdcpr_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdcpr_")]
    others = [f for f in os.listdir(inc) if f.endswith(".h")]  # (the headers before this one: it lives in include/ext)
    assert len(others) == 6 and os.listdir(os.path.join(inc, "ext")) == ["psdcascade_pairread.h"]
    for other in others:
        text = open(os.path.join(inc, other)).read()
        assert not re.search(r"psdcpr_[a-z]", text), other
    assert "psdcascade_pairread.h" in open(os.path.join(inc, "psdcascade_carrierread.h")).read()
    assert pkg.lib().psdc_abi_version() == 3
    from stabilizer_stream_amd import pairread
    L = pairread._lib()
    lens = np.full(4, 77, np.uintp)
    buf = np.zeros(64, np.float32)
    info = pairread._CInfo()
    tail = (lens.ctypes.data, None, None, 0, C.byref(info))
    head = (None, None, 0, 0, 1, 0)
    p = buf.ctypes.data
    calls = {"psdcpr_layout": (*head, *tail),
             "psdcpr_csd_device": (*head, p, *[None] * 10, 64, None, 0, None, None, *tail),
             "psdcpr_csd": (*head, p, *[None] * 10, 64, None, 0, None, *tail),
             "psdcpr_ampm_device": (*head, None, p, *[None] * 7, 64, None, 0, None, None, *tail),
             "psdcpr_ampm": (*head, None, p, *[None] * 7, 64, None, 0, None, *tail),
             "psdcpr_release": (None,)}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == pkg.ERR_ARG, name
        for family in ("psdc_zcsd", "psdc_iqcsd", "psdc_zxampm", "psdc_iqxampm"):
            assert getattr(pkg.lib(), family + "_last_error")(None).decode() == name + ": null handle"
    assert np.all(lens == 77) and np.all(buf == 0)
    assert pairread.MAX_BANDS == 8
    for cls in ("ZoomCsdCascadeBank", "ZoomCsdCascade", "IqCsdCascadeBank", "IqCsdCascade", "ZoomAmPmCsdCascadeBank", "ZoomAmPmCsdCascade",
                "IqAmPmCsdCascadeBank", "IqAmPmCsdCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "bank_" in m or "layout" in m], cls
    for fn in (pairread.layout, pairread.bank_csd, pairread.bank_am_pm_cross, pairread.release):
        with pytest.raises(pkg.PsdError) as e:
            fn(object())
        assert e.value.code == pkg.ERR_ARG
    for fn in (pairread.bank_csd_device, pairread.bank_am_pm_cross_device):
        with pytest.raises(pkg.PsdError) as e:
            fn(object(), 64, freq=p)
        assert e.value.code == pkg.ERR_ARG
    co = pairread.band_coherence(np.array([[2.0, 0.0, 8.0, 5.0, 3.0, 1.0, 1.0, 2.0]]))
    assert co[0][0] == 10.0 / 16.0 and np.isnan(co[1][0])
