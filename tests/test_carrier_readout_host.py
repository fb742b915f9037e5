"""Bank read-out of the zoom, IQ, zoom / IQ SK and zoom / IQ AM/PM objects (include/psdcascade_carrierread.h, psdczr_*;
stabilizer-stream_amd/carrierread.py): the parts that run without a GPU.

csrc/carrier_readout.h -- the job and unit tables made from Break lists, what one thread of carrier_stitch_kernel<MODE> computes
for one bin (sides, SK, the AM/PM split with the carrier from bin 0 of stage 0 or given), the carrier records, what
carrier_band_kernel<R> adds up for one channel and the argument rules that need no object -- runs on the host in
tests/host/carrier_readout_check.cpp, which this file compiles itself: once plainly and once under the address and
undefined-behaviour sanitizers (a stand-alone program; nothing is loaded into Python).  The Breaks come from the library's host-only
stitch (pkg.stitch) of the f32-cast accumulator rows; upper, lower and the frequencies must equal that stitch's and
Break.frequencies byte for byte, SK pkg.sk_from_moments and the AM/PM outputs tests/carrier_read_ref.py byte for byte (g++ on
x86-64 without -march does not fuse), the band sums numpy's f64 sum of the same trapezoids within the summation bound of
tests/test_bank_readout_host.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import carrier_read_ref as ref
from test_bank_readout_host import BANDS, band_reference, cases
from test_waterfall_host import host_exe, run_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["psdczr_layout", "psdczr_sides_device", "psdczr_sides", "psdczr_sk_device", "psdczr_sk", "psdczr_ampm_device", "psdczr_ampm",
           "psdczr_release", ]
SIDES, SK, AMPM = 0, 1, 2
GIVEN = 0.3 - 1.7j


@pytest.fixture(scope="session")
def carrier_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("carrier_readout_host")


def accumulators(rng, mode, ns, bins, counts):
    """f64 accumulators [ns][rows][bins] that do not fit f32.  SK: S1 > 0 and S2 near 2 S1^2 / M, with a zero S1 of either side
    in every stage.  AM/PM: upper, lower > 0 and comp of either sign below their geometric mean."""
    rows = 2 if mode == SIDES else 4
    acc = np.exp(rng.normal(0.0, 3.0, (ns, rows, bins)))
    if mode == SK:
        m = np.maximum(np.asarray(counts, np.float64), 1.0)[:, None, None]
        acc[:, 2:] = acc[:, :2] ** 2 / m * rng.uniform(1.0, 3.0, (ns, 2, bins))
        acc[:, 0, 5::11] = 0.0
        acc[:, 1, 7::13] = 0.0
    elif mode == AMPM:
        acc[:, 2:] = rng.normal(0.0, 0.5, (ns, 2, bins)) * np.sqrt(acc[:, 0:1] * acc[:, 1:2])
    return acc


def variants(mode):
    """(tag, given, how stage 0 is prepared) of a case in a mode"""
    if mode != AMPM:
        return [("", 0, None)]
    return [("", 0, None), (" given", 1, None), (" comp[0]=0", 0, "zero"), (" no average", 0, "count0")]


@pytest.fixture(scope="session")
def dump(pkg, carrier_host_dir):
    """every case of tests/test_bank_readout_host.py in the three modes (AM/PM: the carrier from bin 0, given, comp[0] == 0 and
    stage 0 without an average) through the plain program once"""
    rng = np.random.default_rng(20261022)
    wt = pkg.WindowTable.hann(64)
    blob, out = [], []
    # (and stages of one and of no average, included: SK is NaN there through count < 2)
    few = [("a deepest stage of one average", 64, [900, 30, 1], pkg.MergeOpts(min_count=0)),
           ("one stage of one average", 1024, [1], pkg.MergeOpts(min_count=1)),
           ("a deepest stage without an average", 64, [70, 2, 0], pkg.MergeOpts(keep_overlap=True, min_count=0))]
    for what, n, counts, opts in cases(pkg) + few:
        for mode in (SIDES, SK, AMPM):
            for tag, given, prep in variants(mode):
                ns, bins = len(counts), n // 2 + 1
                # (the Break's count is what the stitch reports for the stage: SK takes it, so a stage of one average is NaN)
                acc = accumulators(rng, mode, ns, bins, counts)
                if prep == "zero" and ns:
                    acc[0, 2:, 0] = 0.0
                count0 = 0 if (prep == "count0" or not ns) else min(int(counts[0]), pkg.U32_MAX)
                f32 = acc.astype(np.float32)
                stitched = [pkg.stitch(n, counts, [pkg.U32_MAX] * ns, [0] * ns, np.ascontiguousarray(f32[:, r]), opts) for r in range(2)]
                breaks = stitched[0][1]
                assert len(breaks) == ns and stitched[1][1] == breaks
                blob.append(struct.pack("<7I2f2d", n, ns, len(breaks), len(BANDS), mode, given, count0, wt.nenbw, wt.power, GIVEN.real, GIVEN.imag))
                blob.append(np.asarray(counts, np.uint64).tobytes())
                blob += [bytes(b._c()) for b in breaks]
                blob.append(acc.tobytes())
                blob.append(np.asarray(BANDS, np.float32).tobytes())
                out.append(dict(what=f"{what} mode={mode}{tag}", mode=mode, given=given, count0=count0, n=n, counts=counts, acc=acc,
                                want=[p for p, _ in stitched], breaks=breaks, nenbw=wt.nenbw, power=wt.power))
    src, dst = (os.path.join(str(carrier_host_dir), name) for name in ("cases.bin", "rows.bin"))
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(out)) + b"".join(blob))
    exe = host_exe(carrier_host_dir, "carrier_readout_check", False)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK") and "FAIL" not in r.stdout, (r.stdout + r.stderr)[-3000:]
    raw, pos = open(dst, "rb").read(), 0
    for d in out:
        L = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        pos += 8
        d["upper"], d["lower"], d["freq"] = (np.frombuffer(raw, np.float32, L, pos + 4 * L * k) for k in range(3))
        pos += 12 * L
        if d["mode"] != SIDES:
            d["a"], d["b"] = (np.frombuffer(raw, np.float64, L, pos + 8 * L * k) for k in range(2))
            pos += 16 * L
        if d["mode"] == AMPM:
            d["c"] = np.frombuffer(raw, np.float64, 2 * L, pos).reshape(L, 2)
            d["carrier"] = np.frombuffer(raw, np.float64, 4, pos + 16 * L)
            pos += 16 * L + 32
        rows = {SIDES: 2, SK: 0, AMPM: 4}[d["mode"]]
        d["bands"] = np.frombuffer(raw, np.float64, rows * len(BANDS), pos).reshape(len(BANDS), rows)
        pos += 8 * rows * len(BANDS)
    assert pos == len(raw)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_carrier_readout_check(pkg, carrier_host_dir, dump, sanitize):
    """the program's own checks (every element of every asked output written exactly once and nothing else, each output alone and all
    together, exactly one write a carrier record, the known answers of SK and of pure AM / pure PM, the NaN records, an excluded
    middle stage, an empty channel, 300 records in two blocks, the argument rules), plainly and under ASan + UBSan; the sanitized
    program also runs every case of this file and must write the same bytes"""
    exe = host_exe(carrier_host_dir, "carrier_readout_check", sanitize)
    out = run_host(exe)
    assert int(re.search(r"carrier_readout_check: (\d+) checks", out).group(1)) > 1000
    if sanitize:
        src, dst = (os.path.join(str(carrier_host_dir), name) for name in ("cases.bin", "rows_san.bin"))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        assert open(dst, "rb").read() == open(os.path.join(str(carrier_host_dir), "rows.bin"), "rb").read()


def test_sides_and_frequencies_equal_the_stitch(pkg, dump):
    """byte for byte in all three modes: 1, 3 and 16 stages, the merge options on and off, a min_count that excludes the deepest,
    a middle and every stage, counts at and above 2^32, no stage"""
    seen = dict(empty=0, excluded=0, big=0, none=0)
    for d in dump:
        assert d["upper"].tobytes() == d["want"][0].tobytes() and d["lower"].tobytes() == d["want"][1].tobytes(), d["what"]
        assert d["freq"].tobytes() == pkg.Break.frequencies(d["breaks"]).tobytes(), d["what"]
        assert len(d["freq"]) == sum(len(b.bins) for b in d["breaks"] if b.include), d["what"]
        seen["empty"] += int(len(d["freq"]) == 0)
        seen["excluded"] += int(any(not b.include for b in d["breaks"]) and len(d["freq"]) > 0)
        seen["big"] += int("2^32" in d["what"])
        seen["none"] += int(not d["breaks"])
    assert all(seen.values()), seen


def test_sk_equals_sk_from_moments(pkg, dump):
    """sk_upper / sk_lower = pkg.sk_from_moments(break.count, s1, s2) byte for byte; NaN exactly where count < 2 or s1 == 0"""
    nans = np.zeros(2, int)
    for d in dump:
        if d["mode"] != SK:
            continue
        rows, _, m = ref.placed(d["acc"], d["breaks"], d["n"], d["counts"], d["nenbw"], d["power"])
        for side, got in ((0, d["a"]), (1, d["b"])):
            full = np.empty(len(m))
            for c in set(m.tolist()):  # (the count of a Break: one stage's bins at a time)
                full[m == c] = pkg.sk_from_moments(int(c), rows[side][m == c], rows[2 + side][m == c])
            assert got.tobytes() == full.tobytes(), (d["what"], side)
            assert got.tobytes() == ref.sk(m, rows[side], rows[2 + side]).tobytes(), (d["what"], side)
            assert np.array_equal(np.isnan(got), (m < 2) | (rows[side] == 0)), (d["what"], side)
            nans += [int(np.sum((m < 2))), int(np.sum((m >= 2) & (rows[side] == 0)))]
    assert np.all(nans > 10), nans


def test_am_pm_equals_the_restatement(pkg, dump):
    """carrier, s_am, s_pm and s_ampm against tests/carrier_read_ref.py byte for byte: the carrier from bin 0 of stage 0 whatever
    the merge options include, a given amplitude (lock NaN), and the NaN record with NaN rows for comp[0] == 0 and for a stage 0
    without an average"""
    seen = dict(bin0=0, given=0, nan=0, stage0_excluded=0)
    for d in dump:
        if d["mode"] != AMPM:
            continue
        rows, g, _ = ref.placed(d["acc"], d["breaks"], d["n"], d["counts"], d["nenbw"], d["power"])
        if d["given"]:
            car = ref.carrier_given(GIVEN)
        elif len(d["counts"]):
            a0 = d["acc"][0]
            car = ref.carrier_from_bin0(d["n"], d["power"], d["count0"], a0[0, 0], a0[1, 0], a0[2, 0], a0[3, 0])
        else:
            car = ref.carrier_from_bin0(d["n"], d["power"], None, 0, 0, 0, 0)
        assert d["carrier"].tobytes() == np.asarray(car, np.float64).tobytes(), (d["what"], d["carrier"], car)
        if len(g):
            s_am, s_pm, s_x = ref.split(rows[0], rows[1], rows[2], rows[3], g, *car[:3])
            assert d["a"].tobytes() == s_am.tobytes() and d["b"].tobytes() == s_pm.tobytes(), d["what"]
            assert d["c"].tobytes() == np.stack([s_x.real, s_x.imag], axis=1).tobytes(), d["what"]
        no_carrier = np.isnan(car[1])
        assert no_carrier == (not d["given"] and ("comp[0]=0" in d["what"] or "no average" in d["what"] or not len(d["counts"]))), d["what"]
        if no_carrier:
            assert car[0] == 0.0 and np.all(np.isnan(d["a"])) and np.all(np.isnan(d["b"])) and np.all(np.isnan(d["c"]))
        else:
            ok = np.isfinite(g)
            assert np.all(np.isfinite(d["a"][ok])) and np.all(np.isfinite(d["c"][ok]))
        seen["given"] += int(d["given"] and np.isnan(car[3]))
        seen["bin0"] += int(not d["given"] and not no_carrier and car[3] > 0)
        seen["nan"] += int(no_carrier and len(g) > 0)
        seen["stage0_excluded"] += int(not d["given"] and not no_carrier and len(d["breaks"]) > 0 and not d["breaks"][-1].include)
    assert all(seen.values()), seen


def test_band_sums(pkg, dump):
    """upper and lower: within L * 2^-52 * sum |t_k| of numpy's f64 sum of the trapezoids of the stitched f32 row.  s_am and s_pm:
    the same bound on the trapezoids of the f64 values the program wrote (no f32 cast: the f64 rows are passed as they are)."""
    held = np.zeros(len(BANDS), int)
    f64_rows = 0
    for d in dump:
        if d["mode"] == SK:
            assert d["bands"].size == 0
            continue
        rows = [d["upper"], d["lower"]] + ([d["a"], d["b"]] if d["mode"] == AMPM else [])
        for r, row in enumerate(rows):
            if not np.all(np.isfinite(row)):  # (a stage without a segment stitches to NaN; a channel without a carrier)
                continue
            for b, (want, tol, count) in enumerate(band_reference(row, d["freq"], BANDS)):
                assert abs(d["bands"][b, r] - want) <= tol, (d["what"], r, b, d["bands"][b, r], want, tol)
                if count == 0:
                    assert d["bands"][b, r] == 0.0
                held[b] = max(held[b], count)
                f64_rows += int(r >= 2 and count > 1)
    assert held[3] == 1 and held[4] == 0 and held[0] > 1000 and f64_rows > 100, (held, f64_rows)


def test_exports(pkg):
    """include/psdcascade_carrierread.h declares exactly the eight psdczr_ entry points (layout, the device and host forms of sides,
    sk and ampm, release), compiles as plain C, and the library exports exactly those; each returns ERR_ARG with a text on a NULL handle and touches no
    output; the other headers, EXPORTS and the ABI version are unchanged; carrierread adds nothing to the classes"""
    inc = os.path.join(ROOT, "include")
    hdr = open(os.path.join(inc, "psdcascade_carrierread.h")).read()
    code = hdr[hdr.index("#ifndef PSDCASCADE_CARRIERREAD_H"):]
    assert sorted(set(re.findall(r"\b(psdczr_[a-z0-9_]+)\s*\(", code))) == sorted(SYMBOLS)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "psdcascade_carrierread.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r" T (psdczr_[a-z0-9_]+)", out)) == sorted(SYMBOLS)
    assert not [s for s in pkg.EXPORTS if s.startswith("psdczr_")]
    others = [f for f in os.listdir(inc) if f.endswith(".h") and f != "psdcascade_carrierread.h"]
    assert len(others) == 5
    for other in others:
        assert "psdczr_" not in open(os.path.join(inc, other)).read(), other
    assert pkg.lib().psdc_abi_version() == 3
    from stabilizer_stream_amd import carrierread
    L = carrierread._lib()
    lens = np.full(4, 77, np.uintp)
    buf = np.zeros(64, np.float32)
    info = carrierread._CInfo()
    tail = (lens.ctypes.data, None, None, 0, C.byref(info))
    head = (None, None, 0, 0, 1, 0)
    p = buf.ctypes.data
    calls = {"psdczr_layout": (*head, *tail),
             "psdczr_sides_device": (*head, p, None, None, 64, None, 0, None, None, *tail),
             "psdczr_sides": (*head, p, None, None, 64, None, 0, None, *tail),
             "psdczr_sk_device": (*head, p, None, None, None, None, 64, None, *tail),
             "psdczr_sk": (*head, p, None, None, None, None, 64, *tail),
             "psdczr_ampm_device": (*head, None, p, None, None, None, None, None, None, 64, None, 0, None, None, *tail),
             "psdczr_ampm": (*head, None, p, None, None, None, None, None, None, 64, None, 0, None, *tail),
             "psdczr_release": (None,)}
    assert sorted(calls) == sorted(SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(*args) == pkg.ERR_ARG, name
        for family in ("psdc_zoom", "psdc_iq", "psdc_zsk", "psdc_iqsk", "psdc_zampm", "psdc_iqampm"):
            assert getattr(pkg.lib(), family + "_last_error")(None).decode() == name + ": null handle"
    assert np.all(lens == 77) and np.all(buf == 0)
    assert carrierread.MAX_BANDS == 8
    for cls in ("ZoomCascadeBank", "ZoomCascade", "IqCascadeBank", "IqCascade", "ZoomSkCascadeBank", "ZoomSkCascade", "IqSkCascadeBank",
                "IqSkCascade", "ZoomAmPmCascadeBank", "ZoomAmPmCascade", "IqAmPmCascadeBank", "IqAmPmCascade"):
        assert not [m for m in dir(getattr(pkg, cls)) if "bank_" in m or "layout" in m], cls
    for fn in (carrierread.layout, carrierread.bank_sides, carrierread.bank_sk, carrierread.bank_am_pm, carrierread.release):
        with pytest.raises(pkg.PsdError) as e:
            fn(object())
        assert e.value.code == pkg.ERR_ARG
    for fn in (carrierread.bank_sides_device, carrierread.bank_sk_device, carrierread.bank_am_pm_device):
        with pytest.raises(pkg.PsdError) as e:
            fn(object(), 64, upper=p)
        assert e.value.code == pkg.ERR_ARG
