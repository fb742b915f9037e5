"""Waterfall cascades (psdc_wf_*, psdc_zwf_*): the parts that run without a GPU.  Semantics: include/psdcascade.h, "waterfall
cascades".

restate_waterfall / restate_zoom_waterfall below are the yardsticks of tests/test_gpu_waterfall.py: restate_sk / restate_zoom_sk
(tests/test_sk_host.py, tests/test_zoom_sk_host.py) with the segments of a stage grouped into blocks of B and one row set a
block, every segment with weight 1.  They are anchored here: summed over a stage's blocks they are restate_sk / restate_zoom_sk
with default averaging to 1e-12.  The tone-switch property the GPU test asserts is checked on the f64 restatement first.

The piece cut (csrc/waterfall_plan.h) and the read-out kernel's per-element arithmetic and ring-order map
(csrc/waterfall_read.h) run on the host in tests/host/waterfall_plan_check.cpp and tests/host/waterfall_emul.cpp, which this file
compiles itself: once plainly and once under the address and undefined-behaviour sanitizers (stand-alone programs; nothing is
loaded into Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cross_host import DRAIN, _window
from test_sk_host import gaussian, restate_sk
from test_zoom_host import mix_f64
from test_zoom_sk_host import restate_zoom_sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_COMMON = ["supported", "create", "create_window", "destroy", "reset", "set_detrend", "process", "process_device", "sync", "num_stages",
           "stage_blocks", "stage_rows", "image", "image_device", "stats_read", "last_error"]
WF_SYMBOLS = ["psdc_wf_" + s for s in _COMMON]
ZWF_SYMBOLS = ["psdc_zwf_" + s for s in _COMMON + ["set_carrier"]]

WF_ROWS = ("s1", "s2")
ZWF_ROWS = ("upper", "lower", "s2_upper", "s2_lower")


# ---- the restatements ----

def _restate_blocks(ora, streams, n, block, window, detrend, prec, max_stages, rows_of, schedule=None):
    """The cascade of the m streams (one for the real kind; I and Q for the zoom kind): per stage
    dict(segs, pending, blocks=[dict(index, count, rows...)]), stage 0 first, EVERY block since the stream's start (a ring keeps the
    newest K of them).  rows_of(specs of one segment) -> {row name: its periodogram term}.  Stage bookkeeping as restate_sk.
    schedule: a settings_schedule.Schedule of mid-stream set_detrend calls; it then replaces detrend."""
    win, _, _, overlap, kind = _window(ora, n, window)
    hop = n - overlap
    ft = np.float64 if prec == "f64" else np.float32
    xs = [np.asarray(s, ft if len(streams) > 1 else np.float32) for s in streams]
    stages = []
    k = 0
    while xs[0].size and (max_stages is None or k < max_stages):
        size = xs[0].size
        nseg = 0 if size < n else 1 + (size - n) // hop

        def prep(seg):
            if kind is not None:
                return ora.detrend_apply(seg, detrend, kind, prec)
            return ora.detrend_apply(seg, detrend, "rect", prec) * win.astype(ft)

        blocks = []
        for j in range(nseg):
            if schedule is not None:  # the detrend in force when segment j of stage k completed
                detrend = schedule.stage(k, j)[0]
            terms = rows_of([prep(x[j * hop:j * hop + n]) for x in xs])
            if j % block == 0:
                blocks.append(dict(index=j // block, count=0, **{name: np.zeros(n // 2 + 1, ft) for name in terms}))
            b = blocks[-1]
            b["count"] += 1
            for name, t in terms.items():
                b[name] = b[name] + t.astype(ft)
        pending = size if nseg == 0 else size - nseg * hop
        stages.append(dict(segs=nseg, pending=pending, blocks=blocks))
        p = nseg * hop + overlap if nseg else 0
        xs = [ora.hbf_dec8(x[:p], prec)[DRAIN:].astype(ft) for x in xs]
        k += 1
    return stages


def restate_waterfall(ora, x, n, block, window="hann", detrend="none", prec="f64", max_stages=None, schedule=None):
    """Waterfall cascade of the real stream x: per block the rows s1 = sum P and s2 = sum P^2 of its segments, with restate_sk's
    segment arithmetic (prec "f64": truth; "f32": the reference's arithmetic with f32 accumulation inside a block)"""
    h = n // 2 + 1
    ft = np.float64 if prec == "f64" else np.float32
    ct = np.complex128 if prec == "f64" else np.complex64

    def rows_of(segs):
        X = ora.fft_forward(segs[0].astype(ct), prec)[:h].astype(ct)
        p = (X.real * X.real + X.imag * X.imag).astype(ft)
        return {"s1": p, "s2": (p * p).astype(ft)}

    return _restate_blocks(ora, [x], n, block, window, detrend, prec, max_stages, rows_of, schedule)


def restate_zoom_waterfall(ora, x, n, ftw, block, window="hann", detrend="none", prec="f64", iq=None, max_stages=None,
                           schedule=None):
    """Zoom waterfall cascade of the real stream x around the carrier ftw: per block the four rows of restate_zoom_sk (upper,
    lower, s2_upper, s2_lower).  prec and iq as restate_zoom_sk takes them."""
    h = n // 2 + 1
    ft = np.float64 if prec == "f64" else np.float32
    ct = np.complex128 if prec == "f64" else np.complex64
    lower_idx = (n - np.arange(h)) % n
    si, sq = mix_f64(x, ftw, 0) if iq is None else iq

    def rows_of(segs):
        z = (segs[0].real + 1j * segs[1].real).astype(ct)
        Z = np.fft.fft(z) if prec == "f64" else ora.fft_forward(z, "f32").astype(ct)
        p = (Z.real * Z.real + Z.imag * Z.imag).astype(ft)
        p2 = (p * p).astype(ft)
        return {"upper": p[:h], "lower": p[lower_idx], "s2_upper": p2[:h], "s2_lower": p2[lower_idx]}

    return _restate_blocks(ora, [si, sq], n, block, window, detrend, prec, max_stages, rows_of, schedule)


def ring_of(stage, depth):
    """what a ring of `depth` rows holds of a restated stage: its newest blocks, oldest first"""
    return stage["blocks"][-depth:] if stage["blocks"] else []


# ---- the tone-switch property, shared with tests/test_gpu_waterfall.py ----

TONE_N, TONE_B, TONE_BLOCKS = 256, 8, 40
TONE_BINS = (10, 20)


def tone_input():
    """a tone at bin 10 of stage 0 for the first half of the stream and at bin 20 for the second half, on a weak noise floor;
    40 blocks of 8 Hann segments and a few samples more"""
    n = TONE_N
    length = (TONE_BLOCKS * TONE_B) * (n // 2) + n // 2 + 77
    half = length // 2
    t = np.arange(length, dtype=np.float64)
    f = np.where(t < half, TONE_BINS[0] / n, TONE_BINS[1] / n)
    x = np.cos(2 * np.pi * np.cumsum(f)) + 1e-3 * gaussian(length, 7)
    return x.astype(np.float32), half


def check_tone_switch(pkg, block_index, s1_rows, half, length):
    """every row whose block lies wholly in one half has its PSD argmax at that half's bin; at most 2 rows (the blocks touching the
    switch: consecutive blocks share `overlap` samples) may be left out, and that bound is asserted.  Returns the rows left out."""
    assert len(block_index) == len(s1_rows) > 4
    left_out = []
    seen = [0, 0]
    for b, row in zip(block_index, s1_rows):
        span = pkg.waterfall_block_span(TONE_N, TONE_N // 2, TONE_B, 0, int(b))
        assert span.stop <= length
        if span.stop <= half:
            side = 0
        elif span.start >= half:
            side = 1
        else:
            left_out.append(int(b))
            continue
        seen[side] += 1
        assert int(np.argmax(row)) == TONE_BINS[side], (int(b), int(np.argmax(row)), side)
    print(f"tone switch: {seen[0]} rows at bin {TONE_BINS[0]}, {seen[1]} at bin {TONE_BINS[1]}, left out {left_out}")
    assert len(left_out) <= 2 and min(seen) >= 4
    return left_out


# ---- exports ----

def test_waterfall_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    for prefix, symbols in (("psdc_wf_", WF_SYMBOLS), ("psdc_zwf_", ZWF_SYMBOLS)):
        declared = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr))
        assert declared == set(symbols), prefix
        assert set(re.findall(r" T (" + prefix + r"[a-z0-9_]+)", out)) == declared, prefix
        assert declared <= set(pkg.EXPORTS)
        for s in symbols:
            assert hasattr(pkg.lib(), s)
    assert not [s for s in WF_SYMBOLS + ZWF_SYMBOLS if s.endswith("set_avg")]  # every segment has weight 1
    assert pkg.lib().psdc_abi_version() == 3
    assert re.search(r"#define\s+PSDC_ABI_VERSION\s+3\b", hdr)
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "waterfall cascades" in hdr
    for text in ("Block b lives in ring slot b mod K", "[b B hop 8^k, ((b + 1) B - 1) hop 8^k + n 8^k)", "is NOT included",
                 "There is no set_avg", "exceeds 2^27 bytes", "OVERWRITES", "psd[r][k] = float32(S1[r][k] (double)gsc_r)"):  # (" * " is gone from `flat`)
        assert text in flat, text
    for cls in ("WaterfallCascadeBank", "WaterfallCascade", "ZoomWaterfallCascadeBank", "ZoomWaterfallCascade"):
        for m in ("process", "process_device", "set_detrend", "num_stages", "stage_blocks", "stage_rows", "image", "image_device",
                  "block_span", "recent_psd", "sync", "reset", "stats"):
            assert callable(getattr(getattr(pkg, cls), m)), (cls, m)
        assert not hasattr(getattr(pkg, cls), "set_avg")
    assert callable(pkg.ZoomWaterfallCascadeBank.set_carrier) and callable(pkg.ZoomWaterfallCascade.set_carrier)


def test_waterfall_supported(pkg):
    for n in (64, 128, 256, 512, 1024, 2048, 4096):
        assert pkg.waterfall_supported(n) and pkg.zoom_waterfall_supported(n), n
        assert pkg.waterfall_supported(n) == pkg.sk_supported(n) and pkg.zoom_waterfall_supported(n) == pkg.zoom_sk_supported(n)
    for n in (0, 32, 1000, 8192, 1 << 31):
        assert not pkg.waterfall_supported(n) and not pkg.zoom_waterfall_supported(n), n


@pytest.mark.parametrize("cls", ["WaterfallCascadeBank", "ZoomWaterfallCascadeBank"])
def test_waterfall_creation_errors(pkg, cls):
    """what creation refuses before it looks for a device: block < 2 and above 2^24, depth 0, a ring over 2^27 bytes (the text
    names the numbers), an unsupported n; null handles"""
    make = getattr(pkg, cls)
    tag = "psdc_wf" if cls == "WaterfallCascadeBank" else "psdc_zwf"
    rows = 2 if tag == "psdc_wf" else 4
    for block in (0, 1, (1 << 24) + 1):
        with pytest.raises(pkg.PsdError) as e:
            make(256, 1, block=block, depth=4)
        assert e.value.code == pkg.ERR_ARG and f"{tag}_create: block = {block}" in str(e.value) and "[2, 2^24]" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        make(256, 1, block=8, depth=0)
    assert e.value.code == pkg.ERR_ARG and "depth" in str(e.value)
    # n = 4096: 2049 bins; the largest depth that fits and the first that does not
    fit = (1 << 27) // (rows * 2049 * 8)
    with pytest.raises(pkg.PsdError) as e:
        make(4096, 1, block=8, depth=fit + 1)
    msg = str(e.value)
    assert e.value.code == pkg.ERR_ARG
    for number in (str(fit + 1), str(rows), "2049", str((fit + 1) * rows * 2049 * 8), str(1 << 27)):
        assert number in msg, (number, msg)
    for n in (32, 8192, 1000, 0):
        with pytest.raises(pkg.PsdError) as e:
            make(n, 1, block=8, depth=4)
        assert e.value.code == pkg.ERR_ARG and "n must be a power of two in [64, 4096]" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        make(256, 1, block=8, depth=4, window=pkg.WindowTable(np.ones(128, np.float32), 1.0, 1.0, 0))
    assert e.value.code == pkg.ERR_ARG
    L = pkg.lib()
    f = lambda name: getattr(L, tag + "_" + name)  # noqa: E731
    w = np.ones(256, np.float32)
    assert not f("create_window")(256, pkg._fptr(w), 1.0, 1.0, 0, 1, 1, 4, 0)
    assert f"{tag}_create_window: block = 1" in f("last_error")(None).decode()
    assert not f("create_window")(256, None, 1.0, 1.0, 0, 1, 8, 4, 0)
    assert "null window" in f("last_error")(None).decode()
    assert not f("create")(256, 7, 1, 8, 4, 0)
    assert "window_kind" in f("last_error")(None).decode()
    assert not f("create")(256, 1, 0, 8, 4, 0)
    assert "n_channels" in f("last_error")(None).decode()
    for rc in (f("process")(None, 0, None, 4), f("process_device")(None, 0, None, 4, None), f("sync")(None), f("reset")(None),
               f("set_detrend")(None, 0), f("num_stages")(None, 0), f("stage_blocks")(None, 0, 0, None),
               f("image")(None, 0, 0, 1, None, None, None, None, None), f("image_device")(None, 0, 0, 1, None, None, None, None, None),
               f("stats_read")(None, None, None, 0)):
        assert rc == pkg.ERR_ARG
    assert f"{tag}_stats_read: null handle" in f("last_error")(None).decode()
    f("destroy")(None)


def test_waterfall_no_gpu_fails_loudly(pkg):
    """Without a device create fails with ERR_DEVICE and says that there is no CPU path; with one it succeeds."""
    from conftest import has_gpu
    if has_gpu():
        pkg.WaterfallCascade(1024, block=4, depth=4).close()
        pkg.ZoomWaterfallCascade(1024, f0=0.2, block=4, depth=4).close()
        return
    for make in (lambda: pkg.WaterfallCascade(1024, block=4, depth=4), lambda: pkg.ZoomWaterfallCascade(1024, f0=0.2, block=4, depth=4)):
        with pytest.raises(pkg.PsdError) as e:
            make()
        assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)


def test_block_span(pkg):
    """the nominal time of a block: stage 0 blocks of B Hann segments start B hop apart and are (B - 1) hop + n long; a stage's
    spans are 8^stage times stage 0's; consecutive blocks share `overlap` (decimated) samples"""
    n, ov, B = 256, 128, 8
    s = pkg.waterfall_block_span(n, ov, B, 0, 0)
    assert (s.start, s.stop) == (0, 7 * 128 + 256)
    s = pkg.waterfall_block_span(n, ov, B, 0, 3)
    assert (s.start, s.stop) == (3 * 8 * 128, (4 * 8 - 1) * 128 + 256)
    t = pkg.waterfall_block_span(n, ov, B, 2, 3)
    assert (t.start, t.stop) == (64 * s.start, 64 * s.stop)
    a, b = pkg.waterfall_block_span(n, ov, B, 1, 4), pkg.waterfall_block_span(n, ov, B, 1, 5)
    assert a.stop - b.start == 8 * ov
    r = pkg.waterfall_block_span(1024, 0, 2, 0, 5)  # rectangular window: no overlap, blocks abut
    assert (r.start, r.stop) == (5 * 2048, 6 * 2048)


# ---- the host programs ----

_EXE = {}


def host_exe(tmp_dir, name, sanitize):
    key = (name, sanitize)
    if key not in _EXE:
        exe = os.path.join(str(tmp_dir), name + ("_san" if sanitize else ""))
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe], check=True)
        _EXE[key] = exe
    return _EXE[key]


@pytest.fixture(scope="session")
def wf_host_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("waterfall_host")


def run_host(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    assert "FAIL" not in r.stdout
    return r.stdout


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_waterfall_plan_check(wf_host_dir, sanitize):
    """csrc/waterfall_plan.h, exhaustively over s0 = 0 ... 40, s1 = s0 ... s0 + 40, B = 2 ... 9, K = 1 ... 5 and over sequences of
    three consecutive spans (tests/host/waterfall_plan_check.cpp; the program asserts)"""
    out = run_host(host_exe(wf_host_dir, "waterfall_plan_check", sanitize))
    assert int(re.search(r"waterfall_plan_check: (\d+) checks", out).group(1)) > 1_000_000


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_waterfall_emulation(wf_host_dir, sanitize):
    """csrc/waterfall_read.h: the ring-order map for started < K, = K, = K + 1 and = 3 K + 2, psd against (float)(s1 (double)gsc), sk
    against the f64 formula with its NaNs (tests/host/waterfall_emul.cpp)"""
    out = run_host(host_exe(wf_host_dir, "waterfall_emul", sanitize))
    for what in ("order started<K K=5", "order started=K K=5", "order started=K+1 K=5", "order started=3K+2 K=5 started=17 valid=5",
                 "psd 200000 elements bit-equal", "sk 200000 elements", "sk NaN at count<2 and S1==0"):
        assert what in out, what


# ---- the restatements are anchored ----

@pytest.mark.parametrize("n,window,detrend,block,length", [
    (64, "hann", "none", 4, 200 * 64),
    (256, "rect", "mean", 3, 40_017),
    (128, "hann", "span", 7, 30_000),
])
def test_restatement_sums_to_restate_sk(ora, n, window, detrend, block, length):
    """summed over all blocks a stage's rows are restate_sk's with default averaging (1e-12 relative); every block but the newest
    holds B segments, the newest the rest; stages, segments and pendings are restate_sk's"""
    x = gaussian(length, n + block)
    wf = restate_waterfall(ora, x, n, block, window, detrend)
    sk = restate_sk(ora, x, n, window, detrend)
    assert len(wf) == len(sk) >= 3
    for k, (w, s) in enumerate(zip(wf, sk)):
        assert (w["segs"], w["pending"]) == (s["count"], s["pending"]), k
        assert [b["index"] for b in w["blocks"]] == list(range(len(w["blocks"]))) and len(w["blocks"]) == -(-s["count"] // block)
        assert [b["count"] for b in w["blocks"][:-1]] == [block] * (len(w["blocks"]) - 1)
        if w["blocks"]:
            assert w["blocks"][-1]["count"] == s["count"] - block * (len(w["blocks"]) - 1)
        for name in WF_ROWS:
            tot = sum(b[name] for b in w["blocks"]) if w["blocks"] else np.zeros(n // 2 + 1)
            assert np.all(np.abs(tot - s[name]) <= 1e-12 * np.abs(s[name])), (k, name)
    # the f32 sibling has the same bookkeeping and f32 rows
    w32 = restate_waterfall(ora, x, n, block, window, detrend, "f32", max_stages=2)
    assert [len(s["blocks"]) for s in w32] == [len(s["blocks"]) for s in wf[:2]]
    assert w32[0]["blocks"][0]["s1"].dtype == np.float32
    assert np.allclose(w32[0]["blocks"][0]["s1"], wf[0]["blocks"][0]["s1"], rtol=1e-4, atol=1e-6 * wf[0]["blocks"][0]["s1"].max())


@pytest.mark.parametrize("n,window,detrend,block,length", [
    (64, "hann", "none", 4, 200 * 64),
    (256, "rect", "mean", 5, 30_000),
])
def test_zoom_restatement_sums_to_restate_zoom_sk(pkg, ora, n, window, detrend, block, length):
    x = gaussian(length, n + block)
    ftw = pkg.zoom_ftw(0.23)[0]
    wf = restate_zoom_waterfall(ora, x, n, ftw, block, window, detrend)
    sk = restate_zoom_sk(ora, x, n, ftw, 0, window, detrend)
    assert len(wf) == len(sk) >= 3
    for k, (w, s) in enumerate(zip(wf, sk)):
        assert (w["segs"], w["pending"]) == (s["count"], s["pending"]), k
        assert [b["count"] for b in w["blocks"][:-1]] == [block] * (len(w["blocks"]) - 1)
        assert sum(b["count"] for b in w["blocks"]) == s["count"]
        for name in ZWF_ROWS:
            tot = sum(b[name] for b in w["blocks"]) if w["blocks"] else np.zeros(n // 2 + 1)
            assert np.all(np.abs(tot - s[name]) <= 1e-12 * np.abs(s[name])), (k, name)


def test_ring_of():
    st = dict(blocks=[dict(index=i) for i in range(7)])
    assert [b["index"] for b in ring_of(st, 3)] == [4, 5, 6] and [b["index"] for b in ring_of(st, 64)] == list(range(7))
    assert ring_of(dict(blocks=[]), 4) == []


# ---- the tone-switch property on the f64 restatement ----

_TONE = {}


def tone_restatement(ora):
    if "st" not in _TONE:
        x, half = tone_input()
        _TONE["st"] = restate_waterfall(ora, x, TONE_N, TONE_B, max_stages=1)[0]
    return _TONE["st"]


def test_restatement_tone_switch(pkg, ora):
    """the restatement stays inside the bound the GPU is held to: every block wholly in one half peaks at that half's bin, at most 2
    blocks touch the switch"""
    x, half = tone_input()
    st = tone_restatement(ora)
    assert len(st["blocks"]) == TONE_BLOCKS and st["blocks"][-1]["count"] == TONE_B
    left = check_tone_switch(pkg, [b["index"] for b in st["blocks"]], [b["s1"] for b in st["blocks"]], half, x.size)
    assert 1 <= len(left) <= 2
