"""Integer sample feeds on the GPU (psdc_int_*, csrc/sample_int.hip).  Semantics: include/psdcascade.h, "integer sample feeds".

The yardstick is exact: an integer call gives the bits of the object's existing f32 call of the same length (plain for the real
objects, interleaved for the complex ones) fed float32(v) * float32(scale), on the same object state and from the same memory
side.  Every test but the absolute anchor compares bytes: psd() / csd(), every stage's raw rows and every stage's stats."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_iq import assert_bits as assert_bits_1, bits as bits_1
from test_gpu_iq_cross import assert_bits as assert_bits_2, bits as bits_2
from test_iq_host import mix_c_f64
from test_zoom_host import restate_zoom, stitch_zoom

pytestmark = pytest.mark.gpu

N = 64
OBJECTS = ("zoom", "zcsd", "iq", "iqcsd")
KINDS = (np.int16, np.int8)
LENS = [1, 2, 5, 64, 251, 1024, 4099, 3]  # the destination head takes every value 0 ... 3
# units the source of call k is offset by, side a and side b: the calls of 64 and 1024 units read whole groups with one load
# on side a, the others element-wise; side b differs from side a, so a pair's sources are judged each on its own
OFFS_A = [0, 1, 2, 0, 3, 0, 1, 2]
OFFS_B = [1, 0, 0, 0, 0, 2, 1, 0]
ODD_SCALE = 3.0517578e-5 * 1.2345678  # not a power of two
FTW_A, PH_A = 0x3C6EF372FE94F82B, 0x9E3779B97F4A7C15
FTW_B, PH_B = 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9
# (ftw, phase0) of side a and side b; a single object takes side a's
CARRIERS = {"none": ((0, 0), (0, 0)), "carrier": ((FTW_A, PH_A), (FTW_B, PH_B)), "shared": ((FTW_A, PH_A), (FTW_A, PH_A))}


def is_pair(obj):
    return obj in ("zcsd", "iqcsd")


def is_complex(obj):
    return obj in ("iq", "iqcsd")


def carriers_of(obj):
    return ("none", "carrier", "shared") if is_pair(obj) else ("none", "carrier")


def make(pkg, obj, carrier, n=N):
    cls = {"zoom": pkg.ZoomCascadeBank, "zcsd": pkg.ZoomCsdCascadeBank, "iq": pkg.IqCascadeBank, "iqcsd": pkg.IqCsdCascadeBank}[obj]
    b = cls(n, 1)
    (fa, pa), (fb, pb) = CARRIERS[carrier]
    if is_pair(obj):
        b.set_carrier(0, ftw=fa, phase0=pa, side=0)
        b.set_carrier(0, ftw=fb, phase0=pb, side=1)
    else:
        b.set_carrier(0, ftw=fa, phase0=pa)
    return b


def stream(obj, dtype, length, seed):
    """the integer units of every side of one object: [side] -> (length,) or (length, 2), full range, the extremes included"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    out = []
    for _ in range(2 if is_pair(obj) else 1):
        v = rng.integers(info.min, info.max + 1, size=(length, 2) if is_complex(obj) else (length,)).astype(dtype)
        flat = v.reshape(-1)
        flat[::17], flat[5::19], flat[3::23], flat[7::29] = info.min, info.max, 0, -1
        out.append(v)
    return out


def converted(v, scale):
    """float32(v) * float32(scale): the stream the f32 call is fed -- f32 samples, or complex64 for (re, im) rows"""
    f = v.astype(np.float32) * np.float32(scale)
    assert f.dtype == np.float32
    return f if v.ndim == 1 else np.ascontiguousarray(f).view(np.complex64).reshape(-1)


def default_scale(pkg, dtype):
    return pkg.sample_kind(dtype)[1]


def bits(obj, bank):
    return bits_2(bank) if is_pair(obj) else bits_1(bank)


def assert_bits(obj, a, b, what):
    (assert_bits_2 if is_pair(obj) else assert_bits_1)(a, b, what)


class DeviceStreams:
    """every side's units in device memory, once behind each offset 0 ... 3 (so a call's source can start at any position of a
    group), and the converted f32 / complex64 stream beside them"""

    def __init__(self, pkg, sides, scale):
        import torch
        self.unit = sides[0].itemsize * (2 if sides[0].ndim == 2 else 1)
        self.ints = []
        for v in sides:
            per_off = []
            for off in range(4):
                padded = np.concatenate([np.zeros((off,) + v.shape[1:], v.dtype), v])
                per_off.append(torch.from_numpy(padded).cuda())
            self.ints.append(per_off)
        self.f32 = [torch.from_numpy(converted(v, scale)).cuda() for v in sides]
        self.f32_unit = self.f32[0].element_size()
        torch.cuda.synchronize()

    def int_ptr(self, side, off, start):
        t = self.ints[side][off]
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + (off + start) * self.unit

    def f32_ptr(self, side, start):
        return self.f32[side].data_ptr() + start * self.f32_unit


def feed_int_device(pkg, obj, bank, dev, dtype, scale, start, length, off_a, off_b):
    kind = pkg.sample_kind(dtype)[0]
    if is_pair(obj):
        bank.process_int_device(0, dev.int_ptr(0, off_a, start), dev.int_ptr(1, off_b, start), length, kind, scale)
    else:
        bank.process_int_device(0, dev.int_ptr(0, off_a, start), length, kind, scale)


def feed_f32_device(obj, bank, dev, start, length):
    if is_pair(obj):
        bank.process_device(0, dev.f32_ptr(0, start), dev.f32_ptr(1, start), length)
    else:
        bank.process_device(0, dev.f32_ptr(0, start), length)


def feed_int_host(obj, bank, sides, scale, s, e):
    if is_pair(obj):
        bank.process_int(0, sides[0][s:e], sides[1][s:e], scale)
    else:
        bank.process_int(0, sides[0][s:e], scale)


def feed_f32_host(obj, bank, conv, s, e):
    if is_pair(obj):
        bank.process(0, conv[0][s:e], conv[1][s:e])
    else:
        bank.process(0, conv[0][s:e])


def cuts_of(lens):
    c = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    return list(zip(c[:-1].tolist(), c[1:].tolist()))


def run_device(pkg, obj, dtype, carrier, scale, sides, lens=LENS):
    """(bits of the integer-fed object, bits of the f32-fed object), both fed the same calls from device memory"""
    dev = DeviceStreams(pkg, sides, scale)
    gi, gf = make(pkg, obj, carrier), make(pkg, obj, carrier)
    for k, (s, e) in enumerate(cuts_of(lens)):
        feed_int_device(pkg, obj, gi, dev, dtype, scale, s, e - s, OFFS_A[k % 8], OFFS_B[k % 8])
        feed_f32_device(obj, gf, dev, s, e - s)
    out = bits(obj, gi), bits(obj, gf)  # (a read-out syncs: the device memory may go after it)
    assert gi.stats_read() == gf.stats_read()
    return out


CASES = [(o, k, c) for o in OBJECTS for k in KINDS for c in carriers_of(o)]


@pytest.mark.parametrize("obj,dtype,carrier", CASES, ids=[f"{o}-{np.dtype(k).name}-{c}" for o, k, c in CASES])
def test_int_equals_f32_from_device_memory(pkg, gpu_required, obj, dtype, carrier):
    """Two objects in the same fresh state, one fed integer calls and one the f32 call of float32(v) * float32(scale), with the
    call lengths 1, 2, 5, 64, 251, 1024, 4099, 3 and the sources offset by 0 ... 3 units: equal bytes everywhere."""
    scale = default_scale(pkg, dtype)
    sides = stream(obj, dtype, sum(LENS), 11)
    a, b = run_device(pkg, obj, dtype, carrier, scale, sides)
    assert_bits(obj, a, b, f"{obj} {np.dtype(dtype).name} {carrier}: integer against f32 calls")
    assert len(a[1]) >= 2  # more than one stage holds data


@pytest.mark.parametrize("obj", OBJECTS)
@pytest.mark.parametrize("dtype", KINDS, ids=["int16", "int8"])
def test_scale_and_extremes(pkg, gpu_required, obj, dtype):
    """Streams of the extremes alone (-32768, 32767, -128, 127, 0 and -1, whichever the type holds) with a scale that is no power
    of two, so the product rounds: equal bytes with the f32 calls of the rounded products."""
    info = np.iinfo(dtype)
    values = np.array([v for v in (-32768, 32767, -128, 127, 0, -1) if info.min <= v <= info.max], dtype)
    length = sum(LENS)
    sides = []
    for side in range(2 if is_pair(obj) else 1):
        flat = values[np.random.default_rng(57 + side).integers(0, values.size, length * (2 if is_complex(obj) else 1))]
        sides.append(np.ascontiguousarray(flat.reshape(length, 2) if is_complex(obj) else flat))
    for v in values:
        assert np.any(sides[0] == v)
    prod = converted(sides[0], ODD_SCALE)
    assert np.any(prod.view(np.float32).astype(np.float64) != sides[0].reshape(-1).astype(np.float64) * ODD_SCALE)  # the product rounds
    a, b = run_device(pkg, obj, dtype, "carrier", ODD_SCALE, sides)
    assert_bits(obj, a, b, f"{obj} {np.dtype(dtype).name}: extremes at scale {ODD_SCALE!r}")


@pytest.mark.parametrize("obj", OBJECTS)
@pytest.mark.parametrize("dtype", KINDS, ids=["int16", "int8"])
def test_host_route_equals_device_route(pkg, gpu_required, obj, dtype):
    """The same integer calls from host arrays (sliced, so the host pointers sit at every unit offset too) give the bytes of the
    device calls, and so of the f32 calls."""
    scale = ODD_SCALE
    sides = stream(obj, dtype, sum(LENS), 23)
    a, b = run_device(pkg, obj, dtype, "carrier", scale, sides)
    gh, gf = make(pkg, obj, "carrier"), make(pkg, obj, "carrier")
    conv = [converted(v, scale) for v in sides]
    for s, e in cuts_of(LENS):
        feed_int_host(obj, gh, sides, scale, s, e)
        feed_f32_host(obj, gf, conv, s, e)
    h = bits(obj, gh)
    assert_bits(obj, h, a, f"{obj}: host integer calls against device integer calls")
    assert_bits(obj, h, bits(obj, gf), f"{obj}: host integer calls against host f32 calls")
    assert_bits(obj, h, b, f"{obj}: host integer calls against device f32 calls")


@pytest.mark.parametrize("obj", OBJECTS)
def test_host_call_across_a_staging_piece(pkg, gpu_required, obj):
    """One host call of 2^22 + 5 units is two pieces (2^22 and 5) on the integer route as on the f32 route: equal bytes, and the
    same launches"""
    length = (1 << 22) + 5
    dtype = np.int16
    scale = default_scale(pkg, dtype)
    sides = stream(obj, dtype, length, 31)
    gi, gf = make(pkg, obj, "carrier"), make(pkg, obj, "carrier")
    feed_int_host(obj, gi, sides, scale, 3, 3 + 100)  # a short call first: the long one starts off the 16-byte grid
    feed_int_host(obj, gi, sides, scale, 0, length)
    conv = [converted(v, scale) for v in sides]
    feed_f32_host(obj, gf, conv, 3, 3 + 100)
    feed_f32_host(obj, gf, conv, 0, length)
    assert_bits(obj, bits(obj, gi), bits(obj, gf), f"{obj}: a host call of 2^22 + 5 units")
    assert gi.stats_read() == gf.stats_read()


def adcdac_frames(pkg, batches, nframes, seed):
    words = np.random.default_rng(seed).integers(-32768, 32768, size=(4, 8 * batches * nframes)).astype(np.int16)
    return pkg.make_adcdac_frames(words, batches, seq0=3)


@pytest.mark.parametrize("obj", ["zoom", "iq"])
def test_routes_mix(pkg, gpu_required, obj):
    """An f32 call, an integer call, a frames call and another integer call on one channel against f32, f32 (the converted
    samples), the same frames, f32 on a second object: the stream index, and so the phase, runs through all of them."""
    dtype = np.int16
    scale = ODD_SCALE
    la, lb, lc = 1001, 2049, 777  # odd lengths: every later call starts off the 16-byte grid
    first = stream(obj, np.int16, la, 41)[0]
    ints = stream(obj, dtype, lb + lc, 43)[0]
    data, fs = adcdac_frames(pkg, 4, 25, 47)
    traces = ["ADC0"] if obj == "zoom" else [("ADC0", "DAC1")]
    conv0, conv = converted(first, 2.0 ** -15), converted(ints, scale)
    g, twin = make(pkg, obj, "carrier"), make(pkg, obj, "carrier")
    g.process(0, conv0)
    g.process_int(0, ints[:lb], scale)
    assert g.process_frames(data, fs, traces) == 25
    g.process_int(0, ints[lb:], scale)
    twin.process(0, conv0)
    twin.process(0, conv[:lb])
    assert twin.process_frames(data, fs, traces) == 25
    twin.process(0, conv[lb:])
    assert_bits(obj, bits(obj, g), bits(obj, twin), f"{obj}: f32, integer, frames, integer")
    assert g.stats_read() == twin.stats_read()
    assert g.stats_read()["samples_in"] == la + lb + lc + 25 * 4 * 8


@pytest.mark.parametrize("obj", ["zoom", "iq"])
def test_absolute_anchor(pkg, ora, gpu_required, obj):
    """An integer-fed object at N = 1024 on 3 x 10^5 noise samples quantised to int16, against the f64 restatement of the zoom and
    IQ tests fed the converted samples, within their bound (assert_psd_close(pure=True): 1e-5 on every bin)."""
    n, length = 1024, 300_000
    rng = np.random.default_rng(53)
    shape = (length, 2) if obj == "iq" else (length,)
    v = np.clip(np.rint(rng.standard_normal(shape) * 6000.0), -32768, 32767).astype(np.int16)
    scale = default_scale(pkg, np.int16)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    if obj == "zoom":
        g = pkg.ZoomCascade(n, ftw=ftw)
        g.process_int(v)
        x = converted(v, scale)
        stages = restate_zoom(ora, x, n, ftw)
    else:
        g = pkg.IqCascade(n, ftw=ftw)
        g.process_int(v)
        z = converted(v, scale)
        i, q = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        stages = restate_zoom(ora, i, n, ftw, iq=mix_c_f64(i, q, ftw))
    up, lo, br = g.psd()
    rup, rlo, rbr = stitch_zoom(pkg, n, pkg.Window.HANN, stages)
    assert br == rbr
    for name, got, want in (("upper", up, rup), ("lower", lo, rlo)):
        rel = assert_psd_close(got, want, f"integer-fed {obj} {name}", pure=True)
        print(f"integer-fed {obj} {name}: worst relative error {rel:.3g}")


LAST_ERROR = {"zoom": "psdc_zoom_last_error", "zcsd": "psdc_zcsd_last_error", "iq": "psdc_iq_last_error", "iqcsd": "psdc_iqcsd_last_error"}


@pytest.mark.parametrize("obj", OBJECTS)
def test_errors_leave_the_object_unchanged(pkg, gpu_required, obj):
    """Unknown kind, a misaligned pointer for each kind, NULL with len > 0, a non-finite scale and an out-of-range channel or pair
    are PSDC_ERR_ARG with a text that names the call; len == 0 is OK; and the object is as it was: the calls that follow give the
    yardstick's bytes."""
    L = pkg.lib()
    dtype = np.int16
    scale = default_scale(pkg, dtype)
    sides = stream(obj, dtype, sum(LENS), 61)
    dev = DeviceStreams(pkg, sides, scale)
    g, twin = make(pkg, obj, "carrier"), make(pkg, obj, "carrier")
    host = np.zeros(64, np.int16)
    hp = host.ctypes.data
    dp = dev.int_ptr(0, 0, 0)
    S16, S8 = int(pkg.SampleKind.S16), int(pkg.SampleKind.S8)
    unit = {k: (2 if is_complex(obj) else 1) * b for k, b in ((S16, 2), (S8, 1))}

    def call(device, ptr, kind, sc, length, unit_index=0, ptr_b=None):
        fn = getattr(L, f"psdc_int_{obj}_process" + ("_device" if device else ""))
        args = [g._h, unit_index, C.c_void_p(ptr)]
        if is_pair(obj):
            args.append(C.c_void_p(ptr if ptr_b is None else ptr_b))
        args += [kind, C.c_float(sc), length]
        if device:
            args.append(None)
        return fn(*args), f"psdc_int_{obj}_process" + ("_device" if device else "")

    def refused(rc_name, *words):
        rc, name = rc_name
        assert rc == pkg.ERR_ARG, (name, rc)
        msg = getattr(L, LAST_ERROR[obj])(g._h).decode()
        assert msg.startswith(name + ": "), msg
        for w in words:
            assert w in msg, msg

    def run_calls(lo, hi):
        for k, (s, e) in list(enumerate(cuts_of(LENS)))[lo:hi]:
            feed_int_device(pkg, obj, g, dev, dtype, scale, s, e - s, OFFS_A[k], OFFS_B[k])
            feed_f32_device(obj, twin, dev, s, e - s)

    run_calls(0, 4)
    before = g.stats_read()
    for device, base in ((False, hp), (True, dp)):
        refused(call(device, base, 0, scale, 8), "unknown sample kind")
        refused(call(device, base, 3, scale, 8), "unknown sample kind")
        refused(call(device, base, -1, scale, 8), "unknown sample kind")
        for kind in (S16, S8):
            for off in range(1, unit[kind]):  # every address that is not a multiple of the unit
                refused(call(device, base + off, kind, scale, 8), "not aligned", f"{unit[kind]} bytes")
            if is_pair(obj) and unit[kind] > 1:  # side b alone off the grid
                refused(call(device, base, kind, scale, 8, ptr_b=base + 1), "not aligned")
            assert call(device, base + unit[kind], kind, scale, 0)[0] == 0  # len == 0 is OK
        refused(call(device, 0, S16, scale, 8), "null sample pointer")
        if is_pair(obj):
            refused(call(device, base, S16, scale, 8, ptr_b=0), "null sample pointer")
        assert call(device, 0, S16, scale, 0)[0] == 0
        for bad in (float("nan"), float("inf"), float("-inf")):
            refused(call(device, base, S16, bad, 8), "scale", "finite")
        refused(call(device, base, S16, scale, 8, unit_index=1), "out of range")
    assert g.stats_read() == before
    run_calls(4, 8)
    assert_bits(obj, bits(obj, g), bits(obj, twin), f"{obj}: a valid sequence around refused calls")
    assert g.stats_read() == twin.stats_read()


@pytest.mark.parametrize("obj", OBJECTS)
@pytest.mark.parametrize("dtype", KINDS, ids=["int16", "int8"])
def test_launches_are_those_of_the_f32_call(pkg, gpu_required, obj, dtype):
    """Steady calls of one length: every integer call reports through stats_read the launches of the f32 call"""
    length, calls = 4096, 6
    scale = default_scale(pkg, dtype)
    sides = stream(obj, dtype, length * calls, 71)
    dev = DeviceStreams(pkg, sides, scale)
    gi, gf = make(pkg, obj, "carrier"), make(pkg, obj, "carrier")
    per_call = []
    for k in range(calls):
        feed_int_device(pkg, obj, gi, dev, dtype, scale, k * length, length, 0, 0)
        feed_f32_device(obj, gf, dev, k * length, length)
        si, sf = gi.stats_read(reset=True), gf.stats_read(reset=True)
        assert si == sf, (k, si, sf)
        per_call.append(si["launches"])
    gi.sync(), gf.sync()
    print(f"{obj} {np.dtype(dtype).name}: launches a call {per_call}")
    assert per_call[-1] == per_call[-2] > 0
    assert per_call[-1] <= (pkg.ZCSD_STEADY_LAUNCHES if obj == "zcsd" else 4)  # 2 + 3 for zoom cross, 1 + 3 for the others


def test_cli_reads_integer_files(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --sample-format s16 on raw integer files: --iq and --zoom print what the objects give for one process_int
    call of the same integers (the streams are shorter than the tool's 2^20 units a call, so the calls coincide), at the tool's
    print precision; --scale reaches the feed; the pair options run; the f32 default refuses --scale."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = [sys.executable, os.path.join(root, "tools", "psd_cli.py")]
    length = (1 << 16) + 77
    za, zb = stream("iqcsd", np.int16, length, 83)
    xa, xb = stream("zcsd", np.int16, length, 89)
    paths = {}
    for name, v in (("za", za), ("zb", zb), ("xa", xa), ("xb", xb)):
        paths[name] = str(tmp_path / f"{name}.s16")
        v.astype("<i2").tofile(paths[name])
    scale = 2.0 ** -12
    r = subprocess.run(cli + ["--sample-format", "s16", "--scale", repr(scale), "--iq", paths["za"] + ":0.2", "--zoom", "0.3:" + paths["xa"],
                              "--iq-pair", paths["za"] + ":" + paths["zb"], "--zoom-pair", "0.1:" + paths["xa"] + ":" + paths["xb"],
                              "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for label in ("iq za.s16 @ 0.2", "zoom xa.s16 @ 0.3", "iq pair za.s16:zb.s16 @ 0", "zoom pair xa.s16:xb.s16 @ 0.1"):
        assert label in r.stdout, r.stdout
    for name, cls, f0, v in (("iq_za_s16_0_2.csv", pkg.IqCascadeBank, 0.2, za), ("zoom_xa_s16_0_3.csv", pkg.ZoomCascadeBank, 0.3, xa)):
        d = np.loadtxt(tmp_path / "csv" / name, delimiter=",")
        bank = cls(512, 1)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
        bank.set_detrend(pkg.Detrend.MEAN)
        bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
        bank.set_carrier(0, f0=f0)
        bank.process_int(0, v, scale)
        up, lo, br = bank.psd(0)
        assert d.shape == (up.size, 3)
        assert np.allclose(d[:, 0], pkg.Break.frequencies(br), rtol=1e-6, atol=0)
        assert np.allclose(d[:, 1], up, rtol=2e-8, atol=0) and np.allclose(d[:, 2], lo, rtol=2e-8, atol=0), name
    for name, cols in (("iqpair_za_s16__zb_s16_0.csv", 9), ("zoompair_xa_s16__xb_s16_0_1.csv", 9)):
        d = np.loadtxt(tmp_path / "csv" / name, delimiter=",")
        assert d.ndim == 2 and d.shape[1] == cols and np.all(d[:, 1] > 0)
    r = subprocess.run(cli + ["--scale", "2", "--iq", paths["za"] + ":" + paths["zb"]], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--sample-format" in r.stderr
