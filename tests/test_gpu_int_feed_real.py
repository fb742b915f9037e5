"""Integer sample feeds of the real-input objects on the GPU (psdc_sint_*, sample_cvt_int_kernel of csrc/sample_int.hip).
Semantics: include/psdcascade.h, "integer sample feeds of the real-input objects".

The yardstick is exact wherever the header promises bits: an integer call of the pair or the matrix object gives the bytes of the f32
call of float32(v) * float32(scale) from the same memory side; a PSD stream fed with one (kind, scale) gives the bytes of
psdc_process in the same call sizes.  Where kinds change inside a quantum, and on the device route of the PSD object, the
project's existing bounds apply unchanged (conftest.assert_psd_close with its defaults, the f64 oracle)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

KINDS = (np.int16, np.int8)
CUTS = [1, 3, 5, 1000, 4099]  # then the rest
TOTAL = 70_003
ODD_SCALE = 3.0e-3
# integers the source of call k of channel c is offset by: (OFFS[k] + 3 c) % 8 -- group-aligned for some channels and calls (one
# wide load a group), not for others (element-wise), and different from channel to channel
OFFS = [0, 1, 4, 3, 0, 5, 2]


def default_scale(pkg, dtype):
    return pkg.sample_kind(dtype)[1]


def converted(v, scale):
    f = v.astype(np.float32) * np.float32(scale)
    assert f.dtype == np.float32
    return f


def cuts_of(lens, total):
    edges = np.concatenate([[0], np.cumsum(lens), [total]])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def int_streams(dtype, m, length, seed, cuts=(), tone=True):
    """m integer streams: noise over the full range (a tone on top), the extremes sprinkled in and, with cuts, at the head and
    tail positions of every call"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    out = []
    for c in range(m):
        v = rng.normal(0.0, info.max / 6.0, length)
        if tone:
            v += info.max / 4.0 * np.sin(2 * np.pi * (0.05 + 0.01 * c) * np.arange(length))
        v = np.clip(np.round(v), info.min, info.max).astype(dtype)
        v[11::97], v[5::89], v[3::83], v[7::79] = info.min, info.max, 0, -1
        ext = [info.min, info.max, -1, 0, 1]
        for a, b in cuts:
            for k in range(min(5, b - a)):
                v[a + k] = ext[(k + c) % 5]
                v[b - 1 - k] = ext[(k + c + 2) % 5]
        out.append(v)
    return out


class Sources:
    """every channel's integers in host and in device memory, once behind each offset 0 ... 7 so that a call's source can start at
    any offset from a group boundary, and the converted f32 streams beside them"""

    def __init__(self, streams, scale):
        import torch
        self.itemsize = streams[0].itemsize
        self.f32 = [converted(v, scale) for v in streams]
        self.dev_f32 = [torch.from_numpy(f).cuda() for f in self.f32]
        # one shifted copy per offset: a call that wants its source `off` integers past a group boundary reads the copy shifted by off
        self.host_sh = [[np.concatenate([np.zeros(off, v.dtype), v]) for off in range(8)] for v in streams]
        self.dev_sh = [[torch.from_numpy(h).cuda() for h in per] for per in self.host_sh]
        torch.cuda.synchronize()

    def host_int(self, c, off, a, b):
        return self.host_sh[c][off][off + a:off + b]

    def dev_int(self, c, off, a):
        t = self.dev_sh[c][off]
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + (off + a) * self.itemsize

    def dev_f(self, c, a):
        return self.dev_f32[c].data_ptr() + 4 * a


def off_of(k, c):
    return (OFFS[k % len(OFFS)] + 3 * c) % 8


def make_x(pkg, kind, n, m):
    return pkg.CsdCascadeBank(n, 1) if kind == "pair" else pkg.CsmCascadeBank(n, m, 1)


def feed_x(pkg, kind, bank, src, dtype, scale, device, ints, k, a, b):
    """call k: samples [a, b) of every channel into unit 0, as integers or as the converted f32, from host or device memory"""
    m = len(src.f32)
    sk = pkg.sample_kind(dtype)[0]
    if ints and not device:
        xs = [src.host_int(c, off_of(k, c), a, b) for c in range(m)]
        bank.process_int(0, xs[0], xs[1], scale) if kind == "pair" else bank.process_int(0, xs, scale)
    elif ints:
        ps = [src.dev_int(c, off_of(k, c), a) for c in range(m)]
        bank.process_int_device(0, ps[0], ps[1], b - a, sk, scale) if kind == "pair" else bank.process_int_device(0, ps, b - a, sk, scale)
    elif not device:
        xs = [src.f32[c][a:b] for c in range(m)]
        bank.process(0, xs[0], xs[1]) if kind == "pair" else bank.process(0, xs)
    else:
        ps = [src.dev_f(c, a) for c in range(m)]
        bank.process_device(0, ps[0], ps[1], b - a) if kind == "pair" else bank.process_device(0, ps, b - a)


def xbits(bank, unit=0):
    """csd() and every stage's stats and raw rows of one pair / group"""
    return bank.csd(unit), [bank.stage_spectra(unit, k) for k in range(bank.num_stages(unit))]


def same(a, b, what):
    if isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for k, (p, q) in enumerate(zip(a, b)):
            same(p, q, f"{what}[{k}]")
    else:
        assert a == b, (what, a, b)


X_OBJECTS = [("pair", 64, 2), ("pair", 256, 2), ("matrix", 64, 3), ("matrix", 256, 4)]


@pytest.mark.parametrize("kind,n,m", X_OBJECTS, ids=[f"{k}{n}x{m}" for k, n, m in X_OBJECTS])
@pytest.mark.parametrize("dtype", KINDS, ids=["int16", "int8"])
def test_pair_and_matrix_bits(pkg, gpu_required, kind, n, m, dtype):
    """One stream cut into calls of 1, 3, 5, 1000, 4099 units and the rest, sources at offsets that differ from channel to channel,
    from host and from device memory: every stage's rows and stats, and csd(), equal the f32 twin's byte for byte.  Again with a
    scale that is no power of two, the extremes at the head and tail positions of every call, and a leading call of 2 units (so
    that the destination starts at the other two positions of a 16-byte group)."""
    for scale, lens in ((None, CUTS), (ODD_SCALE, [2] + CUTS)):
        cuts = cuts_of(lens, TOTAL)
        sc = default_scale(pkg, dtype) if scale is None else scale
        src = Sources(int_streams(dtype, m, TOTAL, 100 + n + m, cuts if scale else ()), sc)
        for device in (False, True):
            g, twin = make_x(pkg, kind, n, m), make_x(pkg, kind, n, m)
            for k, (a, b) in enumerate(cuts):
                feed_x(pkg, kind, g, src, dtype, scale, device, True, k, a, b)
                feed_x(pkg, kind, twin, src, dtype, sc, device, False, k, a, b)
            assert g.num_stages(0) >= 3
            same(xbits(g), xbits(twin), f"{kind} n={n} m={m} {np.dtype(dtype).name} scale={scale} device={device}")
            g.close(), twin.close()


def test_pair_across_a_staging_piece(pkg, gpu_required):
    """one host call of 2^22 + 5 units: two pieces through the pinned staging, the second one of 5 units"""
    total = (1 << 22) + 5
    x, y = int_streams(np.int16, 2, total, 7, tone=False)
    sc = default_scale(pkg, np.int16)
    g, twin = pkg.CsdCascadeBank(64, 1), pkg.CsdCascadeBank(64, 1)
    g.process_int(0, x, y)
    twin.process(0, converted(x, sc), converted(y, sc))
    assert g.stats_read()["launches"] == twin.stats_read()["launches"] + 2  # one converter a piece
    same(xbits(g), xbits(twin), "2^22 + 5 units")
    g.close(), twin.close()


def test_routes_mix_on_one_pair(pkg, ora, gpu_required):
    """an f32 call, an integer call, an AdcDac frames call and an integer call of the other kind on one pair, against an all-f32 twin"""
    n, batches, nframes = 256, 4, 300
    rng = np.random.default_rng(5)
    raw = np.clip(np.round(rng.standard_normal((4, nframes * batches * 8)) * 3000), -32768, 32767).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(raw, batches, seq0=3)
    lsb = np.float32(4.096) * np.float32(2.5) / np.float32(32768)
    tr = [raw[c].astype(np.float32) * lsb for c in range(2)]
    st, _, nb, dec = ora.adcdac_decode(bytes(data[:fs]))  # the oracle's decode of the first frame, held against the line above
    assert st == 0 and nb == batches and all(np.array_equal(dec[c], tr[c][:batches * 8]) for c in range(2))
    f = [np.random.default_rng(9 + c).standard_normal(5001).astype(np.float32) for c in range(2)]
    a16, a8 = int_streams(np.int16, 2, 7003, 21), int_streams(np.int8, 2, 9001, 22)
    s16, s8 = default_scale(pkg, np.int16), ODD_SCALE
    g, twin = pkg.CsdCascadeBank(n, 1), pkg.CsdCascadeBank(n, 1)
    g.process(0, f[0], f[1])
    g.process_int(0, a16[0][1:-1], a16[1][2:])
    assert g.process_frames(data, fs, [(0, 1)]) == nframes
    g.process_int(0, a8[0][3:], a8[1][:-3], s8)
    twin.process(0, f[0], f[1])
    twin.process(0, converted(a16[0][1:-1], s16), converted(a16[1][2:], s16))
    twin.process(0, tr[0], tr[1])
    twin.process(0, converted(a8[0][3:], s8), converted(a8[1][:-3], s8))
    same(xbits(g), xbits(twin), "f32, s16, frames, s8 on one pair")
    g.close(), twin.close()


def psd_bits(bank, channel):
    ns = bank.num_stages(channel)
    return (bank.psd(channel), [bank.stage_info(channel, k) for k in range(ns)], [bank.stage_spectrum(channel, k) for k in range(ns)],
            [bank.stage_buf(channel, k) for k in range(ns)])


PSD_LENS = [1, 511, 4095, 4097, 20000]


@pytest.mark.parametrize("n,nch", [(256, 2), (64, 1)], ids=["fused256x2", "generic64"])
@pytest.mark.parametrize("dtype", KINDS, ids=["int16", "int8"])
def test_psd_host_bits(pkg, gpu_required, n, nch, dtype):
    """quantum 4096: integer calls of 1, 511, 4095, 4097 and 20 000 units on every channel against process of the converted
    stream in the same calls -- the stage spectra, stats, pending samples and psd() are the same bytes"""
    total = sum(PSD_LENS)
    for scale in (None, ODD_SCALE):
        sc = default_scale(pkg, dtype) if scale is None else scale
        xs = int_streams(dtype, nch, total + 8, 300 + n)
        g, twin = pkg.PsdCascadeBank(n, nch), pkg.PsdCascadeBank(n, nch)
        g.configure(quantum=4096), twin.configure(quantum=4096)
        for k, (a, b) in enumerate(cuts_of(PSD_LENS[:-1], total)):
            for c in range(nch):
                v = xs[c][(k + c) % 8:][a:b]  # (sources at every offset from a group boundary)
                g.process_int(c, v, scale)
                twin.process(c, converted(v, sc))
        for c in range(nch):
            assert g.num_stages(c) >= 2
            same(psd_bits(g, c), psd_bits(twin, c), f"n={n} channel {c} {np.dtype(dtype).name} scale={scale}")
        g.close(), twin.close()


def test_psd_kind_changes_inside_a_quantum(pkg, gpu_required):
    """f32, s16 and s8 calls interleaved at quantum 4096 against an all-f32 twin: a change of kind submits what is staged, so
    the chunks differ from the twin's -- Break fields and counts are exactly equal, spectra within the chunk-invariance bound"""
    n = 256
    rng = np.random.default_rng(77)
    g, twin = pkg.PsdCascadeBank(n), pkg.PsdCascadeBank(n)
    g.configure(quantum=4096), twin.configure(quantum=4096)
    s16, s8 = default_scale(pkg, np.int16), default_scale(pkg, np.int8)
    for k, length in enumerate([700, 1500, 33, 5000, 900, 4096, 1, 2500, 12000, 333, 8000, 3000]):
        which = k % 3
        if which == 0:
            f = (rng.standard_normal(length) * 0.2).astype(np.float32)
            g.process(0, f)
        elif which == 1:
            v = int_streams(np.int16, 1, length, 500 + k, tone=False)[0]
            f = converted(v, s16)
            g.process_int(0, v)
        else:
            v = int_streams(np.int8, 1, length, 500 + k, tone=False)[0]
            f = converted(v, s8)
            g.process_int(0, v)
        twin.process(0, f)
    (p, br), (pt, brt) = g.psd(0), twin.psd(0)
    assert br == brt and len(br) >= 2
    assert g.num_stages(0) == twin.num_stages(0)
    for k in range(g.num_stages(0)):
        assert g.stage_info(0, k) == twin.stage_info(0, k), k
    print("max rel diff", float(np.max(np.abs(p - pt) / pt)))
    assert_psd_close(p, pt, "kinds interleaved inside a quantum")
    g.close(), twin.close()


DEV_LENS = [100, 5000, 60000]


def dev_case(pkg, n, v, scale, held=None, after=False):
    """feed device int16 in calls of 100, 5000 and 60 000 units; returns the bank.  held: an f32 device tensor handed over first
    (an in-place span, held); after: the integers are produced on another torch stream and handed over with an event"""
    import torch
    g = pkg.PsdCascadeBank(n)
    keep = []
    if held is not None:
        g.process_device(0, held.data_ptr(), held.numel())
    if after:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dv = torch.zeros(v.size + 3, dtype=torch.int16, device="cuda")
            dv[3:].copy_(torch.from_numpy(v).pin_memory(), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
        base, event = dv.data_ptr() + 6, ev.cuda_event
        keep += [dv, ev, s]
    else:
        dv = torch.from_numpy(np.concatenate([np.zeros(1, v.dtype), v])).cuda()  # (an odd element offset: 2 bytes past 16)
        torch.cuda.synchronize()
        base, event = dv.data_ptr() + 2, None
        keep.append(dv)
    for a, b in cuts_of(DEV_LENS[:-1], v.size):
        g.process_int_device(0, base + 2 * a, b - a, pkg.SampleKind.S16, scale, after=event)
    g.sync()
    g._keep = keep
    return g


@pytest.mark.parametrize("n", [256, 1024])
def test_psd_device(pkg, ora, gpu_required, n):
    """device int16 in calls of 100, 5000 and 60 000 units: psd() and every stage against the f64 oracle of the converted stream
    as tests/test_gpu_parity.py holds the f32 routes; Break fields and stage_info exactly those of the f32 device feed; a second
    run gives the same bytes; so does a buffer handed over with an event; a held in-place f32 span in front keeps its place"""
    import torch
    v = int_streams(np.int16, 1, sum(DEV_LENS), 900 + n)[0]
    sc = default_scale(pkg, np.int16)
    f = converted(v, sc)
    g = dev_case(pkg, n, v, None)
    check_against_oracle(pkg, ora, g, [f], n, what=f"device int16 n={n}")
    fd = torch.from_numpy(f).cuda()
    torch.cuda.synchronize()
    twin = pkg.PsdCascadeBank(n)
    for a, b in cuts_of(DEV_LENS[:-1], v.size):
        twin.process_device(0, fd.data_ptr() + 4 * a, b - a)
    twin.sync()
    (p, br), (pt, brt) = g.psd(0), twin.psd(0)
    assert br == brt and g.num_stages(0) == twin.num_stages(0)
    for k in range(g.num_stages(0)):
        assert g.stage_info(0, k) == twin.stage_info(0, k), k
    again = dev_case(pkg, n, v, None)
    same(psd_bits(again, 0), psd_bits(g, 0), "a second identical run")
    handed = dev_case(pkg, n, v, None, after=True)
    same(psd_bits(handed, 0), psd_bits(g, 0), "handed over with an event")
    # a held in-place f32 span of 2^16 samples first: the order is kept
    lead = (np.random.default_rng(n).standard_normal(1 << 16) * 0.1).astype(np.float32)
    ld = torch.from_numpy(lead).cuda()
    torch.cuda.synchronize()
    behind = dev_case(pkg, n, v, sc, held=ld)
    check_against_oracle(pkg, ora, behind, [lead, f], n, what=f"a held f32 span, then device int16, n={n}")
    for b in (g, twin, again, handed, behind):
        b.close()


LAST_ERROR = {"psd": "psdc_last_error", "pair": "psdc_cross_last_error", "matrix": "psdc_csm_last_error"}
CALL = {"psd": "psdc_sint_process", "pair": "psdc_sint_cross_process", "matrix": "psdc_sint_csm_process"}


@pytest.mark.parametrize("obj", ["psd", "pair", "matrix"])
def test_errors_leave_the_object_unchanged(pkg, gpu_required, obj):
    """an unknown kind, a scale that is not finite, an int16 pointer at an odd address, NULL with len > 0: PSDC_ERR_ARG with a text
    that names the call; len == 0 is OK; the object then gives the bytes of a twin that never saw the refused calls"""
    import torch
    L = pkg.lib()
    n, m = 256, {"psd": 1, "pair": 2, "matrix": 3}[obj]
    total = 30_000
    xs = int_streams(np.int16, m, total, 40)
    sc = default_scale(pkg, np.int16)
    S16 = int(pkg.SampleKind.S16)

    def make():
        return pkg.PsdCascadeBank(n) if obj == "psd" else make_x(pkg, obj, n, m)

    def feed(bank, a, b):
        v = [x[a:b] for x in xs]
        if obj == "psd":
            bank.process_int(0, v[0])
        elif obj == "pair":
            bank.process_int(0, v[0], v[1])
        else:
            bank.process_int(0, v)

    g, twin = make(), make()
    feed(g, 0, 9000), feed(twin, 0, 9000)
    host = np.zeros(64, np.int16)
    dev = torch.zeros(64, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def call(device, ptrs, kind, scale, length, unit=0):
        name = CALL[obj] + ("_device" if device else "")
        args = [g._h, unit]
        if obj == "matrix":
            args.append((C.c_void_p * m)(*ptrs))
        else:
            args += [C.c_void_p(p) for p in ptrs]
        args += [kind, C.c_float(scale), length] + ([None] if device else [])
        return getattr(L, name)(*args), name

    def refused(rc_name, *words):
        rc, name = rc_name
        assert rc == pkg.ERR_ARG, (name, rc)
        msg = getattr(L, LAST_ERROR[obj])(g._h).decode()
        assert msg.startswith(name + ": "), msg
        for w in words:
            assert w in msg, msg

    stats = None if obj == "psd" else g.stats_read()
    for device, base in ((False, host.ctypes.data), (True, dev.data_ptr())):
        good = [base + 8 * c for c in range(m)]
        for kind in (0, 3, -1):
            refused(call(device, good, kind, sc, 8), "unknown sample kind")
        for bad in (float("nan"), float("inf"), float("-inf")):
            refused(call(device, good, S16, bad, 8), "scale", "finite")
        for c in range(m):  # each pointer alone at an odd address, and NULL
            refused(call(device, [p + (1 if k == c else 0) for k, p in enumerate(good)], S16, sc, 8), "not aligned", "2 bytes")
            refused(call(device, [0 if k == c else p for k, p in enumerate(good)], S16, sc, 8), "null sample pointer")
        refused(call(device, good, S16, sc, 8, unit=1), "out of range")
        assert call(device, good, S16, sc, 0)[0] == 0  # len == 0 is OK, with any pointers
        assert call(device, [0] * m, S16, sc, 0)[0] == 0
    if stats is not None:
        assert g.stats_read() == stats
    feed(g, 9000, total), feed(twin, 9000, total)
    if obj == "psd":
        same(psd_bits(g, 0), psd_bits(twin, 0), "psd: a valid sequence around refused calls")
    else:
        same(xbits(g), xbits(twin), f"{obj}: a valid sequence around refused calls")
        assert g.stats_read() == twin.stats_read()
    g.close(), twin.close()


@pytest.mark.parametrize("kind,m", [("pair", 2), ("matrix", 4)])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_launch_counts(pkg, gpu_required, kind, m, device):
    """steady calls of one length (one piece): an integer call reports the f32 call's launches + 1, the converter -- a piece from
    host memory, in place of the copies from device memory -- call after call: 3 + 1"""
    n, length, calls = 256, 4096, 6
    src = Sources(int_streams(np.int16, m, length * calls, 71), default_scale(pkg, np.int16))
    gi, gf = make_x(pkg, kind, n, m), make_x(pkg, kind, n, m)
    per_int, per_f32 = [], []
    for k in range(calls):
        feed_x(pkg, kind, gi, src, np.int16, None, device, True, 0, k * length, (k + 1) * length)
        feed_x(pkg, kind, gf, src, np.int16, None, device, False, 0, k * length, (k + 1) * length)
        per_int.append(gi.stats_read(reset=True)["launches"])
        per_f32.append(gf.stats_read(reset=True)["launches"])
    gi.sync(), gf.sync()
    print(f"{kind} device={device}: launches a call, integer {per_int}, f32 {per_f32}")
    assert [a - b for a, b in zip(per_int, per_f32)] == [1] * calls
    assert per_int[-1] == per_int[-2] == per_int[-3] == 4
    gi.close(), gf.close()


def test_cli_reads_real_integer_files(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --sample-format s16 --raw FILE and --pair FILEX:FILEY on files shorter than the tool's 2^20 units a call
    print what one process_int call on a fresh object gives, at the tool's print precision; --file is still refused"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = [sys.executable, os.path.join(root, "tools", "psd_cli.py")]
    length = (1 << 16) + 77
    xa, xb = int_streams(np.int16, 2, length, 83)
    paths = {}
    for name, v in (("xa", xa), ("xb", xb)):
        paths[name] = str(tmp_path / f"{name}.s16")
        v.astype("<i2").tofile(paths[name])
    scale = 2.0 ** -12
    r = subprocess.run(cli + ["--sample-format", "s16", "--scale", repr(scale), "--raw", paths["xa"], "--pair", paths["xa"] + ":" + paths["xb"],
                              "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    avg = pkg.AvgOpts(limit=999, count=0xFFFFFFFE)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
    bank = pkg.PsdCascadeBank(512, 1)
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(avg)
    bank.process_int(0, xa, scale)
    psd, br = bank.psd(0)
    rms, xy = pkg.trace_plot(psd, pkg.Break.frequencies(br), fs=1.0, integrate=False, integral_start=1e-6, integral_end=0.5)
    line = f"raw: stages {bank.num_stages(0)} top-stage averages {bank.stage_info(0, 0)['count']} bins {psd.size} breaks {len(br)} rms {rms:.9g}"
    assert line in r.stdout, r.stdout
    d = np.loadtxt(tmp_path / "csv" / "raw.csv", delimiter=",")
    xy = np.asarray(xy, dtype=np.float64)
    assert d.shape == xy.shape and np.allclose(d, xy, rtol=2e-8, atol=0)
    cross = pkg.CsdCascadeBank(512, 1)
    cross.set_detrend(pkg.Detrend.MEAN)
    cross.set_avg(avg)
    cross.process_int(0, xa, xb, scale)
    sxx, syy, sxy, brx = cross.csd(0)
    coh, h1 = pkg.coherence(sxx, syy, sxy), pkg.transfer(sxx, sxy)
    assert f"xa.s16:xb.s16: bins {sxx.size} median coherence {np.nanmedian(coh):.6g}" in r.stdout, r.stdout
    d = np.loadtxt(tmp_path / "csv" / "pair_xa_s16__xb_s16.csv", delimiter=",")
    assert d.shape == (sxx.size, 4)
    assert np.allclose(d[:, 0], pkg.Break.frequencies(brx), rtol=1e-6, atol=0)
    assert np.allclose(d[:, 1], np.abs(h1), rtol=2e-8, atol=0) and np.allclose(d[:, 3], coh, rtol=2e-8, atol=0)
    assert np.allclose(d[:, 2], np.angle(h1), rtol=2e-8, atol=1e-12)
    bank.close(), cross.close()
    r = subprocess.run(cli + ["--sample-format", "s16", "--file", paths["xa"], "--raw", paths["xa"]], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--sample-format" in r.stderr and "--file" in r.stderr
