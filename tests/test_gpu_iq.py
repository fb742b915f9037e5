"""IQ cascade on the GPU (psdc_iq_*, csrc/iq.hip, csrc/iq_frames.hip) against the f64 restatement of tests/test_zoom_host.py fed the
complex f64 mix of tests/test_iq_host.py, against its complex64 sibling, and against the zoom object where Q = 0 makes the two
the same thing.  Semantics: include/psdcascade.h, "IQ cascade"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS
from test_gpu_payload_formats import make_frames, random_payloads
from test_gpu_zoom import same_psd
from test_iq_host import iq_emul, mix_c_f32, mix_c_f64  # noqa: F401
from test_zoom_host import U32_MAX, carrier_ftw, noise, restate_zoom, stitch_zoom, windows_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF

# (n, window, detrend, avg, carrier, length, route): the issue's six cases
PARITY_CASES = [
    (64, "hann", "none", None, ("bin", 5), 1 << 17, "planar"),
    (256, "rect", "mean", None, 0.2345678901234567, 1 << 18, "planar"),
    (512, "custom", "span", (U32_MAX, 1000), 0.7131313131313131, 1 << 18, "planar"),
    (1024, "hann", "midpoint", (100, U32_MAX), 0.1 * 2 ** 0.5, 1 << 19, "planar"),
    (4096, "hann", "none", None, 0.0, 1 << 20, "planar"),
    (256, "hann", "none", None, 0.0, 1 << 18, "interleaved"),
]


def iq_noise(length, seed):
    """complex Gaussian input: independent I and Q"""
    return noise(length, seed), noise(length, seed + 7919)


def bits(bank, ch=0):
    """psd() and every stage's raw rows and stats of one channel"""
    bank = getattr(bank, "_b", bank)
    return bank.psd(ch), [bank.stage_spectra(ch, k) for k in range(bank.num_stages(ch))]


def assert_bits(a, b, what):
    (pa, sa), (pb, sb) = a, b
    same_psd(pa, pb, 0, what)
    assert len(sa) == len(sb), what
    for k, (u, v) in enumerate(zip(sa, sb)):
        assert u[0] == v[0], (what, k)
        for p, q in zip(u[1:], v[1:]):
            assert p.tobytes() == q.tobytes(), (what, k)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_iq_parity(pkg, ora, gpu_required, iq_emul, case):  # noqa: F811
    n, wkind, detrend, avg, carrier, length, route = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    i, q = iq_noise(length, 2000 + n)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.IqCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    if route == "planar":
        g.process((i, q))
    else:
        g.process((i + 1j * q).astype(np.complex64))
    up, lo, br = g.psd()
    rup, rlo, rbr = stitch_zoom(pkg, n, pwin, restate_zoom(ora, i, n, ftw, 0, owin, detrend, avg, "f64", iq=mix_c_f64(i, q, ftw)))
    assert br == rbr
    if detrend == "none":
        for name, got, want in (("upper", up, rup), ("lower", lo, rlo)):
            rel = assert_psd_close(got, want, f"iq {name} case {case}", pure=True)
            print(f"case {case} {name}: worst relative error {rel:.3g}")
    else:  # a detrend nulls bin 0 of both rows: the widened bound, held to the complex64 sibling's own f32 arithmetic there
        sup, slo, _ = stitch_zoom(pkg, n, pwin, restate_zoom(ora, i, n, ftw, 0, owin, detrend, avg, "f32",
                                                             iq=mix_c_f32(iq_emul, i, q, ftw)))
        assert_psd_close(up, rup, f"iq upper case {case} {detrend}", ref_f32=sup)
        assert_psd_close(lo, rlo, f"iq lower case {case} {detrend}", ref_f32=slo)


@pytest.mark.parametrize("n", [1024, 64])
def test_iq_with_q_zero_is_the_zoom_object(pkg, gpu_required, n):
    """IqCascade fed (x, 0) gives the rows of ZoomCascade fed x, with equal bytes: the mix formula with Q = 0 is zoom_mix, and
    everything behind the mixer is the same code.  One call each, so the rounds coincide."""
    x = noise(1 << 19, 51 + n)
    z = pkg.ZoomCascade(n, f0=0.2)
    z.process(x)
    g = pkg.IqCascade(n, f0=0.2)
    g.process((x, np.zeros_like(x)))
    assert_bits(bits(g), bits(z), f"(x, 0) against the zoom object, n = {n}")


def test_iq_routes_agree_bit_for_bit(pkg, gpu_required):
    """The same stream by the four sample routes, every route with the same call cut: equal bits"""
    import torch
    n = 256
    length = (1 << 17) + 13
    cuts = [0, 1000, 34_331, 34_334, length]
    i, q = iq_noise(length, 61)
    z = (i + 1j * q).astype(np.complex64)
    assert np.array_equal(z.real, i) and np.array_equal(z.imag, q)
    di, dq, dz = torch.from_numpy(i).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(z).cuda()
    assert dz.dtype == torch.complex64
    torch.cuda.synchronize()
    got = {}
    for route in ("planar host", "planar device", "interleaved host", "interleaved device"):
        g = pkg.IqCascade(n, f0=0.3)
        for s, e in zip(cuts[:-1], cuts[1:]):
            if route == "planar host":
                g.process((i[s:e], q[s:e]))
            elif route == "planar device":
                g.process_device_planar(di.data_ptr() + 4 * s, dq.data_ptr() + 4 * s, e - s)
            elif route == "interleaved host":
                g.process(z[s:e])
            else:
                g.process_device(dz.data_ptr() + 8 * s, e - s)
        got[route] = bits(g)
        assert g.stats_read()["samples_in"] == length
    for route in list(got)[1:]:
        assert_bits(got[route], got["planar host"], route)


def test_iq_alignment_and_cuts(pkg, gpu_required):
    """Calls of 1, 2, 3, 5, ... samples take the stream position off the 16-byte grid and keep it there; device sources offset by 1,
    2 and 3 floats (planar) and by one complex sample (interleaved) take the sources off it.  Against the one-call result: the
    zoom tests' chunking bound (2e-6), counts and pendings equal; a second identical run: equal bytes."""
    import torch
    n = 64
    length = (1 << 15) + 37
    lens = [1, 2, 3, 5, 64, 1001, 4099, 7, 12_345, 6]
    lens.append(length - sum(lens))
    assert lens[-1] > 0 and sum(lens) == length
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    assert any(c % 4 for c in cuts[1:-1])
    i, q = iq_noise(length, 71)
    z = (i + 1j * q).astype(np.complex64)
    one = pkg.IqCascade(n, f0=0.123)
    one.process((i, q))
    ref = bits(one)

    def check(g, what):
        b = bits(g)
        same_psd(b[0], ref[0], 2e-6, what)
        assert len(b[1]) == len(ref[1]), what
        for k, (u, v) in enumerate(zip(b[1], ref[1])):
            assert (u[0]["count"], u[0]["pending"]) == (v[0]["count"], v[0]["pending"]), (what, k)
        return b

    def host_run():
        g = pkg.IqCascade(n, f0=0.123)
        for s, e in zip(cuts[:-1], cuts[1:]):
            g.process((i[s:e], q[s:e]))
        return g

    first = check(host_run(), "host cuts")
    assert_bits(bits(host_run()), first, "host cuts, the same calls twice")
    for off in (1, 2, 3):
        oq = (off + 1) % 4
        ti, tq = torch.zeros(length + 4), torch.zeros(length + 4)
        ti[off:off + length] = torch.from_numpy(i)
        tq[oq:oq + length] = torch.from_numpy(q)
        ti, tq = ti.cuda(), tq.cuda()
        torch.cuda.synchronize()
        runs = []
        for _ in range(2):
            g = pkg.IqCascade(n, f0=0.123)
            for s, e in zip(cuts[:-1], cuts[1:]):
                g.process_device_planar(ti.data_ptr() + 4 * (off + int(s)), tq.data_ptr() + 4 * (oq + int(s)), int(e - s))
            runs.append(check(g, f"planar device sources offset by {off} and {oq} floats"))
        assert_bits(runs[0], runs[1], f"offset {off}, the same calls twice")
        assert_bits(runs[0], first, f"offset {off} against the host route")
        whole = pkg.IqCascade(n, f0=0.123)
        whole.process_device_planar(ti.data_ptr() + 4 * off, tq.data_ptr() + 4 * oq, length)
        assert_bits(bits(whole), ref, f"one call from sources offset by {off} and {oq} floats")
    tz = torch.zeros(length + 1, dtype=torch.complex64)
    tz[1:] = torch.from_numpy(z)
    tz = tz.cuda()
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        g = pkg.IqCascade(n, f0=0.123)
        for s, e in zip(cuts[:-1], cuts[1:]):
            g.process_device(tz.data_ptr() + 8 * (1 + int(s)), int(e - s))
        runs.append(check(g, "interleaved device source offset by one complex sample"))
    assert_bits(runs[0], runs[1], "interleaved offset, the same calls twice")
    assert_bits(runs[0], first, "interleaved offset against the host route")
    # an interleaved pointer off the 8-byte grid is refused
    with pytest.raises(pkg.PsdError) as e:
        one.process_device(tz.data_ptr() + 4, 10)
    assert e.value.code == pkg.ERR_ARG and "8 bytes" in str(e.value)


def eem_frames(i, q, batches, seq0=0):
    """ThermostatEem frames whose traces 0 and 1 (words 0 and 8 of a batch, f32 as they are) carry i and q"""
    nf = i.size // batches
    assert nf * batches == i.size
    w = np.zeros((nf, batches, 20), np.float32)
    w[:, :, 0] = i.reshape(nf, batches)
    w[:, :, 8] = q.reshape(nf, batches)
    return make_frames(3, batches, [w[f].astype("<f4").tobytes() for f in range(nf)], seq0=seq0)


def test_iq_phase_continuity_and_carrier_rule(pkg, ora, gpu_required, iq_emul):  # noqa: F811
    """A complex tone at f0 + delta, delta the centre of bin 100 of stage 1, cut into uneven calls that mix the sample routes and
    the frames route: the peak is at offset delta in `upper` (the phase continues across calls and routes), and its image in `lower`
    is, relative to the peak, no larger than 4 x the worse of the f64 restatement's and the complex64 sibling's."""
    n, k, b = 256, 1, 100
    ftw, f0 = pkg.zoom_ftw(0.2)
    delta = b / (n * 8.0 ** k)
    length = 1 << 17
    ph = 2 * np.pi * ((f0 + delta) * np.arange(length, dtype=np.float64) % 1.0)
    i, q = np.cos(ph).astype(np.float32), np.sin(ph).astype(np.float32)
    batches, nf = 17, 2000
    a0, a1 = 1001, 1001 + batches * nf
    data, fs = eem_frames(i[a0:a1], q[a0:a1], batches)
    g = pkg.IqCascade(n, ftw=ftw)
    g.process((i[:a0], q[:a0]))
    assert g.process_frames(data, fs, ("T00", "T20")) == nf
    mid = a1 + 33_333
    g.process((i[a1:mid] + 1j * q[a1:mid]).astype(np.complex64))
    g.process((i[mid:], q[mid:]))
    assert g.stats_read()["samples_in"] == length
    up, lo, br = g.psd()
    f = pkg.Break.frequencies(br)
    assert abs(f[int(np.argmax(up))] - delta) <= 0.5 / (n * 8.0 ** k)
    _, su, sl = g.stage_spectra(k)
    assert int(np.argmax(su)) == b
    gpu = float(sl[b]) / float(su[b])
    st64 = restate_zoom(ora, i, n, ftw, iq=mix_c_f64(i, q, ftw))
    st32 = restate_zoom(ora, i, n, ftw, prec="f32", iq=mix_c_f32(iq_emul, i, q, ftw))
    r64 = float(st64[k]["lower"][b] / st64[k]["upper"][b])
    r32 = float(st32[k]["lower"][b] / st32[k]["upper"][b])
    print(f"image / peak at stage {k} bin {b}: GPU {gpu:.3g}, f64 restatement {r64:.3g}, complex64 sibling {r32:.3g}")
    assert gpu <= 4.0 * max(r64, r32), (gpu, r64, r32)
    # a carrier is set before the first sample only; a bank's reset restores the default carrier
    with pytest.raises(pkg.PsdError) as err:
        g.set_carrier(ftw=1)
    assert err.value.code == pkg.ERR_ARG and "before the first" in str(err.value)
    bank = pkg.IqCascadeBank(n, 1)
    bank.set_carrier(0, ftw=ftw, phase0=12345)
    bank.process(0, (i[:10], q[:10]))
    bank.reset()
    assert bank.carriers[0] == (0, 0)
    bank.process(0, (i[:50_000], q[:50_000]))
    z0 = pkg.IqCascade(n)
    z0.process((i[:50_000], q[:50_000]))
    assert_bits(bits(bank), bits(z0), "a bank's reset puts the carrier back to 0")


def test_iq_reference_statistical_bound(pkg, gpu_required):
    """The reference's own test shape (src/psd.rs:623-643) on both rows: complex uniform noise with E|z|^2 = 1 reads 2 -- 0.5 row within
    10 / sqrt(count) of 1 in every included bin."""
    n = 512
    s = np.float32(0.5 ** 0.5)
    i = pkg.noise_host(1 << 21, seed=0xC0FFEE) * s
    q = pkg.noise_host(1 << 21, seed=0xBEEF) * s
    z = pkg.IqCascade(n, f0=0.2)
    z.process((i, q))
    up, lo, br = z.psd()
    assert len(br) >= 4
    checked = 0
    for b in br:
        if not b.include or b.count == 0:
            continue
        for name, row in (("upper", up), ("lower", lo)):
            p = row[b.start:b.start + b.bins.stop - b.bins.start].astype(np.float64)
            dev = np.max(np.abs(0.5 * p - 1.0))
            assert dev < 10.0 / np.sqrt(b.count), (name, b, dev)
            checked += p.size
    assert checked > 0


_FRAMES = {}


def frames_of(pkg, fmt, batches, nframes, seed, seq0=7):
    """(data, frame_size, traces as source.decode_frame gives them) of `nframes` random frames; made once, never modified"""
    from stabilizer_stream_amd import source
    key = (fmt, batches, nframes, seed, seq0)
    if key not in _FRAMES:
        rng = np.random.default_rng(seed)
        if fmt == 1:
            words = np.clip(rng.standard_normal((4, 8 * batches * nframes)) * 3000, -32768, 32767).astype(np.int16)
            data, fs = pkg.make_adcdac_frames(words, batches, seq0=seq0)
        else:
            data, fs = make_frames(fmt, batches, random_payloads(rng, fmt, batches, nframes, wild=False), seq0=seq0)
        data = bytes(data)
        assert len(data) == nframes * fs
        tr = None
        for f in range(nframes):
            t = source.decode_frame(data[f * fs:(f + 1) * fs])[3]
            tr = [[] for _ in t] if tr is None else tr
            for c, (_, v) in enumerate(t):
                tr[c].append(v)
        tr = [np.concatenate(t).astype(np.float32) for t in tr]
        for t in tr:
            t.setflags(write=False)
        _FRAMES[key] = (data, fs, tr)
    return _FRAMES[key]


def raw_frames_call(pkg, bank, data_or_ptr, fs, nf, m, device=False):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    bank = getattr(bank, "_b", bank)
    mp = np.asarray(m, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None
    ok = C.c_size_t(77)
    if device:
        rc = L.psdc_iq_process_frames_device(bank._h, mp, C.c_void_p(data_or_ptr), fs, nf, C.byref(ok), None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_iq_process_frames(bank._h, mp, buf.ctypes.data_as(C.c_void_p), fs, nf, C.byref(ok))
    return rc, ok.value


# Fls BI / BQ by label, AdcDac traces 0 / 1, and the two other formats once (batches odd for the one-sample formats: the second
# call starts off the 16-byte grid and calls end in a partial run of the four-batch threads)
@pytest.mark.parametrize("fmt,batches,pair,n", [(2, 25, ("BI", "BQ"), 64), (1, 19, (0, 1), 64), (3, 17, (3, 1), 64), (4, 61, (2, 2), 64)])
def test_iq_frames_against_the_sample_route(pkg, gpu_required, fmt, batches, pair, n):
    """Calls of one piece each: the same bits as the planar sample route fed the decoded traces at the same cuts, from host and from
    device memory (base offsets 0 and 1: the aligned loads, then bytes)."""
    import torch
    spf = batches * (8 if fmt == 1 else 1)
    nf = 40_000 // spf
    assert nf * spf <= 1 << 16
    data, fs, tr = frames_of(pkg, fmt, batches, nf, 10 * fmt + batches)
    ti, tq = (tr[pkg.trace_index(t)] for t in pair)
    ftw, ph0 = pkg.zoom_ftw(0.2718281828459045)[0], 0x0123456789ABCDEF
    cuts = [0, 1, nf // 3, nf]
    g = pkg.IqCascade(n, ftw=ftw, phase0=ph0)
    twin = pkg.IqCascade(n, ftw=ftw, phase0=ph0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert g.process_frames(data[a * fs:b * fs], fs, pair) == b - a
        twin.process((ti[a * spf:b * spf], tq[a * spf:b * spf]))
    assert g.num_stages() >= 2
    assert_bits(bits(g), bits(twin), f"format {fmt}, host frames")
    assert g.stats_read()["samples_in"] == nf * spf
    assert g.loss() == {"received": nf * batches, "dropped": 0}
    host_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for shift in (0, 1):
        buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        buf[shift:shift + len(data)].copy_(host_bytes)
        torch.cuda.synchronize()
        d = pkg.IqCascade(n, ftw=ftw, phase0=ph0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert d.process_frames_device(buf.data_ptr() + shift + a * fs, fs, b - a, pair) == b - a
        assert_bits(bits(d), bits(g), f"format {fmt}, device frames at offset {shift}")
        assert d.loss() == g.loss()


def test_iq_frames_shared_pair_gap_and_errors(pkg, gpu_required):
    """Two channels on one trace pair with different carriers, a sequence gap in Loss, the three de::Error codes and the map errors."""
    n = 64
    rng = np.random.default_rng(5)
    L = pkg.lib()
    # AdcDac (3 batches) and Mpll (8 batches) frames share frame_size 200; a gap of 7 batches at frame 6
    ad, fs = make_frames(1, 3, random_payloads(rng, 1, 3, 10, wild=False), seq0=0xFFFFFFF4)
    ad = bytearray(ad)
    for f in range(6, 10):
        seq = int.from_bytes(ad[f * fs + 4:f * fs + 8], "little")
        ad[f * fs + 4:f * fs + 8] = ((seq + 7) & 0xFFFFFFFF).to_bytes(4, "little")
    ad = bytes(ad)
    mp, fs2 = make_frames(4, 8, random_payloads(rng, 4, 8, 4, wild=False), seq0=100)
    assert fs == fs2 == 200
    from stabilizer_stream_amd import source
    dec = [source.decode_frame(ad[f * fs:(f + 1) * fs])[3] for f in range(10)]
    tr = [np.concatenate([d[c][1] for d in dec]).astype(np.float32) for c in range(4)]
    spf = 24
    car = [(pkg.zoom_ftw(0.2)[0], 3), ((1 << 63) - 1, 9)]

    def make():
        b = pkg.IqCascadeBank(n, 2)
        for c, (f, p) in enumerate(car):
            b.set_carrier(c, ftw=f, phase0=p)
        return b

    def twin_of(pieces, ti, tq, c):
        t = pkg.IqCascade(n, ftw=car[c][0], phase0=car[c][1])
        for a, b in pieces:
            t.process((tr[ti][a * spf:b * spf], tr[tq][a * spf:b * spf]))
        return bits(t)

    # both channels take (ADC0, DAC1), each with its own carrier; the gap is counted
    bank = make()
    assert bank.process_frames(ad, fs, [("ADC0", "DAC1"), (0, 3)]) == 10
    assert bank.stats_read()["samples_in"] == 2 * 10 * spf
    assert bank.loss() == {"received": 30, "dropped": 7}
    for c in range(2):
        assert_bits(bits(bank, c), twin_of([(0, 10)], 0, 3, c), f"shared pair, channel {c}")
    assert bits(bank, 0)[0][0].tobytes() != bits(bank, 1)[0][0].tobytes()
    # Mpll has no trace 3: PSDC_ERR_ARG at the run's first frame, the AdcDac run before it is ingested and counted
    b1 = make()
    assert raw_frames_call(pkg, b1, ad + mp, fs, 14, [0, 1, 2, 3]) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_iq_last_error(b1._h).decode()
    assert b1.stats_read()["samples_in"] == 2 * 10 * spf
    assert_bits(bits(b1, 1), twin_of([(0, 10)], 2, 3, 1), "the run before the refused one")
    # bad magic, format id and batch count mid-call: the code, n_ok, and the frames before are ingested
    for pos, val, code in ((4 * fs + 1, 0, pkg.ERR_FRAME_HEADER), (4 * fs + 2, 9, pkg.ERR_FRAME_FORMAT), (4 * fs + 3, 2, pkg.ERR_FRAME_SIZE)):
        bad = bytearray(ad)
        bad[pos] = val
        b2 = make()
        assert raw_frames_call(pkg, b2, bytes(bad), fs, 10, [1, 0, NONE, NONE]) == (code, 4)
        assert b2.stats_read()["samples_in"] == 4 * spf
        with pytest.raises(pkg.FrameError) as e:
            b2.process_frames(bytes(bad[4 * fs:]), fs, [(1, 0)])
        assert e.value.code == code
        assert b2.process_frames(ad[4 * fs:], fs, [(1, 0)]) == 6
        assert_bits(bits(b2, 0), twin_of([(0, 4), (4, 10)], 1, 0, 0), f"remainder after error {code}")
        assert b2.num_stages(1) == 0
    # map errors ingest nothing: NULL, a trace >= 4, one PSDC_TRACE_NONE in a channel, no channel fed
    before = (bank.stats_read()["samples_in"], bank.loss())
    for mm in (None, [0, 4, NONE, NONE], [0, NONE, 1, 2], [NONE, 1, NONE, NONE], [NONE, NONE, NONE, NONE]):
        assert raw_frames_call(pkg, bank, ad, fs, 10, mm) == (pkg.ERR_ARG, 0), mm
    assert (bank.stats_read()["samples_in"], bank.loss()) == before
    import torch
    t = torch.from_numpy(np.frombuffer(ad + mp, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    db = make()
    assert raw_frames_call(pkg, db, t.data_ptr(), fs, 14, [0, 1, 2, 3], device=True) == (pkg.ERR_ARG, 10)
    for mm in (None, [0, NONE, 1, 2], [NONE, NONE, NONE, NONE]):
        assert raw_frames_call(pkg, db, t.data_ptr(), fs, 14, mm, device=True) == (pkg.ERR_ARG, 0), mm
    assert db.loss() == b1.loss()
    assert_bits(bits(db, 1), bits(b1, 1), "device path after an error")
    # a carrier is fixed by frames as by samples; reset zeroes Loss
    with pytest.raises(pkg.PsdError) as e:
        db.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    db.reset()
    assert db.loss() == {"received": 0, "dropped": 0}


def test_iq_bank_launches_events_and_errors(pkg, gpu_required):
    import torch
    n = 256
    # a 3-channel bank's channels each equal a single object, when fed and read in turn
    lens = [100_000, 65_537, 1 << 16]
    step = [10_000, 33_333, 65_536]
    car = [pkg.zoom_ftw(f)[0] for f in (0.2, 0.0, 0.75)]
    ph = [0, 1 << 63, 12345]
    xs = [iq_noise(m, 400 + c) for c, m in enumerate(lens)]
    bank = pkg.IqCascadeBank(n, 3)
    for c in range(3):
        bank.set_carrier(c, ftw=car[c], phase0=ph[c])
    for c in range(3):
        s = pkg.IqCascade(n, ftw=car[c], phase0=ph[c])
        for p in range(0, lens[c], step[c]):
            cut = (xs[c][0][p:p + step[c]], xs[c][1][p:p + step[c]])
            s.process(cut)
            bank.process(c, cut)
        assert_bits(bits(bank, c), bits(s), f"channel {c}, fed in turn")
    # a steady one-piece sample call is 1 + 3 launches; a device frames call 5
    m = 1 << 18
    dz = torch.randn(m, dtype=torch.complex64, device="cuda")
    di = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.IqCascade(n, f0=0.2)
    for _ in range(6):  # the first calls make the stages and grow the buffers
        g.process_device(dz.data_ptr(), m)
    g.stats_read(reset=True)
    for _ in range(3):
        g.process_device(dz.data_ptr(), m)
        g.process_device_planar(di.data_ptr(), dz.data_ptr(), m)
    assert g.stats_read(reset=True)["launches"] == 4 * 6
    hz = np.zeros(m, np.complex64)
    hz.real = 1.0
    g.process(hz)
    g.stats_read(reset=True)
    g.process(hz)
    g.process((hz.real.copy(), hz.imag.copy()))
    assert g.stats_read(reset=True)["launches"] == 4 * 2
    data, fs, _ = frames_of(pkg, 2, 25, 1600, 77)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    f = pkg.IqCascade(64, f0=0.1)
    per = 200
    for k in range(4):
        f.process_frames_device(t.data_ptr() + k * per * fs, fs, per, ("BI", "BQ"))
    f.stats_read(reset=True)
    for k in range(4, 6):
        assert f.process_frames_device(t.data_ptr() + k * per * fs, fs, per, ("BI", "BQ")) == per
    assert f.stats_read(reset=True)["launches"] == 5 * 2
    for k in range(6, 8):
        assert f.process_frames(data[k * per * fs:(k + 1) * per * fs], fs, ("BI", "BQ")) == per
    assert f.stats_read()["launches"] == 4 * 2
    # producer_event: samples made on a torch stream and handed over with an event
    i, q = iq_noise(1 << 18, 300)
    z = (i + 1j * q).astype(np.complex64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tz = torch.from_numpy(z).pin_memory().cuda(non_blocking=True) * 1.0
        ev = torch.cuda.Event()
        ev.record(s)
    a = pkg.IqCascade(n, f0=0.3)
    a.process_device(tz.data_ptr(), z.size, after=ev.cuda_event)
    got = bits(a)
    h = pkg.IqCascade(n, f0=0.3)
    h.process(z)
    assert_bits(got, bits(h), "after=")
    s.synchronize()
    # errors: a bad channel, Detrend::Linear, NULL pointers, unequal lengths
    with pytest.raises(pkg.PsdError) as e:
        bank.process(3, (i[:10], q[:10]))
    assert e.value.code == pkg.ERR_ARG and "out of range" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        bank.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED
    L = pkg.lib()
    assert L.psdc_iq_process(bank._h, 0, pkg._fptr(i), None, 10) == pkg.ERR_ARG
    assert "null sample pointer" in L.psdc_iq_last_error(bank._h).decode()
    assert L.psdc_iq_process(bank._h, 0, None, pkg._fptr(q), 10) == pkg.ERR_ARG
    assert L.psdc_iq_process_interleaved(bank._h, 0, None, 10) == pkg.ERR_ARG
    assert L.psdc_iq_process_device(bank._h, 0, None, None, 10, None) == pkg.ERR_ARG
    assert L.psdc_iq_process_interleaved_device(bank._h, 0, None, 10, None) == pkg.ERR_ARG
    with pytest.raises(pkg.PsdError) as e:
        bank.process(0, (i[:10], q[:11]))
    assert e.value.code == pkg.ERR_ARG and "differ in length" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        bank.process(0, i[:10])
    assert e.value.code == pkg.ERR_ARG


def _cli(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _cli_bank(pkg, i, q, f0):
    """what tools/psd_cli.py --iq builds: IqCascade<512> with the reference's default AcqOpts (detrend mean, avg_max 1000)"""
    bank = pkg.IqCascadeBank(512, 1)
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.set_carrier(0, f0=f0)
    bank.process(0, (i, q))
    return bank


def _cli_close(d, up, lo):
    return (np.all(np.abs(d[:, 1] - up) <= 2e-6 * up + 1e-6 * np.mean(up)) and
            np.all(np.abs(d[:, 2] - lo) <= 2e-6 * lo + 1e-6 * np.mean(lo)))


def test_iq_cli(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --iq on a planar raw pair and on an Fls file (BI:BQ by label, 2:3 by index) against the object's read-out (the
    tool feeds about 2^20 samples a call: the chunking bound, 2e-6)."""
    fs = 1000.0
    length = (1 << 17) + 777
    i, q = iq_noise(length, 41)
    ph = 2 * np.pi * 0.2001 * np.arange(length)
    i, q = (i + np.cos(ph)).astype(np.float32), (q + np.sin(ph)).astype(np.float32)
    pi, pq = tmp_path / "i.f32", tmp_path / "q.f32"
    i.astype("<f4").tofile(pi)
    q.astype("<f4").tofile(pq)
    out = _cli(["--iq", f"{pi}:{pq}:0.2", "--fs", str(fs), "--csv", str(tmp_path / "csv")])
    assert "iq i.f32:q.f32 @ 0.2" in out
    d = np.loadtxt(tmp_path / "csv" / "iq_i_f32__q_f32_0_2.csv", delimiter=",")
    up, lo, br = _cli_bank(pkg, i, q, 0.2).psd(0)
    assert d.shape == (up.size, 3)
    assert np.allclose(d[:, 0], pkg.Break.frequencies(br) * fs, rtol=1e-6, atol=0)
    assert _cli_close(d, up, lo)
    assert abs(d[int(np.argmax(d[:, 1])), 0] - 0.0001 * fs) <= 0.5 * fs / (512 * 8)  # the tone, 1e-4 fs above the carrier
    # an Fls file, by label and by index
    data, fsz, tr = frames_of(pkg, 2, 25, 2000, 91)
    p = tmp_path / "fls.bin"
    p.write_bytes(data)
    out = _cli(["--file", str(p), "--frame-size", str(fsz), "--iq", "BI:BQ:0.125", "--iq", "2:3", "--csv", str(tmp_path / "csv")])
    assert "iq BI:BQ @ 0.125" in out and "iq BI:BQ @ 0" in out
    for name, f0 in (("iq_BI__BQ_0_125.csv", 0.125), ("iq_BI__BQ_0.csv", 0.0)):
        d = np.loadtxt(tmp_path / "csv" / name, delimiter=",")
        up, lo, br = _cli_bank(pkg, tr[2], tr[3], f0).psd(0)
        assert d.shape == (up.size, 3) and np.allclose(d[:, 0], pkg.Break.frequencies(br), rtol=1e-6, atol=0)
        assert _cli_close(d, up, lo)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--file", str(p), "--frame-size", str(fsz), "--iq",
                        "BI:nonesuch"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "unknown trace" in r.stderr
