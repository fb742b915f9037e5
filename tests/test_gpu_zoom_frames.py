"""Stream frames into the zoom cascade (psdc_zoomcascade_process_frames[_device], csrc/zoom_frames.hip): the fused decode-and-mix against
the sample route (psdc_zoom_process fed the oracle's Payload::traces) bit for bit, banks against single objects, host memory
against device memory, mixed sample / frame feeds, accuracy against the f64 restatement, frame errors and Loss against the
auto-PSD side, and the launch count.  Semantics: include/psdcascade.h, "Stream frames into zoom channels"."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross_frames import adcdac_words, decoded
from test_gpu_payload_formats import make_frames, random_payloads
from test_gpu_zoom import same_psd
from test_zoom_host import restate_zoom, stitch_zoom

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
PIECE = 1 << 22  # a frames call is cut into pieces of whole frames of at most this many samples a trace (the header comment)
_CACHE = {}


def frames_of(pkg, ora, fmt, batches, nframes, seed, seq0=7):
    """(data, frame_size, oracle traces) of `nframes` random frames; made once and shared, never modified"""
    key = (fmt, batches, nframes, seed, seq0)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        if fmt == 1:
            data, fs = pkg.make_adcdac_frames(adcdac_words(rng, 8 * batches * nframes), batches, seq0=seq0)
        else:
            data, fs = make_frames(fmt, batches, random_payloads(rng, fmt, batches, nframes, wild=False), seq0=seq0)
        assert len(data) == nframes * fs
        tr = decoded(ora, data, fs)
        for t in tr:
            t.setflags(write=False)
        _CACHE[key] = (data, fs, tr)
    return _CACHE[key]


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


def raw_call(pkg, bank, data_or_ptr, fs, nf, m, device=False, after=None):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    bank = getattr(bank, "_b", bank)
    mp = np.asarray(m, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None
    ok = C.c_size_t(77)
    if device:
        rc = L.psdc_zoomcascade_process_frames_device(bank._h, mp, C.c_void_p(data_or_ptr), fs, nf, C.byref(ok), C.c_void_p(after) if after else None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_zoomcascade_process_frames(bank._h, mp, buf.ctypes.data_as(C.c_void_p), fs, nf, C.byref(ok))
    return rc, ok.value


def loss_fields(pkg, obj, zoom):
    l = pkg._CLoss()
    L = pkg.lib()
    obj = getattr(obj, "_b", obj)
    rc = L.psdc_zoomcascade_loss_read(obj._h, C.byref(l), 0) if zoom else L.psdc_loss_read(obj._h, C.byref(l), 0)
    assert rc == 0
    return (l.received, l.dropped, l.next_seq, l.have_seq)


# batches: odd for the one-sample formats, so that the first call (one frame) leaves every later call at a stream position that is
# no multiple of 4 (dword stores) and ends calls in a partial run of the four-batch threads
@pytest.mark.parametrize("fmt,batches,trace,n", [(1, 19, 2, 1024), (2, 25, 0, 256), (3, 17, 3, 64), (4, 61, 1, 512)])
def test_bit_exact_against_the_sample_route(pkg, ora, gpu_required, fmt, batches, trace, n):
    """One channel, calls of one piece each: the same bits as psdc_zoom_process fed the oracle's Payload::traces at the same cuts."""
    spf = batches * (8 if fmt == 1 else 1)
    nf = 120_000 // spf
    data, fs, tr = frames_of(pkg, ora, fmt, batches, nf, 10 * fmt + batches)
    ftw, ph0 = pkg.zoom_ftw(0.2718281828459045)[0], 0x0123456789ABCDEF
    c = nf // 7
    while c % 4 not in (1, 2):  # c and c + 1 no multiples of 4: with an odd batch count neither cut is at a multiple of 4 samples
        c += 1
    cuts = [0, 1, c, c + 1, nf // 2, nf]
    if fmt != 1:
        assert all((k * spf) % 4 for k in cuts[1:4])
    g = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    twin = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert g.process_frames(data[a * fs:b * fs], fs, trace) == b - a
        twin.process(tr[trace][a * spf:b * spf])
    assert g.num_stages() >= 2
    assert_bits(bits(g), bits(twin), f"format {fmt}")
    assert g.stats_read()["samples_in"] == nf * spf
    # a label names the same trace
    h = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_frames(data[a * fs:b * fs], fs, pkg.TRACE_NAMES[pkg.Format(fmt)][trace])
    assert_bits(bits(h), bits(g), "label")


def test_a_call_of_several_pieces(pkg, ora, gpu_required):
    """Slightly more than 2^22 samples a trace in one call: the twin is fed at the piece boundaries (whole frames, <= 2^22 samples)."""
    n, batches = 1024, 255
    spf = 8 * batches
    per_piece = PIECE // spf  # frames of a piece
    nf = per_piece + 30
    assert nf * spf > PIECE
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 99)
    ftw = pkg.zoom_ftw(0.1234567)[0]
    g = pkg.ZoomCascade(n, ftw=ftw, phase0=1 << 62)
    assert g.process_frames(data, fs, "ADC1") == nf
    twin = pkg.ZoomCascade(n, ftw=ftw, phase0=1 << 62)
    twin.process(tr[1][:per_piece * spf])
    twin.process(tr[1][per_piece * spf:])
    assert_bits(bits(g), bits(twin), "two pieces")


def test_one_trace_many_carriers(pkg, ora, gpu_required):
    """17 channels on ADC0 (two launches a call), carriers whose 64-bit phase product wraps, channels sitting calls out: each
    channel against a single object fed its own calls -- the bank bound 2e-6 (header, "Determinism") when the channels share
    calls, bit for bit when each is fed and read in turn."""
    n, nch, batches = 64, 17, 11
    spf = 8 * batches
    nf = 500
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 5)
    x = tr[0]
    car = [pkg.zoom_ftw(0.01 + 0.057 * i)[0] for i in range(nch)]
    car[3] = (1 << 63) - 1            # near 2^63 and odd: ftw * j wraps from the third sample on
    car[7] = (1 << 63) + 12345
    car[16] = (1 << 64) - 1
    ph = [(i * 0x9E3779B97F4A7C15) & ((1 << 64) - 1) for i in range(nch)]
    cuts = [0, 1, 90, 91, 300, nf]
    calls = list(zip(cuts[:-1], cuts[1:]))
    out = {(3, 1), (3, 2), (16, 0), (5, 4), (0, 3)}  # (channel, call) that sit out
    singles = []
    for c in range(nch):
        s = pkg.ZoomCascade(n, ftw=car[c], phase0=ph[c])
        for k, (a, b) in enumerate(calls):
            if (c, k) not in out:
                s.process(x[a * spf:b * spf])
        singles.append(bits(s))
    bank = pkg.ZoomCascadeBank(n, nch)
    for c in range(nch):
        bank.set_carrier(c, ftw=car[c], phase0=ph[c])
    total = 0
    for k, (a, b) in enumerate(calls):
        m = [None if (c, k) in out else "ADC0" for c in range(nch)]
        assert bank.process_frames(data[a * fs:b * fs], fs, m) == b - a
        total += (b - a) * spf * sum(t is not None for t in m)
    assert bank.stats_read()["samples_in"] == total
    for c in range(nch):
        same_psd(bank.psd(c), singles[c][0], 2e-6, f"channel {c}, shared calls")
    turn = pkg.ZoomCascadeBank(n, nch)
    for c in range(nch):
        turn.set_carrier(c, ftw=car[c], phase0=ph[c])
    for c in range(nch):
        m = [None] * nch
        m[c] = 0
        for k, (a, b) in enumerate(calls):
            if (c, k) not in out:
                turn.process_frames(data[a * fs:b * fs], fs, m)
        assert_bits(bits(turn, c), singles[c], f"channel {c}, fed and read in turn")


@pytest.mark.parametrize("fmt,batches,trace", [(1, 13, 3), (4, 59, 2)])
def test_host_equals_device(pkg, ora, gpu_required, fmt, batches, trace):
    """The same frames from host and from device memory: equal bits, at base offsets 0, 4 and 1 (AdcDac: the 8-byte loads, then
    bytes twice; Mpll: 4-byte words twice, then bytes), and behind a producer's event."""
    import torch
    n = 256
    spf = batches * (8 if fmt == 1 else 1)
    nf = 60_000 // spf
    data, fs, _ = frames_of(pkg, ora, fmt, batches, nf, 40 + fmt, seq0=0xFFFFFF00)
    cuts = [0, 3, nf // 3, nf]
    traces = [trace, None, 0]
    car = [(pkg.zoom_ftw(0.31)[0], 5), (0, 0), ((1 << 63) + 1, 1 << 40)]

    def make():
        b = pkg.ZoomCascadeBank(n, 3)
        for c, (f, p) in enumerate(car):
            b.set_carrier(c, ftw=f, phase0=p)
        return b

    def read(b):
        return [bits(b, c) for c in (0, 2)]

    hb = make()
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert hb.process_frames(data[a * fs:b * fs], fs, traces) == b - a
    ref = read(hb)
    ref_loss = loss_fields(pkg, hb, True)
    assert hb.num_stages(1) == 0
    host_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for shift in (0, 4, 1):
        buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        buf[shift:shift + len(data)].copy_(host_bytes)
        torch.cuda.synchronize()
        db = make()
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert db.process_frames_device(buf.data_ptr() + shift + a * fs, fs, b - a, traces) == b - a
        for u, v in zip(read(db), ref):
            assert_bits(u, v, f"device frames at offset {shift}")
        assert loss_fields(pkg, db, True) == ref_loss
    # a producer on another stream fills the device buffer; the gather and the decode wait for its event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pb = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        pb[0:len(data)].copy_(host_bytes.pin_memory(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
    eb = make()
    for a, b in zip(cuts[:-1], cuts[1:]):
        eb.process_frames_device(pb.data_ptr() + a * fs, fs, b - a, traces, after=ev.cuda_event)
    for u, v in zip(read(eb), ref):
        assert_bits(u, v, "producer event")
    s.synchronize()


def test_mixed_feeds(pkg, ora, gpu_required):
    """Samples, then frames, then samples on one channel: the stream index and so the phase continue.  The odd sample count in
    front puts the AdcDac frames at a stream position that is no multiple of 4 (the dword stores)."""
    n, batches = 512, 16
    spf = 8 * batches
    nf = 700
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 77)
    x = tr[0]
    a, b = 1001, 1001 + 500 * spf  # samples [0, a) and [b, end) go in as samples, the 500 frames between as frames
    assert a % 4 and (b - a) % spf == 0
    f0 = 100  # the frames that hold the middle part: any 500 consecutive ones serve, the trace is what counts
    mid = tr[0][f0 * spf:(f0 + 500) * spf]
    whole = np.concatenate([x[:a], mid, x[b:]])
    ftw, ph0 = pkg.zoom_ftw(0.4142135623730951)[0], 0xFEDCBA9876543210
    g = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    g.process(whole[:a])
    assert g.process_frames(data[f0 * fs:(f0 + 500) * fs], fs, "ADC0") == 500
    g.process(whole[b:])
    twin = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for s, e in ((0, a), (a, b), (b, whole.size)):
        twin.process(whole[s:e])
    assert_bits(bits(g), bits(twin), "samples, frames, samples against the same cuts of samples")
    one = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    one.process(whole)
    same_psd(g.psd(), one.psd(), 2e-6, "against the whole trace in one call (the chunking bound)")
    assert g.stats_read()["samples_in"] == whole.size


@pytest.mark.parametrize("fmt,batches,trace,n", [(1, 32, 0, 256), (3, 18, 2, 128)])
def test_accuracy_against_the_f64_restatement(pkg, ora, gpu_required, fmt, batches, trace, n):
    """test_zoom_parity's assertion (detrend none: the pure bound) on the oracle's decoded trace"""
    spf = batches * (8 if fmt == 1 else 1)
    nf = (1 << 16) // spf
    data, fs, tr = frames_of(pkg, ora, fmt, batches, nf, 200 + fmt)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    g = pkg.ZoomCascade(n, ftw=ftw)
    assert g.process_frames(data, fs, trace) == nf
    up, lo, br = g.psd()
    x = np.asarray(tr[trace], np.float32)
    rup, rlo, rbr = stitch_zoom(pkg, n, pkg.Window.HANN, restate_zoom(ora, x, n, ftw, 0, "hann", "none"))
    assert br == rbr
    for name, got, want in (("upper", up, rup), ("lower", lo, rlo)):
        rel = assert_psd_close(got, want, f"zoom frames {name} format {fmt}", pure=True)
        print(f"format {fmt} {name}: worst relative error {rel:.3g}")


def test_errors_and_loss(pkg, ora, gpu_required):
    n = 64
    rng = np.random.default_rng(5)
    L = pkg.lib()
    # AdcDac (3 batches) and Mpll (8 batches) frames share frame_size 200; seq wraps and has a gap of 7 batches at frame 6
    ad, fs = make_frames(1, 3, random_payloads(rng, 1, 3, 10, wild=False), seq0=0xFFFFFFF4)
    ad = bytearray(ad)
    for f in range(6, 10):
        seq = int.from_bytes(ad[f * fs + 4:f * fs + 8], "little")
        ad[f * fs + 4:f * fs + 8] = ((seq + 7) & 0xFFFFFFFF).to_bytes(4, "little")
    ad = bytes(ad)
    mp, fs2 = make_frames(4, 8, random_payloads(rng, 4, 8, 4, wild=False), seq0=100)
    assert fs == fs2 == 200
    tr = decoded(ora, ad, fs)
    spf = 24
    car = [(pkg.zoom_ftw(0.2)[0], 3), ((1 << 63) - 1, 9)]

    def make():
        b = pkg.ZoomCascadeBank(n, 2)
        for c, (f, p) in enumerate(car):
            b.set_carrier(c, ftw=f, phase0=p)
        return b

    def twin_of(pieces, trace, c):
        t = pkg.ZoomCascade(n, ftw=car[c][0], phase0=car[c][1])
        for a, b in pieces:
            t.process(tr[trace][a * spf:b * spf])
        return bits(t)

    # Mpll has no trace 3: PSDC_ERR_ARG at the run's first frame, the AdcDac run before it is ingested; the sequence gap
    bank = make()
    psd = pkg.PsdCascadeBank(256, 4)
    rc, ok = raw_call(pkg, bank, ad + mp, fs, 14, [0, 3])
    assert (rc, ok) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_zoom_last_error(bank._h).decode()
    psd.process_frames(ad, fs)
    assert bank.stats_read()["samples_in"] == 2 * 10 * spf
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    assert loss_fields(pkg, bank, True)[1] > 0  # the gap is counted
    assert_bits(bits(bank, 0), twin_of([(0, 10)], 0, 0), "the run before the refused one")
    # header-only frames: Loss only
    ho, fs0 = make_frames(1, 0, [b""] * 5, seq0=3)
    assert bank.process_frames(ho, fs0, [0, 3]) == 5
    psd.process_frames(ho, fs0)
    assert bank.stats_read()["samples_in"] == 2 * 10 * spf
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    # bad magic, format id and batch count mid-call: n_ok, the frames before are ingested, and the good remainder continues the
    # stream exactly behind them
    for pos, val, code in ((4 * fs + 1, 0, pkg.ERR_FRAME_HEADER), (4 * fs + 2, 9, pkg.ERR_FRAME_FORMAT), (4 * fs + 3, 2, pkg.ERR_FRAME_SIZE)):
        bad = bytearray(ad)
        bad[pos] = val
        b2 = make()
        p2 = pkg.PsdCascadeBank(256, 4)
        assert raw_call(pkg, b2, bytes(bad), fs, 10, [1, 0]) == (code, 4)
        with pytest.raises(pkg.FrameError):
            p2.process_frames(bytes(bad), fs)
        assert b2.stats_read()["samples_in"] == 2 * 4 * spf
        assert loss_fields(pkg, b2, True) == loss_fields(pkg, p2, False)
        with pytest.raises(pkg.FrameError) as e:
            b2.process_frames(bytes(bad[4 * fs:]), fs, [1, 0])
        assert e.value.code == code
        assert b2.process_frames(ad[4 * fs:], fs, [1, 0]) == 6
        assert_bits(bits(b2, 0), twin_of([(0, 4), (4, 10)], 1, 0), f"remainder after error {code}, channel 0")
        assert_bits(bits(b2, 1), twin_of([(0, 4), (4, 10)], 0, 1), f"remainder after error {code}, channel 1")
    # map errors ingest nothing
    before = (bank.stats_read()["samples_in"], loss_fields(pkg, bank, True))
    for mm in (None, [0, 4], [NONE, 7], [NONE, NONE]):
        assert raw_call(pkg, bank, ad, fs, 10, mm) == (pkg.ERR_ARG, 0), mm
    assert (bank.stats_read()["samples_in"], loss_fields(pkg, bank, True)) == before
    # the same on the device path, through the gather
    import torch
    t = torch.from_numpy(np.frombuffer(ad + mp, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    db = make()
    assert raw_call(pkg, db, t.data_ptr(), fs, 14, [0, 3], device=True) == (pkg.ERR_ARG, 10)
    for mm in (None, [0, 4], [NONE, NONE]):
        assert raw_call(pkg, db, t.data_ptr(), fs, 14, mm, device=True) == (pkg.ERR_ARG, 0), mm
    fresh = make()
    raw_call(pkg, fresh, ad + mp, fs, 14, [0, 3])
    assert loss_fields(pkg, db, True) == loss_fields(pkg, fresh, True)
    assert_bits(bits(db, 1), bits(fresh, 1), "device path after an error")
    # a carrier is fixed once the channel has taken a sample, by frames as by samples; a channel the map left out is still free
    only0 = make()
    only0.process_frames(ad, fs, [2, None])
    with pytest.raises(pkg.PsdError) as e:
        only0.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    only0.set_carrier(1, ftw=1)
    # reset zeroes Loss and the carriers
    only0.reset()
    assert loss_fields(pkg, only0, True) == (0, 0, 0, 0)
    assert only0.loss() == {"received": 0, "dropped": 0}
    only0.process_frames(ad, fs, [2, None])
    z0 = pkg.ZoomCascade(n)
    z0.process(tr[2])
    assert_bits(bits(only0, 0), bits(z0), "after a reset the carrier is the default")


def test_launch_count(pkg, ora, gpu_required):
    """A steady-state call of one piece with 16 fed channels: 1 + 3 launches from host memory, and one more -- the header gather --
    from device memory (the header comment, invariant (d))."""
    import torch
    n, nch, batches = 64, 16, 20
    nf = 2400
    data, fs, _ = frames_of(pkg, ora, 1, batches, nf, 31)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    bank = pkg.ZoomCascadeBank(n, nch)
    for c in range(nch):
        bank.set_carrier(c, f0=0.03 * c)
    m = ["ADC0"] * 8 + ["DAC1"] * 8
    per = 200
    for k in range(4):  # the first calls make the stages and grow the buffers
        bank.process_frames_device(t.data_ptr() + k * per * fs, fs, per, m)
    bank.stats_read(reset=True)
    for k in range(4, 8):
        assert bank.process_frames_device(t.data_ptr() + k * per * fs, fs, per, m) == per
    assert bank.stats_read(reset=True)["launches"] == 4 * 5
    for k in range(8, 12):
        assert bank.process_frames(data[k * per * fs:(k + 1) * per * fs], fs, m) == per
    st = bank.stats_read()
    assert st["launches"] == 4 * 4
    assert st["samples_in"] == 4 * per * 8 * batches * nch
    bank.sync()
    assert bank.num_stages(0) >= 3
