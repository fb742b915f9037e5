"""Stream frames into the zoom cross cascade (psdc_zoomcsdcascade_process_frames[_device], csrc/zoom_cross_frames.hip): the fused
decode-and-mix of both sides of a pair against the sample route (psdc_zcsd_process fed the oracle's Payload::traces) bit for bit --
with two carriers, with one carrier on both sides (the shared oscillator), and with what must not share one --, banks against
single objects, host memory against device memory, mixed sample / frame feeds, accuracy against the f64 restatement, frame errors
and Loss against the auto-PSD side, and the launch counts.  Semantics: include/psdcascade.h, "Stream frames into zoom cross pairs".
"Bits" is csd(), every stage's eight raw rows and its stats, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross_frames import decoded
from test_gpu_payload_formats import make_frames, random_payloads
from test_gpu_zoom_cross import assert_cross_rows, make, same_csd
from test_gpu_zoom_frames import PIECE, frames_of
from test_zoom_cross_host import restate_zoom_cross, stitch_zoom_cross

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def bits(bank, pair=0):
    """csd() and every stage's raw rows and stats of one pair"""
    bank = getattr(bank, "_b", bank)
    return bank.csd(pair), [bank.stage_spectra(pair, k) for k in range(bank.num_stages(pair))]


def assert_bits(a, b, what):
    (ca, sa), (cb, sb) = a, b
    same_csd(ca, cb, 0, what)
    assert len(sa) == len(sb), what
    for k, (u, v) in enumerate(zip(sa, sb)):
        assert u[0] == v[0], (what, k)
        assert u[1].shape == (8, v[1].shape[1]) and u[1].tobytes() == v[1].tobytes(), (what, k)


def raw_call(pkg, bank, data_or_ptr, fs, nf, m, device=False, after=None):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    bank = getattr(bank, "_b", bank)
    mp = np.asarray(m, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None
    ok = C.c_size_t(77)
    if device:
        rc = L.psdc_zoomcsdcascade_process_frames_device(bank._h, mp, C.c_void_p(data_or_ptr), fs, nf, C.byref(ok),
                                                         C.c_void_p(after) if after else None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_zoomcsdcascade_process_frames(bank._h, mp, buf.ctypes.data_as(C.c_void_p), fs, nf, C.byref(ok))
    return rc, ok.value


def loss_fields(pkg, obj, zcsd):
    l = pkg._CLoss()
    L = pkg.lib()
    obj = getattr(obj, "_b", obj)
    rc = L.psdc_zoomcsdcascade_loss_read(obj._h, C.byref(l), 0) if zcsd else L.psdc_loss_read(obj._h, C.byref(l), 0)
    assert rc == 0
    return (l.received, l.dropped, l.next_seq, l.have_seq)


def make_bank(pkg, n, car):
    """a bank whose pair p has the carriers car[p] = ((ftw_a, phase0_a), (ftw_b, phase0_b))"""
    b = pkg.ZoomCsdCascadeBank(n, len(car))
    for p, sides in enumerate(car):
        for side, (f, ph) in enumerate(sides):
            b.set_carrier(p, ftw=f, phase0=ph, side=side)
    return b


def single(pkg, n, sides):
    return make(pkg, n, (sides[0][0], sides[1][0]), phase0=(sides[0][1], sides[1][1]))


FTW = 0x4596B2C1A3F07E55  # about 0.2718 cycles a sample
PH = 0x0123456789ABCDEF

# batches: odd for the one-sample formats, so that the first call (one frame) leaves every later call at a stream position that is
# no multiple of 4 (dword stores) and ends calls in a partial run of the four-batch threads
BIT_CASES = [
    # fmt, batches, n, (x, y), ((ftw_a, phase0_a), (ftw_b, phase0_b))
    (1, 19, 1024, (2, 0), ((FTW, PH), (0x9E3779B97F4A7C15, 7))),            # two different carriers
    (2, 25, 256, (0, 3), ((FTW, PH), (FTW, PH))),                            # one carrier on both sides: the shared oscillator
    (3, 17, 64, (3, 1), ((FTW, PH), (FTW, PH + 1))),                         # equal ftw, another phase0: two oscillators
    (4, 61, 512, (1, 1), ((FTW, 0), ((-FTW) & M64, 0))),                     # the AM / PM recipe: one trace, +-ftw
    (3, 17, 64, (0, 2), (((1 << 63) - 1, 5), ((1 << 63) - 1, 5))),           # shared, near 2^63 and odd: ftw j wraps from j = 2 on
    (1, 19, 1024, (1, 3), (((1 << 63) - 1, 5), ((1 << 63) + 12345, 1 << 40))),  # wrapping products, not shared
]


@pytest.mark.parametrize("case", range(len(BIT_CASES)))
def test_bit_exact_against_the_sample_route(pkg, ora, gpu_required, case):
    """One pair, calls of one piece each: the same bits as psdc_zcsd_process fed the oracle's Payload::traces at the same cuts."""
    fmt, batches, n, (x, y), car = BIT_CASES[case]
    spf = batches * (8 if fmt == 1 else 1)
    nf = 120_000 // spf
    data, fs, tr = frames_of(pkg, ora, fmt, batches, nf, 10 * fmt + batches)
    c = nf // 7
    while c % 4 not in (1, 2):  # c and c + 1 no multiples of 4: with an odd batch count neither cut is at a multiple of 4 samples
        c += 1
    cuts = [0, 1, c, c + 1, nf // 2, nf]
    if fmt != 1:
        assert all((k * spf) % 4 for k in cuts[1:4])
    g = single(pkg, n, car)
    twin = single(pkg, n, car)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert g.process_frames(data[a * fs:b * fs], fs, (x, y)) == b - a
        twin.process(tr[x][a * spf:b * spf], tr[y][a * spf:b * spf])
    assert g.num_stages() >= 2
    assert_bits(bits(g), bits(twin), f"case {case}")
    assert g.stats_read()["pairs_in"] == nf * spf
    # labels name the same traces
    names = pkg.TRACE_NAMES[pkg.Format(fmt)]
    h = single(pkg, n, car)
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_frames(data[a * fs:b * fs], fs, (names[x], names[y]))
    assert_bits(bits(h), bits(g), "labels")


def test_a_call_of_several_pieces(pkg, ora, gpu_required):
    """Slightly more than 2^22 samples a trace in one call: the twin is fed at the piece boundary (whole frames, <= 2^22 samples)."""
    n, batches = 1024, 255
    spf = 8 * batches
    per_piece = PIECE // spf  # frames of a piece
    nf = per_piece + 30
    assert nf * spf > PIECE
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 99)
    car = ((0x1F9ADD3739635F3B, 1 << 62), (0x1F9ADD3739635F3B, 1 << 62))
    g = single(pkg, n, car)
    assert g.process_frames(data, fs, ("ADC1", "DAC1")) == nf
    twin = single(pkg, n, car)
    k = per_piece * spf
    twin.process(tr[1][:k], tr[3][:k])
    twin.process(tr[1][k:], tr[3][k:])
    assert_bits(bits(g), bits(twin), "two pieces")


def test_banks(pkg, ora, gpu_required):
    """9 pairs (two decode launches a call) on the four traces of AdcDac frames, one trace on many sides, shared and separate
    carriers, pairs sitting calls out: each pair against a single object fed its own calls -- the bank bound 2e-6 (header, the
    bank rule) when the pairs share calls, bit for bit when each is fed and read in turn."""
    n, npairs, batches = 64, 9, 11
    spf = 8 * batches
    nf = 500
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 5)
    maps = [(p % 4, (3 * p + 1) % 4) for p in range(npairs)]
    maps[4] = (0, 0)
    maps[8] = (0, 2)
    assert sum(0 in m for m in maps) >= 4  # ADC0 feeds many sides
    car = []
    for p in range(npairs):
        fa = (0x0A3D70A3D70A3D71 * (p + 1)) & M64
        pa = (p * 0x9E3779B97F4A7C15) & M64
        car.append(((fa, pa), (fa, pa)) if p % 2 == 0 else ((fa, pa), ((fa * 3 + 1) & M64, pa ^ 0xFFFF)))
    car[4] = (((1 << 63) - 1, 0), ((1 << 63) + 1, 0))  # +-ftw on one trace
    car[6] = (((1 << 64) - 1, 9), ((1 << 64) - 1, 9))
    cuts = [0, 1, 90, 91, 300, nf]
    calls = list(zip(cuts[:-1], cuts[1:]))
    out = {(3, 1), (3, 2), (8, 0), (5, 4), (0, 3)}  # (pair, call) that sit out
    singles = []
    for p in range(npairs):
        s = single(pkg, n, car[p])
        x, y = maps[p]
        for k, (a, b) in enumerate(calls):
            if (p, k) not in out:
                s.process(tr[x][a * spf:b * spf], tr[y][a * spf:b * spf])
        singles.append(bits(s))
    bank = make_bank(pkg, n, car)
    total = 0
    for k, (a, b) in enumerate(calls):
        m = [None if (p, k) in out else maps[p] for p in range(npairs)]
        assert bank.process_frames(data[a * fs:b * fs], fs, m) == b - a
        total += (b - a) * spf * sum(t is not None for t in m)
    assert bank.stats_read()["pairs_in"] == total
    for p in range(npairs):
        same_csd(bank.csd(p), singles[p][0], 2e-6, f"pair {p}, shared calls")
    turn = make_bank(pkg, n, car)
    for p in range(npairs):
        m = [None] * npairs
        m[p] = maps[p]
        for k, (a, b) in enumerate(calls):
            if (p, k) not in out:
                turn.process_frames(data[a * fs:b * fs], fs, m)
        assert_bits(bits(turn, p), singles[p], f"pair {p}, fed and read in turn")


@pytest.mark.parametrize("fmt,batches,pairs", [(1, 13, [(3, 0), None, (1, 1)]), (4, 59, [(2, 0), None, (1, 1)])])
def test_host_equals_device(pkg, ora, gpu_required, fmt, batches, pairs):
    """The same frames from host and from device memory: equal bits and Loss, at base offsets 0, 4 and 1 (AdcDac: the 8-byte
    loads, then bytes twice; Mpll: 4-byte words twice, then bytes), with a seq that wraps, and behind a producer's event."""
    import torch
    n = 256
    spf = batches * (8 if fmt == 1 else 1)
    nf = 60_000 // spf
    data, fs, _ = frames_of(pkg, ora, fmt, batches, nf, 40 + fmt, seq0=0xFFFFFF00)
    cuts = [0, 3, nf // 3, nf]
    car = [((FTW, 5), (FTW, 5)), ((0, 0), (0, 0)), (((1 << 63) + 1, 1 << 40), ((1 << 63) - 1, 0))]

    def read(b):
        return [bits(b, p) for p in (0, 2)]

    hb = make_bank(pkg, n, car)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert hb.process_frames(data[a * fs:b * fs], fs, pairs) == b - a
    ref = read(hb)
    ref_loss = loss_fields(pkg, hb, True)
    assert ref_loss[0] > 0
    assert hb.num_stages(1) == 0
    host_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for shift in (0, 4, 1):
        buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        buf[shift:shift + len(data)].copy_(host_bytes)
        torch.cuda.synchronize()
        db = make_bank(pkg, n, car)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert db.process_frames_device(buf.data_ptr() + shift + a * fs, fs, b - a, pairs) == b - a
        for u, v in zip(read(db), ref):
            assert_bits(u, v, f"device frames at offset {shift}")
        assert loss_fields(pkg, db, True) == ref_loss
        assert db.num_stages(1) == 0
    # a producer on another stream fills the device buffer; the gather and the decode wait for its event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pb = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        pb[0:len(data)].copy_(host_bytes.pin_memory(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
    eb = make_bank(pkg, n, car)
    for a, b in zip(cuts[:-1], cuts[1:]):
        eb.process_frames_device(pb.data_ptr() + a * fs, fs, b - a, pairs, after=ev.cuda_event)
    for u, v in zip(read(eb), ref):
        assert_bits(u, v, "producer event")
    assert loss_fields(pkg, eb, True) == ref_loss
    s.synchronize()


def test_mixed_feeds(pkg, ora, gpu_required):
    """Samples, then frames, then samples on one pair: the stream index and so both phases continue.  The odd sample count in
    front puts the AdcDac frames at a stream position that is no multiple of 4 (the dword stores)."""
    n, batches = 512, 16
    spf = 8 * batches
    nf = 700
    data, fs, tr = frames_of(pkg, ora, 1, batches, nf, 77)
    a, b = 1001, 1001 + 500 * spf  # samples [0, a) and [b, end) go in as samples, the 500 frames between as frames
    assert a % 4 and (b - a) % spf == 0
    f0 = 100  # the frames that hold the middle part: any 500 consecutive ones serve, the traces are what counts
    whole = [np.concatenate([tr[t][:a], tr[t][f0 * spf:(f0 + 500) * spf], tr[t][b:]]) for t in (0, 3)]
    car = ((0x6A09E667F3BCC908, 0xFEDCBA9876543210), (0x3C6EF372FE94F82B, 3))
    g = single(pkg, n, car)
    g.process(whole[0][:a], whole[1][:a])
    assert g.process_frames(data[f0 * fs:(f0 + 500) * fs], fs, ("ADC0", "DAC1")) == 500
    g.process(whole[0][b:], whole[1][b:])
    twin = single(pkg, n, car)
    for s, e in ((0, a), (a, b), (b, whole[0].size)):
        twin.process(whole[0][s:e], whole[1][s:e])
    assert_bits(bits(g), bits(twin), "samples, frames, samples against the same cuts of samples")
    one = single(pkg, n, car)
    one.process(whole[0], whole[1])
    same_csd(g.csd(), one.csd(), 2e-6, "against the whole streams in one call (the chunking bound)")
    assert g.stats_read()["pairs_in"] == whole[0].size


@pytest.mark.parametrize("fmt,batches,pair,n", [(1, 32, (0, 2), 256), (3, 18, (2, 1), 128)])
def test_accuracy_against_the_f64_restatement(pkg, ora, gpu_required, fmt, batches, pair, n):
    """test_zoom_cross_parity's assertions (detrend none: the pure bound on the auto rows, 1e-5 sqrt(S_aa S_bb) on the cross rows)
    on the oracle's decoded traces"""
    spf = batches * (8 if fmt == 1 else 1)
    nf = (1 << 16) // spf
    data, fs, tr = frames_of(pkg, ora, fmt, batches, nf, 200 + fmt)
    ftw = (pkg.zoom_ftw(0.2345678901234567)[0],) * 2
    g = make(pkg, n, ftw)
    assert g.process_frames(data, fs, pair) == nf
    got = g.csd()
    xa, xb = (np.asarray(tr[t], np.float32) for t in pair)
    ref = stitch_zoom_cross(pkg, n, pkg.Window.HANN, restate_zoom_cross(ora, xa, xb, n, ftw))
    assert got[6] == ref[6]
    for name, u, v in zip(("S_aa upper", "S_aa lower", "S_bb upper", "S_bb lower"), got[:4], ref[:4]):
        rel = assert_psd_close(u, v, f"zoom cross frames {name} format {fmt}", pure=True)
        print(f"format {fmt} {name}: worst relative error {rel:.3g}")
    err = max(float(np.max(np.abs(got[4 + i] - ref[4 + i]) / np.sqrt(ref[i].astype(np.float64) * ref[2 + i]))) for i in (0, 1))
    print(f"format {fmt} S_ab: worst error / sqrt(S_aa S_bb) {err:.3g}")
    assert_cross_rows(got, ref, 1e-5, f"format {fmt}")


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
    car = [((FTW, 3), (FTW, 3)), (((1 << 63) - 1, 9), (FTW, 3))]

    def twin_of(pieces, xy, p):
        t = single(pkg, n, car[p])
        for a, b in pieces:
            t.process(tr[xy[0]][a * spf:b * spf], tr[xy[1]][a * spf:b * spf])
        return bits(t)

    # Mpll has no trace 3: PSDC_ERR_ARG at the run's first frame, the AdcDac run before it is ingested; the sequence gap
    bank = make_bank(pkg, n, car)
    psd = pkg.PsdCascadeBank(256, 4)
    rc, ok = raw_call(pkg, bank, ad + mp, fs, 14, [0, 3, 1, 0])
    assert (rc, ok) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_zcsd_last_error(bank._h).decode()
    psd.process_frames(ad, fs)
    assert bank.stats_read()["pairs_in"] == 2 * 10 * spf
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    assert loss_fields(pkg, bank, True)[1] > 0  # the gap is counted
    assert_bits(bits(bank, 0), twin_of([(0, 10)], (0, 3), 0), "the run before the refused one, pair 0")
    assert_bits(bits(bank, 1), twin_of([(0, 10)], (1, 0), 1), "the run before the refused one, pair 1")
    # header-only frames: Loss only
    ho, fs0 = make_frames(1, 0, [b""] * 5, seq0=3)
    assert bank.process_frames(ho, fs0, [(0, 3), (1, 0)]) == 5
    psd.process_frames(ho, fs0)
    assert bank.stats_read()["pairs_in"] == 2 * 10 * spf
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    assert bank.loss() == {"received": loss_fields(pkg, psd, False)[0], "dropped": loss_fields(pkg, psd, False)[1]}
    # bad magic, format id and batch count mid-call: n_ok, the frames before are ingested, and the good remainder continues the
    # streams exactly behind them
    for pos, val, code in ((4 * fs + 1, 0, pkg.ERR_FRAME_HEADER), (4 * fs + 2, 9, pkg.ERR_FRAME_FORMAT), (4 * fs + 3, 2, pkg.ERR_FRAME_SIZE)):
        bad = bytearray(ad)
        bad[pos] = val
        b2 = make_bank(pkg, n, car)
        p2 = pkg.PsdCascadeBank(256, 4)
        assert raw_call(pkg, b2, bytes(bad), fs, 10, [1, 0, 2, 2]) == (code, 4)
        with pytest.raises(pkg.FrameError):
            p2.process_frames(bytes(bad), fs)
        assert b2.stats_read()["pairs_in"] == 2 * 4 * spf
        assert loss_fields(pkg, b2, True) == loss_fields(pkg, p2, False)
        with pytest.raises(pkg.FrameError) as e:
            b2.process_frames(bytes(bad[4 * fs:]), fs, [(1, 0), (2, 2)])
        assert e.value.code == code
        assert b2.process_frames(ad[4 * fs:], fs, [(1, 0), (2, 2)]) == 6
        assert_bits(bits(b2, 0), twin_of([(0, 4), (4, 10)], (1, 0), 0), f"remainder after error {code}, pair 0")
        assert_bits(bits(b2, 1), twin_of([(0, 4), (4, 10)], (2, 2), 1), f"remainder after error {code}, pair 1")
    # map errors ingest nothing
    before = (bank.stats_read()["pairs_in"], loss_fields(pkg, bank, True), bits(bank, 0))
    for mm in (None, [0, NONE, NONE, NONE], [0, 4, NONE, NONE], [NONE, NONE, 1, 7], [NONE] * 4):
        assert raw_call(pkg, bank, ad, fs, 10, mm) == (pkg.ERR_ARG, 0), mm
    assert (bank.stats_read()["pairs_in"], loss_fields(pkg, bank, True)) == before[:2]
    assert_bits(bits(bank, 0), before[2], "after the map errors")
    # the same on the device path, through the gather
    import torch
    t = torch.from_numpy(np.frombuffer(ad + mp, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    db = make_bank(pkg, n, car)
    assert raw_call(pkg, db, t.data_ptr(), fs, 14, [0, 3, 1, 0], device=True) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_zcsd_last_error(db._h).decode()
    for mm in (None, [0, NONE, NONE, NONE], [0, 4, NONE, NONE], [NONE] * 4):
        assert raw_call(pkg, db, t.data_ptr(), fs, 14, mm, device=True) == (pkg.ERR_ARG, 0), mm
    fresh = make_bank(pkg, n, car)
    raw_call(pkg, fresh, ad + mp, fs, 14, [0, 3, 1, 0])
    assert loss_fields(pkg, db, True) == loss_fields(pkg, fresh, True)
    assert_bits(bits(db, 1), bits(fresh, 1), "device path after an error")
    # a carrier is fixed once the pair has taken a sample, by frames as by samples; a pair the map left out is still free
    only0 = make_bank(pkg, n, car)
    only0.process_frames(ad, fs, [(2, 1), None])
    with pytest.raises(pkg.PsdError) as e:
        only0.set_carrier(0, ftw=1)
    assert e.value.code == pkg.ERR_ARG and "before the first" in str(e.value)
    only0.set_carrier(1, ftw=1)
    # reset zeroes Loss and the carriers
    only0.reset()
    assert loss_fields(pkg, only0, True) == (0, 0, 0, 0)
    assert only0.loss() == {"received": 0, "dropped": 0}
    only0.process_frames(ad, fs, [(2, 1), None])
    z0 = pkg.ZoomCsdCascade(n)
    z0.process(tr[2], tr[1])
    assert_bits(bits(only0, 0), bits(z0), "after a reset the carriers are the default")


def launch_setup(pkg, ora, npairs):
    import torch
    n, batches = 64, 20
    data, fs, _ = frames_of(pkg, ora, 1, batches, 2400, 31)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    car = [((pkg.zoom_ftw(0.03 * p)[0], p), (pkg.zoom_ftw(0.03 * p)[0], p if p % 2 else p + 1)) for p in range(npairs)]
    return n, batches, data, fs, t, make_bank(pkg, n, car)


def test_launch_count(pkg, ora, gpu_required):
    """A steady-state call of one piece with 8 fed pairs: 1 + 3 launches from host memory, and one more -- the header gather --
    from device memory (the header comment, invariant (d))."""
    npairs, per = 8, 200
    n, batches, data, fs, t, bank = launch_setup(pkg, ora, npairs)
    m = [("ADC0", "DAC1"), ("ADC1", "ADC1")] * 4
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
    assert st["pairs_in"] == 4 * per * 8 * batches * npairs
    bank.sync()
    assert bank.num_stages(0) >= 3


def test_a_ninth_pair_is_one_more_decode_launch(pkg, ora, gpu_required):
    """A decode launch takes 8 pairs: the same calls with a ninth fed pair cost exactly one launch more each."""
    npairs, per = 9, 200
    n, batches, data, fs, t, bank = launch_setup(pkg, ora, npairs)
    m9 = [("ADC0", "DAC0")] * 9
    m8 = m9[:8] + [None]
    for k in range(4):
        bank.process_frames_device(t.data_ptr() + k * per * fs, fs, per, m9)
    bank.stats_read(reset=True)
    for k in range(4, 6):
        assert bank.process_frames_device(t.data_ptr() + k * per * fs, fs, per, m9) == per
    assert bank.stats_read(reset=True)["launches"] == 2 * 6
    for k in range(6, 8):
        assert bank.process_frames_device(t.data_ptr() + k * per * fs, fs, per, m8) == per
    st = bank.stats_read(reset=True)
    assert st["launches"] == 2 * 5
    assert st["pairs_in"] == 2 * per * 8 * batches * 8
    for k in range(8, 10):
        assert bank.process_frames(data[k * per * fs:(k + 1) * per * fs], fs, m9) == per
    assert bank.stats_read(reset=True)["launches"] == 2 * 5
    for k in range(10, 12):
        assert bank.process_frames(data[k * per * fs:(k + 1) * per * fs], fs, m8) == per
    assert bank.stats_read()["launches"] == 2 * 4
