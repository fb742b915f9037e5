"""Stream frames into the cross-spectral cascade (psdc_csd_process_frames[_device], csrc/cross_frames.hip): the decode against
the oracle's Payload::traces bit for bit, pairs against single-pair objects fed f32, host memory against device memory, frame
errors and Loss against the auto-PSD side.  Semantics: include/psdcascade.h, "stream frames into a cross object"."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_psd_close
from test_cross_host import restate, stitch_rows
from test_gpu_cross import _passband_bins, assert_same_csd, assert_sxy_close
from test_gpu_payload_formats import make_frames, random_payloads

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def decoded(ora, data, fs):
    """the oracle's Payload::traces of every frame, concatenated per trace"""
    tr = None
    for f in range(len(data) // fs):
        st, _, _, _, t = ora.frame_decode(data[f * fs:(f + 1) * fs])
        assert st == 0
        tr = [[] for _ in t] if tr is None else tr
        for i, (_, v) in enumerate(t):
            tr[i].append(v)
    return [np.concatenate(t) for t in tr]


def adcdac_words(rng, m, scale=3000):
    """four int16 traces of m samples: the raw wire words make_adcdac_frames takes"""
    return np.clip(rng.standard_normal((4, m)) * scale, -32768, 32767).astype(np.int16)


def spectra(obj, pair):
    """csd() and the raw accumulators of every stage of one pair, as bytes"""
    out = obj.csd(pair)
    st = [obj.stage_spectra(pair, k) for k in range(obj.num_stages(pair))]
    return out, st


def assert_bits(a, b, what):
    (ca, sa), (cb, sb) = a, b
    assert_same_csd(ca, cb, 0, what)
    assert len(sa) == len(sb), what
    for k, (u, v) in enumerate(zip(sa, sb)):
        assert u[0] == v[0], (what, k)
        for p, q in zip(u[1:], v[1:]):
            assert p.tobytes() == q.tobytes(), (what, k)


def raw_call(pkg, bank, data_or_ptr, fs, nf, m, device=False, after=None):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    mp = np.asarray(m, np.uint32)
    ok = C.c_size_t(0)
    if device:
        rc = L.psdc_csd_process_frames_device(bank._h, mp.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(data_or_ptr), fs, nf,
                                              C.byref(ok), C.c_void_p(after) if after else None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_csd_process_frames(bank._h, mp.ctypes.data_as(C.POINTER(C.c_uint32)), buf.ctypes.data_as(C.c_void_p), fs, nf,
                                       C.byref(ok))
    return rc, ok.value


def loss_fields(pkg, obj, cross):
    l = pkg._CLoss()
    L = pkg.lib()
    rc = L.psdc_csd_loss_read(obj._h, C.byref(l), 0) if cross else L.psdc_loss_read(obj._h, C.byref(l), 0)
    assert rc == 0
    return (l.received, l.dropped, l.next_seq, l.have_seq)


@pytest.mark.parametrize("fmt,batches,pair", [(1, 20, (2, 0)), (2, 25, (0, 3)), (3, 18, (1, 2)), (4, 60, (2, 0))])
def test_decode_is_bit_exact(pkg, ora, gpu_required, fmt, batches, pair):
    """One pair, several calls of one piece each: the same bits as psdc_cross_process fed the oracle's traces at the same cuts."""
    n = 1024
    rng = np.random.default_rng(10 * fmt + batches)
    spf = batches * (8 if fmt == 1 else 1)
    nframes = 300_000 // spf
    data, fs = make_frames(fmt, batches, random_payloads(rng, fmt, batches, nframes, wild=False), seq0=7)
    tr = decoded(ora, data, fs)
    cuts = [0, nframes // 7, nframes // 7 + 1, nframes // 2, nframes]
    g = pkg.CsdCascade(n)
    ref = pkg.CsdCascade(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert g.process_frames(data[a * fs:b * fs], fs, pair) == b - a
        ref.process(tr[pair[0]][a * spf:b * spf], tr[pair[1]][a * spf:b * spf])
    assert g.num_stages() >= 2
    assert_bits(spectra(g._b, 0), spectra(ref._b, 0), f"format {fmt}")
    # labels name the same traces
    names = pkg.TRACE_NAMES[pkg.Format(fmt)]
    h = pkg.CsdCascade(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        h.process_frames(data[a * fs:b * fs], fs, (names[pair[0]], names[pair[1]]))
    assert_bits(spectra(h._b, 0), spectra(g._b, 0), "labels")


def test_many_pairs(pkg, ora, gpu_required):
    n = 512
    rng = np.random.default_rng(3)
    batches = 17
    w = adcdac_words(rng, 8 * batches * 9000)
    data, fs = pkg.make_adcdac_frames(w, batches)
    nframes = len(data) // fs
    tr = decoded(ora, data, fs)
    spf = 8 * batches
    full = [("ADC0", "DAC0"), ("ADC1", "DAC1"), ("DAC0", "ADC0"), ("ADC1", "ADC1")]
    idx = [(0, 2), (1, 3), (2, 0), (1, 1)]
    bank = pkg.CsdCascadeBank(n, 4)
    psd = pkg.PsdCascadeBank(n, 4)
    fed = [[] for _ in range(4)]
    cuts = [0, 1, 700, 701, 3000, 3333, 8000, nframes]
    for c, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        pairs = list(full)
        if c in (1, 4):
            pairs[2] = None  # pair 2 sits these calls out
        assert bank.process_frames(data[a * fs:b * fs], fs, pairs) == b - a
        psd.process_frames(data[a * fs:b * fs], fs)
        for p in range(4):
            if pairs[p] is not None:
                fed[p].append((a, b))
    total = 0
    for p in range(4):
        x = np.concatenate([tr[idx[p][0]][a * spf:b * spf] for a, b in fed[p]])
        y = np.concatenate([tr[idx[p][1]][a * spf:b * spf] for a, b in fed[p]])
        total += x.size
        single = pkg.CsdCascade(n)
        single.process(x, y)
        assert_same_csd(bank.csd(p), single.csd(), 2e-6, f"pair {p}")
    assert bank.stats_read()["pairs_in"] == total
    sxx, _, _, br = bank.csd(0)
    pp, pbr = psd.psd(0)
    assert pbr == br
    ref = ora.PsdCascade(n, "f64")
    ref.process(tr[0])
    p_ref, _, _ = ref.psd()
    assert_psd_close(sxx, p_ref, "Sxx of pair 0 vs the f64 oracle", pure=True)
    assert_psd_close(pp, p_ref, "psd() of channel 0 vs the f64 oracle", pure=True)
    xx, yy, xy, _ = bank.csd(3)
    assert np.max(np.abs(pkg.coherence(xx, yy, xy) - 1.0)) <= 1e-5


def test_dac_delayed_adc(pkg, gpu_required):
    """DAC0 = ADC0 delayed by d samples (the DAC word is the delayed ADC word ^ 0x8000): H1 from ADC0 to DAC0 is exp(-2 pi i f d)."""
    n, d = 1024, 3
    rng = np.random.default_rng(9)
    batches = 32
    m = 8 * batches * 8192
    w = adcdac_words(rng, m)
    w[2] = (np.concatenate([np.zeros(d, np.int16), w[0][:-d]]).view(np.uint16) ^ 0x8000).view(np.int16)
    data, fs = pkg.make_adcdac_frames(w, batches)
    g = pkg.CsdCascade(n)
    g.process_frames(data, fs, ("ADC0", "DAC0"))
    sxx, syy, sxy, br = g.csd()
    f = pkg.Break.frequencies(br).astype(np.float64)
    keep = _passband_bins(br, f)
    assert keep.sum() > 500
    h = pkg.transfer(sxx, sxy)
    assert np.max(np.abs(np.abs(h[keep]) - 1.0)) <= 0.02
    assert np.max(np.abs(np.angle(h * np.exp(2j * np.pi * f * d))[keep])) <= 0.01
    assert np.all(pkg.coherence(sxx, syy, sxy)[keep] > 0.99)


def test_host_equals_device(pkg, gpu_required):
    import torch
    n = 1024
    rng = np.random.default_rng(12)
    batches = 255  # 2040 samples a frame: the 2^22-sample pieces cut the 3000-frame call
    w = adcdac_words(rng, 8 * batches * 6000)
    data, fs = pkg.make_adcdac_frames(w, batches, seq0=0xFFFFFF00)
    nframes = len(data) // fs
    pairs = [("ADC0", "DAC0"), None, ("DAC1", "ADC1")]
    cuts = [0, 3, 3000, 4100, nframes]

    def feed_host(obj):
        for a, b in zip(cuts[:-1], cuts[1:]):
            obj.process_frames(data[a * fs:b * fs], fs, pairs)

    def feed_dev(obj, base, after=None):
        for a, b in zip(cuts[:-1], cuts[1:]):
            obj.process_frames_device(base + a * fs, fs, b - a, pairs, after=after)

    def read(obj):
        return [spectra(obj, p) for p in (0, 2)]

    def same(u, v, what):
        for a, b in zip(u, v):
            assert_bits(a, b, what)

    hb = pkg.CsdCascadeBank(n, 3)
    feed_host(hb)
    ref = read(hb)
    ref_loss = loss_fields(pkg, hb, True)
    assert hb.num_stages(1) == 0
    host_bytes = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    for shift in (0, 3):
        buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        buf[shift:shift + len(data)].copy_(host_bytes)
        torch.cuda.synchronize()
        db = pkg.CsdCascadeBank(n, 3)
        feed_dev(db, buf.data_ptr() + shift)
        same(read(db), ref, f"device frames at offset {shift}")
        assert loss_fields(pkg, db, True) == ref_loss
    # a producer on another stream, handed over with an event
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pb = torch.zeros(len(data) + 8, dtype=torch.uint8, device="cuda")
        pb[5:5 + len(data)].copy_(host_bytes.pin_memory(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s)
    eb = pkg.CsdCascadeBank(n, 3)
    feed_dev(eb, pb.data_ptr() + 5, after=ev.cuda_event)
    same(read(eb), ref, "producer event")
    s.synchronize()
    # same calls, same bits; reset + replay == fresh, Loss included
    again = pkg.CsdCascadeBank(n, 3)
    feed_host(again)
    same(read(again), ref, "same calls")
    again.process(1, np.ones(5000, np.float32), np.ones(5000, np.float32))
    again.reset()
    assert loss_fields(pkg, again, True) == (0, 0, 0, 0)
    feed_host(again)
    same(read(again), ref, "reset + replay")
    assert loss_fields(pkg, again, True) == ref_loss


def test_errors_and_loss(pkg, gpu_required):
    n = 256
    rng = np.random.default_rng(5)
    L = pkg.lib()
    # AdcDac (3 batches) and Mpll (8 batches) frames share frame_size 200; seq wraps and has a gap of 7 batches at frame 6
    ad, fs = make_frames(1, 3, random_payloads(rng, 1, 3, 10, wild=False), seq0=0xFFFFFFF4)
    ad = bytearray(ad)
    for f in range(6, 10):
        seq = int.from_bytes(ad[f * fs + 4:f * fs + 8], "little")
        ad[f * fs + 4:f * fs + 8] = ((seq + 7) & 0xFFFFFFFF).to_bytes(4, "little")
    mp, fs2 = make_frames(4, 8, random_payloads(rng, 4, 8, 4, wild=False), seq0=100)
    assert fs == fs2 == 200
    bank = pkg.CsdCascadeBank(n, 2)
    psd = pkg.PsdCascadeBank(n, 4)
    m = [0, 2, 1, 3]  # (ADC0, DAC0), (ADC1, DAC1): Mpll has no trace 3
    rc, ok = raw_call(pkg, bank, bytes(ad) + mp, fs, 14, m)
    assert (rc, ok) == (pkg.ERR_ARG, 10)
    assert "trace 3" in L.psdc_cross_last_error(bank._h).decode()
    psd.process_frames(bytes(ad), fs)
    assert bank.stats_read()["pairs_in"] == 2 * 10 * 24
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    # header-only frames: Loss only
    ho, fs0 = make_frames(1, 0, [b""] * 5, seq0=3)
    assert bank.process_frames(ho, fs0, [(0, 2), (1, 3)]) == 5
    psd.process_frames(ho, fs0)
    assert bank.stats_read()["pairs_in"] == 2 * 10 * 24
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    # a bad header mid-call: the frames before it are ingested
    bad = bytearray(ad)
    bad[4 * fs + 1] = 0
    rc, ok = raw_call(pkg, bank, bytes(bad), fs, 10, m)
    assert (rc, ok) == (pkg.ERR_FRAME_HEADER, 4)
    with pytest.raises(pkg.FrameError):
        psd.process_frames(bytes(bad), fs)
    assert bank.stats_read()["pairs_in"] == 2 * 14 * 24
    assert loss_fields(pkg, bank, True) == loss_fields(pkg, psd, False)
    # an unknown format id and a wrong batch count
    for pos, val, code in ((4 * fs + 2, 9, pkg.ERR_FRAME_FORMAT), (4 * fs + 3, 2, pkg.ERR_FRAME_SIZE)):
        b2 = bytearray(ad)
        b2[pos] = val
        with pytest.raises(pkg.FrameError) as e:
            bank.process_frames(bytes(b2), fs, [(0, 2)])
        assert e.value.code == code
    # map errors ingest nothing
    before = (bank.stats_read()["pairs_in"], loss_fields(pkg, bank, True))
    for mm in ([0, NONE, 1, 3], [0, 2, 4, 1]):
        assert raw_call(pkg, bank, bytes(ad), fs, 10, mm) == (pkg.ERR_ARG, 0)
    ok = C.c_size_t(7)
    buf = np.frombuffer(bytes(ad), np.uint8)
    assert L.psdc_csd_process_frames(bank._h, None, buf.ctypes.data_as(C.c_void_p), fs, 10, C.byref(ok)) == pkg.ERR_ARG
    assert ok.value == 0
    assert (bank.stats_read()["pairs_in"], loss_fields(pkg, bank, True)) == before
    # the same on the device path, through the gather
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(ad) + mp, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    db = pkg.CsdCascadeBank(n, 2)
    rc, ok = raw_call(pkg, db, t.data_ptr(), fs, 14, m, device=True)
    assert (rc, ok) == (pkg.ERR_ARG, 10)
    fresh = pkg.CsdCascadeBank(n, 2)
    raw_call(pkg, fresh, bytes(ad) + mp, fs, 14, m)
    assert loss_fields(pkg, db, True) == loss_fields(pkg, fresh, True)
    assert_same_csd(db.csd(0), fresh.csd(0), 0, "device path after an error")


def test_config_size_and_launches(pkg, ora, gpu_required):
    """2^24 samples a trace of device AdcDac frames at N = 1024, two pairs; a call of one piece is at most five launches."""
    import torch
    n = 1024
    rng = np.random.default_rng(21)
    batches = 128
    m = 1 << 24
    w = adcdac_words(rng, m)
    w[2] = (np.clip(0.5 * w[0].astype(np.float64) + 0.5 * w[2], -32768, 32767).astype(np.int16).view(np.uint16) ^ 0x8000).view(np.int16)
    data, fs = pkg.make_adcdac_frames(w, batches)
    nframes = len(data) // fs
    lsb = np.float32(4.096) * np.float32(2.5) / np.float32(32768.0)
    adc0 = w[0].astype(np.float32) * lsb
    dac0 = (w[2].view(np.uint16) ^ 0x8000).view(np.int16).astype(np.float32) * lsb
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    bank = pkg.CsdCascadeBank(n, 2)
    per_call = (1 << 22) // (8 * batches)  # frames of one piece
    f0 = 0
    while f0 < nframes:
        c = min(per_call, nframes - f0)
        bank.stats_read(reset=True)
        assert bank.process_frames_device(t.data_ptr() + f0 * fs, fs, c, [("ADC0", "DAC0"), ("DAC0", "DAC0")]) == c
        assert bank.stats_read()["launches"] <= 5
        f0 += c
    xx, yy, xy, br = bank.csd(0)
    ref = ora.PsdCascade(n, "f64")
    ref.process(adc0)
    p_ref, _, _ = ref.psd()
    assert_psd_close(xx, p_ref, "Sxx vs the f64 oracle", pure=True)
    ref = ora.PsdCascade(n, "f64")
    ref.process(dac0)
    p_ref, _, _ = ref.psd()
    assert_psd_close(yy, p_ref, "Syy vs the f64 oracle", pure=True)
    _, _, rxy, rbr = stitch_rows(pkg, n, pkg.Window.HANN, restate(ora, adc0, dac0, n), pkg.MergeOpts())
    assert rbr == br
    assert_sxy_close(xy, rxy, xx, yy, 1e-5, "Sxy vs the f64 restatement")
