"""Stream frames into the cross-spectral matrix cascade (psdc_csm_process_frames[_device]): groups of traces against the
oracle's Payload::traces through the f64 restatement, host memory against device memory bit for bit, Loss, frame errors and
map errors.  Semantics: include/psdcascade.h, "cross-spectral matrix cascade"."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_psd_close
from test_cross_host import U32_MAX, restate, stitch_rows
from test_gpu_cross import assert_sxy_close
from test_gpu_cross_frames import adcdac_words, decoded
from test_gpu_payload_formats import make_frames, random_payloads

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ADCDAC = ("ADC0", "ADC1", "DAC0", "DAC1")


def raw_call(pkg, bank, data_or_ptr, fs, nf, gmap, device=False):
    """(rc, n_ok) of one C call (the Python methods raise and lose n_ok)"""
    L = pkg.lib()
    mp = np.asarray(gmap, np.uint32)
    ok = C.c_size_t(0)
    if device:
        rc = L.psdc_csm_process_frames_device(bank._h, mp.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(data_or_ptr), fs, nf,
                                              C.byref(ok), None)
    else:
        buf = np.frombuffer(data_or_ptr, np.uint8)
        rc = L.psdc_csm_process_frames(bank._h, mp.ctypes.data_as(C.POINTER(C.c_uint32)), buf.ctypes.data_as(C.c_void_p), fs, nf,
                                       C.byref(ok))
    return rc, ok.value


def all_bits(bank, group):
    S, br = bank.csd(group)
    st = [bank.stage_spectra(group, k) for k in range(bank.num_stages(group))]
    return S.tobytes(), br, [(i, s.tobytes()) for i, s in st]


def assert_restated(pkg, ora, S, br, tr, n, what):
    """diagonals against the oracle's PsdCascade of each decoded trace, off-diagonals against the f64 restatement"""
    m = S.shape[0]
    avg = (U32_MAX, U32_MAX)
    for a in range(m):
        ref = ora.PsdCascade(n, "f64")
        ref.process(tr[a])
        assert_psd_close(S[a, a].real, ref.psd()[0], f"{what} S[{a},{a}]", pure=True)
        for b in range(a + 1, m):
            st = restate(ora, tr[a], tr[b], n, "hann", "none", avg, "f64")
            rx, ry, rxy, rbr = stitch_rows(pkg, n, pkg.WindowTable.hann(n), st, pkg.MergeOpts())
            assert rbr == br
            assert_sxy_close(S[a, b], rxy, rx, ry, 1e-5, f"{what} S[{a},{b}]")


def test_adcdac_group_host_equals_device(pkg, ora, gpu_required):
    import torch
    n = 1024
    rng = np.random.default_rng(12)
    batches = 40
    w = adcdac_words(rng, 8 * batches * 1500)
    data, fs = pkg.make_adcdac_frames(w, batches, seq0=0xFFFFFF00)
    nframes = len(data) // fs
    tr = decoded(ora, data, fs)
    groups = [None, ADCDAC]
    cuts = [0, 3, 700, 701, nframes]
    hb = pkg.CsmCascadeBank(n, 4, 2)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert hb.process_frames(data[a * fs:b * fs], fs, groups) == b - a
    assert hb.num_stages(0) == 0 and hb.num_stages(1) >= 2
    S, br = hb.csd(1)
    assert_restated(pkg, ora, S, br, tr, n, "AdcDac")
    assert hb.stats_read()["sample_times_in"] == tr[0].size
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    db = pkg.CsmCascadeBank(n, 4, 2)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert db.process_frames_device(buf.data_ptr() + a * fs, fs, b - a, groups) == b - a
    assert all_bits(db, 1) == all_bits(hb, 1)
    assert db.loss() == hb.loss() == {"received": nframes * batches, "dropped": 0}
    # the same traces fed as f32 at the same cuts: the same bits (the decode is Payload::traces)
    spf = 8 * batches
    fb = pkg.CsmCascadeBank(n, 4, 2)
    for a, b in zip(cuts[:-1], cuts[1:]):
        fb.process(1, [t[a * spf:b * spf] for t in tr])
    assert all_bits(fb, 1) == all_bits(hb, 1)


def test_mpll_three_trace_group(pkg, ora, gpu_required):
    import torch
    n = 512
    rng = np.random.default_rng(5)
    batches = 50
    nframes = 4000
    data, fs = make_frames(4, batches, random_payloads(rng, 4, batches, nframes, wild=False), seq0=3)
    tr = decoded(ora, data, fs)
    order = (2, 0, 1)
    h = pkg.CsmCascade(n, 3)
    assert h.process_frames(data, fs, order) == nframes
    S, br = h.csd()
    assert_restated(pkg, ora, S, br, [tr[i] for i in order], n, "Mpll")
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    d = pkg.CsmCascade(n, 3)
    assert d.process_frames_device(buf.data_ptr(), fs, nframes, order) == nframes
    assert all_bits(d._b, 0) == all_bits(h._b, 0)
    # a four-trace group on an Mpll run fails at the run's first frame
    four = pkg.CsmCascadeBank(n, 4, 1)
    rc, ok = raw_call(pkg, four, data, fs, nframes, [0, 1, 2, 3])
    assert (rc, ok) == (pkg.ERR_ARG, 0)
    msg = pkg.lib().psdc_csm_last_error(four._h).decode()
    assert "trace 3" in msg and "Mpll" in msg
    assert four.num_stages(0) == 0


def test_loss_gap_and_bad_frame(pkg, gpu_required):
    import torch
    n = 256
    rng = np.random.default_rng(8)
    batches = 10
    w = adcdac_words(rng, 8 * batches * 900)
    data, fs = pkg.make_adcdac_frames(w, batches)
    nframes = len(data) // fs
    gmap = [0, 1, 2, 3]
    # a gap: frames 300 ... 349 never arrive
    gap = data[:300 * fs] + data[350 * fs:]
    g = pkg.CsmCascadeBank(n, 4, 1)
    assert g.process_frames(gap, fs, [ADCDAC]) == nframes - 50
    assert g.loss() == {"received": (nframes - 50) * batches, "dropped": 50 * batches}
    assert g.loss(reset=True)["dropped"] == 50 * batches and g.loss() == {"received": 0, "dropped": 0}
    # a bad frame in the middle: the frames before it are ingested, n_ok counts them
    bad = bytearray(data)
    bad[500 * fs] ^= 0xFF  # the magic
    ref = pkg.CsmCascadeBank(n, 4, 1)
    ref.process_frames(data[:500 * fs], fs, [ADCDAC])
    for device in (False, True):
        b = pkg.CsmCascadeBank(n, 4, 1)
        if device:
            buf = torch.frombuffer(bytearray(bad), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            rc, ok = raw_call(pkg, b, buf.data_ptr(), fs, nframes, gmap, device=True)
        else:
            rc, ok = raw_call(pkg, b, bytes(bad), fs, nframes, gmap)
        assert (rc, ok) == (pkg.ERR_FRAME_HEADER, 500), device
        assert "frame 500" in pkg.lib().psdc_csm_last_error(b._h).decode()
        assert all_bits(b, 0) == all_bits(ref, 0)
        with pytest.raises(pkg.FrameError):
            b.process_frames(bytes(bad[500 * fs:]), fs, [ADCDAC])


def test_map_errors(pkg, gpu_required):
    n = 256
    rng = np.random.default_rng(1)
    data, fs = pkg.make_adcdac_frames(adcdac_words(rng, 8 * 10 * 100), 10)
    nframes = len(data) // fs
    b = pkg.CsmCascadeBank(n, 3, 2)
    for gmap in ([0, 1, NONE, NONE, NONE, NONE], [NONE, NONE, NONE, 0, NONE, 2]):
        rc, ok = raw_call(pkg, b, data, fs, nframes, gmap)
        assert (rc, ok) == (pkg.ERR_ARG, 0)
        assert "PSDC_TRACE_NONE" in pkg.lib().psdc_csm_last_error(b._h).decode()
    rc, ok = raw_call(pkg, b, data, fs, nframes, [0, 1, 4, NONE, NONE, NONE])
    assert (rc, ok) == (pkg.ERR_ARG, 0) and "trace 4" in pkg.lib().psdc_csm_last_error(b._h).decode()
    assert b.num_stages(0) == 0 and b.num_stages(1) == 0 and b.loss() == {"received": 0, "dropped": 0}
    # nothing fed: Loss only
    rc, ok = raw_call(pkg, b, data, fs, nframes, [NONE] * 6)
    assert (rc, ok) == (0, nframes) and b.num_stages(0) == 0 and b.loss()["received"] == nframes * 10
    # a trace may feed several channels and groups
    assert b.process_frames(data, fs, [("ADC0", "ADC0", "DAC1"), (3, 2, 0)]) == nframes
    S, _ = b.csd(0)
    assert np.all(np.abs(S[0, 1].real - S[0, 0].real) <= 1e-6 * S[0, 0].real)
    S1, _ = b.csd(1)
    assert np.all(np.abs(S1[2, 2].real - S[0, 0].real) <= 2e-6 * S[0, 0].real)  # ADC0 is channel 2 of group 1
