"""Bank read-out on the MI355X (include/psdcascade_readout.h, psdcr_*; stabilizer-stream_amd/bankread.py): one call stitches every
selected channel of a PsdCascadeBank on the device.  Every PSD value, frequency, length and Break must equal what psd(channel) and
Break.frequencies return, byte for byte and field for field; the device form writes exactly lens[i] values a row; band powers
are deterministic f64 sums checked against numpy and against Trace::plot's f32 integral.

Shapes: n = 64 (generic kernels) and n = 1024 (fused kernels) with the Hann window, n = 256 with the rectangular window; a bank of
five channels -- three or more stages, an odd length, one stage of one or two segments, no stage at all, and one with half a call
still in host staging when the first read-out is made -- fed in several process calls; one bank under set_avg with a small limit
and one under Mean detrend."""
import ctypes as C
import filecmp
import itertools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AC3C3  # the bit pattern the device outputs are pre-filled with
# name: (n, window, samples of channels 0 and 4, of channel 1, of channel 2, set_avg, detrend)
SHAPES = {
    "n64": (64, "HANN", 1 << 14, 5000, 100, None, None),
    "n1024": (1024, "HANN", 1 << 18, 5000 * 16, 1600, None, None),
    "n256rect": (256, "RECTANGULAR", 1 << 16, 5000 * 4, 400, None, None),
    "n64avg": (64, "HANN", 1 << 14, 5000, 100, (7, 900), None),
    "n1024mean": (1024, "HANN", 1 << 18, 5000 * 16, 1600, None, "MEAN"),
}
EMPTY = 3  # the channel that is never fed
SELECTIONS = {"all": None, "permutation": [4, 2, 0, 3, 1], "subset with a duplicate": [1, 4, 1], "the empty channel alone": [EMPTY]}


def all_opts(pkg):
    return [pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)
            for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 2, 10 ** 6))]


@pytest.fixture(scope="module")
def bankread(pkg):
    from stabilizer_stream_amd import bankread as mod
    return mod


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request, pkg, bankread, gpu_required):
    """one fed bank a shape: dict(bank, clone, first, ref).  `first` is the bank read-out made while channel 4 had half a call in
    host staging; `clone` was taken right after it and never sees a bank read-out; ref[opts] = [(psd, breaks, frequencies)] of
    every channel from psd(c), computed once"""
    n, window, long, mid, short, avg, detrend = SHAPES[request.param]
    bank = pkg.PsdCascadeBank(n, 5, getattr(pkg.Window, window))
    if avg:
        bank.set_avg(pkg.AvgOpts(*avg))
    if detrend:
        bank.set_detrend(getattr(pkg.Detrend, detrend))
    x = pkg.noise_host(long, seed=1000 + n)
    piece = long // 4
    for k in range(4):
        bank.process(0, x[k * piece:(k + 1) * piece])
    y = pkg.noise_host(mid, seed=2000 + n)
    for part in np.array_split(y, 3):
        bank.process(1, part)
    bank.process(2, pkg.noise_host(short, seed=3000 + n))
    for k in range(3):
        bank.process(4, x[k * piece:(k + 1) * piece])
    bank.process(4, x[3 * piece:3 * piece + piece // 2])
    bank.flush()
    bank.process(4, x[3 * piece + piece // 2:])  # half a call: in host staging when the read-out below is made
    first = bankread.bank_psd(bank, frequencies=True)
    clone = bank.clone()
    ref = {}
    for opts in all_opts(pkg):
        rows = [bank.psd(c, opts) for c in range(5)]
        ref[opts] = [(p, br, pkg.Break.frequencies(br)) for p, br in rows]
    yield dict(bank=bank, clone=clone, first=first, ref=ref, n=n, name=request.param)
    clone.close()
    bank.close()


def check_rows(got, ref, channels, what, frequencies=True):
    """a bank read-out's rows, lens and breaks against psd(c) of each selected channel"""
    sel = range(len(ref)) if channels is None else channels
    assert got["psd"].dtype == np.float32 and got["psd"].shape == (len(sel), max([len(ref[c][0]) for c in sel] or [0])), what
    for i, c in enumerate(sel):
        p, br, f = ref[c]
        assert got["lens"][i] == len(p), (what, i)
        assert got["breaks"][i] == br, (what, i)  # field for field (a frozen dataclass)
        assert got["psd"][i, :len(p)].tobytes() == p.tobytes(), (what, i)
        assert np.all(np.isnan(got["psd"][i, len(p):])), (what, i)
        if frequencies:
            assert got["frequencies"][i, :len(p)].tobytes() == f.tobytes(), (what, i)
            assert np.all(np.isnan(got["frequencies"][i, len(p):])), (what, i)


def test_shape_is_what_the_cases_need(state):
    rows = next(iter(state["ref"].values()))
    live = [sum(b.count > 0 for b in br) for _, br, _ in rows]  # stages that hold a segment
    print(state["name"], "live stages", live, "stage-0 counts", [br[-1].count if br else None for _, br, _ in rows])
    assert live[0] >= 3 and live[4] == live[0] and live[1] >= 2 and live[2] == 1 and live[EMPTY] == 0 and not rows[EMPTY][1], live
    assert 1 <= rows[2][1][-1].count <= 2


def test_first_read_out_with_samples_in_host_staging(pkg, state):
    ref = [(p, br, pkg.Break.frequencies(br)) for p, br in (state["bank"].psd(c) for c in range(5))]  # (the default options)
    check_rows(state["first"], ref, None, "first read-out")
    assert state["first"]["launches"] == 1


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_host_form_equals_psd(pkg, bankread, state, selection):
    """rows, lens, breaks and frequencies for every merge-option combination and min_count 0, 2 and 10^6"""
    channels = SELECTIONS[selection]
    for opts in all_opts(pkg):
        got = bankread.bank_psd(state["bank"], channels, opts, frequencies=True)
        check_rows(got, state["ref"][opts], channels, (state["name"], selection, opts))
        included = any(b.include for c in (range(5) if channels is None else channels) for b in state["ref"][opts][c][1])
        assert got["launches"] == (1 if included else 0), (selection, opts)
        lay = bankread.layout(state["bank"], channels, opts)
        assert lay["lens"] == got["lens"] and lay["breaks"] == got["breaks"] and lay["max_len"] == got["psd"].shape[1]
        only = bankread.bank_psd(state["bank"], channels, opts)
        assert "frequencies" not in only and only["psd"].tobytes() == got["psd"].tobytes()


def test_the_read_out_changes_nothing(pkg, bankread, state):
    """psd(c) after all of the above equals psd(c) of the clone that never saw a bank read-out"""
    bankread.bank_psd(state["bank"], frequencies=True, bands=[(0.0, 0.5)])
    for c in range(5):
        for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True)):
            a, abr = state["bank"].psd(c, opts)
            b, bbr = state["clone"].psd(c, opts)
            assert a.tobytes() == b.tobytes() and abr == bbr, (c, opts)


def device_tensor(torch, rows, stride, tail=13):
    t = torch.full((rows * stride + tail,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def check_device_rows(t, host_rows, lens, stride, what):
    """row i holds the host form's bytes in [0, lens[i]); every other element, and everything behind the last row, is the sentinel"""
    got = t.cpu().numpy()
    want = np.full(got.shape, SENTINEL, np.int32)
    for i, ln in enumerate(lens):
        want[i * stride:i * stride + ln] = host_rows[i, :ln].view(np.int32)
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("selection", ["all", "subset with a duplicate"])
def test_device_form(pkg, bankread, state, selection):
    import torch
    channels = SELECTIONS[selection]
    rows = 5 if channels is None else len(channels)
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True)):
        host = bankread.bank_psd(state["bank"], channels, opts, frequencies=True)
        stride = host["psd"].shape[1] + 7
        tp, tf = device_tensor(torch, rows, stride), device_tensor(torch, rows, stride)
        got = bankread.bank_psd_device(state["bank"], tp.data_ptr(), stride, channels, opts, freq_ptr=tf.data_ptr())
        assert got["lens"] == host["lens"] and got["breaks"] == host["breaks"] and got["launches"] == 1
        check_device_rows(tp, host["psd"], host["lens"], stride, "psd")
        check_device_rows(tf, host["frequencies"], host["lens"], stride, "frequencies")
        # each output alone
        tp2, tf2 = device_tensor(torch, rows, stride), device_tensor(torch, rows, stride)
        assert bankread.bank_psd_device(state["bank"], tp2.data_ptr(), stride, channels, opts)["launches"] == 1
        assert bankread.bank_psd_device(state["bank"], None, stride, channels, opts, freq_ptr=tf2.data_ptr())["launches"] == 1
        check_device_rows(tp2, host["psd"], host["lens"], stride, "psd alone")
        check_device_rows(tf2, host["frequencies"], host["lens"], stride, "frequencies alone")


def test_done_event_form(pkg, bankread, state):
    """the call that returns early, waited for through its event; two of them back to back with different options, each into its
    own tensor (the two job-table slots), and a third and fourth behind them (a slot is reused)"""
    import torch
    opts = [pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True), pkg.MergeOpts(min_count=2),
            pkg.MergeOpts(keep_transition_band=True)]
    host = [bankread.bank_psd(state["bank"], None, o) for o in opts]
    stride = max(h["psd"].shape[1] for h in host) + 7
    tensors = [device_tensor(torch, 5, stride) for _ in opts]
    events = []
    for _ in opts:
        ev = torch.cuda.Event()
        ev.record()  # (the handle exists once the event has been recorded)
        events.append(ev)
    torch.cuda.synchronize()
    got = bankread.bank_psd_device(state["bank"], tensors[0].data_ptr(), stride, None, opts[0], done_event=events[0].cuda_event)
    events[0].synchronize()
    check_device_rows(tensors[0], host[0]["psd"], host[0]["lens"], stride, "one call")
    assert got["lens"] == host[0]["lens"] and got["launches"] == 1
    tensors[0] = device_tensor(torch, 5, stride)
    for t, o, ev in zip(tensors, opts, events):  # back to back, no wait in between
        bankread.bank_psd_device(state["bank"], t.data_ptr(), stride, None, o, done_event=ev.cuda_event)
    for k, (t, h, ev) in enumerate(zip(tensors, host, events)):
        ev.synchronize()
        check_device_rows(t, h["psd"], h["lens"], stride, f"call {k} of four back to back")


def bands_of(n):
    """the whole range; one decade that lies inside stage 0 when the overlap is kept (with the default options a stage spans a
    factor of 8, so there it crosses a seam too); a decade across a seam; a single bin (k = n/4 of stage 0); none"""
    return [(0.0, 0.5), (0.0501, 0.5), (0.01, 0.1), (0.25, 0.25), (0.30001, 0.30002)]


def band_reference(psd, freq, bands):
    p, f = psd.astype(np.float64), freq.astype(np.float64)
    t = 0.5 * (p + np.concatenate(([0.0], p[:-1]))) * (f - np.concatenate(([0.0], f[:-1])))
    out = []
    for lo, hi in np.asarray(bands, np.float32):
        m = (freq >= lo) & (freq <= hi)
        out.append((float(np.sum(t[m])), len(psd) * 2.0 ** -52 * float(np.sum(np.abs(t[m]))), int(m.sum())))
    return out


def test_band_power(pkg, bankread, state):
    import torch
    bank, bands = state["bank"], bands_of(state["n"])
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True)):
        got = bankread.bank_psd(bank, None, opts, frequencies=True, bands=bands)
        assert got["launches"] == 2 and got["band_power"].shape == (5, len(bands)) and got["band_power"].dtype == np.float64
        check_rows(got, [(p, br, pkg.Break.frequencies(br)) for p, br in (bank.psd(c, opts) for c in range(5))], None, "with bands")
        for c in range(5):
            ln = got["lens"][c]
            row, freq = got["psd"][c, :ln], got["frequencies"][c, :ln]
            for b, (want, tol, count) in enumerate(band_reference(row, freq, bands)):
                print(state["name"], "keep_overlap", opts.keep_overlap, "channel", c, "band", b, "bins", count, "got", got["band_power"][c, b],
                      "numpy", want, "tol", tol)
                assert abs(got["band_power"][c, b] - want) <= tol, (c, b)
                if count == 0:
                    assert got["band_power"][c, b] == 0.0
            if c == 0:
                counts = [r[2] for r in band_reference(row, freq, bands)]
                assert counts[0] == ln and counts[3] == 1 and counts[4] == 0 and counts[1] > 1 and counts[2] > 1, counts
            if opts == pkg.MergeOpts() and ln:  # Trace::plot's sequential f32 integral over the same limits, fs = 1
                for b, (lo, hi) in enumerate(np.asarray(bands, np.float32)):
                    rms = pkg.trace_plot(row, freq, 1.0, False, float(lo), float(hi), plot=False)[0]
                    print("   rms", rms, "sqrt(band)", np.sqrt(got["band_power"][c, b]))
                    assert abs(np.sqrt(got["band_power"][c, b]) - rms) <= ln * 2.0 ** -24 * rms, (c, b)
        assert np.all(got["band_power"][EMPTY] == 0.0)
        # the same bits from a second call, from bands alone, and from the device form
        again = bankread.bank_psd(bank, None, opts, bands=bands)
        assert again["band_power"].tobytes() == got["band_power"].tobytes()
        tb = torch.full((5 * len(bands) + 3,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev = bankread.bank_psd_device(bank, None, 0, None, opts, bands=bands, band_ptr=tb.data_ptr())
        assert dev["launches"] == 1
        out = tb.cpu().numpy()
        assert out[:5 * len(bands)].tobytes() == got["band_power"].tobytes() and np.all(out[5 * len(bands):] == -1.0)
        stride = got["psd"].shape[1] + 7
        tp = device_tensor(torch, 5, stride)
        tb.fill_(-1.0)
        torch.cuda.synchronize()
        dev = bankread.bank_psd_device(bank, tp.data_ptr(), stride, None, opts, bands=bands, band_ptr=tb.data_ptr())
        assert dev["launches"] == 2
        assert tb.cpu().numpy()[:5 * len(bands)].tobytes() == got["band_power"].tobytes()
        check_device_rows(tp, got["psd"], got["lens"], stride, "psd with bands")
    # the empty channel alone: nothing is launched, the band powers are 0.0
    tb = torch.full((len(bands),), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = bankread.bank_psd_device(bank, None, 0, [EMPTY], bands=bands, band_ptr=tb.data_ptr())
    assert dev["launches"] == 0 and np.all(tb.cpu().numpy() == 0.0)
    alone = bankread.bank_psd(bank, [EMPTY], bands=bands)
    assert alone["launches"] == 0 and alone["psd"].shape == (1, 0) and np.all(alone["band_power"] == 0.0)


def test_band_bits_equal_the_host_restatement(pkg, bankread, state, tmp_path_factory):
    """The device band sums carry the bits of bank_band_row_host (csrc/bank_readout.h run on the CPU by
    tests/host/bank_readout_check.cpp) on the channel's own accumulators and Breaks: every product rounded before it is added
    (no fused multiply-add on the device), thread t over the elements t, t + 256, ..., the shuffle tree, the wavefronts in order"""
    from test_waterfall_host import host_exe
    bank, bands = state["bank"], bands_of(state["n"])
    _, wt = bank.window_get()
    d = tmp_path_factory.mktemp("bank_band_bits")
    exe = host_exe(d, "bank_readout_check", False)
    nonzero = 0
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True)):
        got = bankread.bank_psd(bank, None, opts, frequencies=True, bands=bands)
        blob = [struct.pack("<I", 5)]
        for c in range(5):
            stats, spectra = bank.read_channel(c)
            breaks = got["breaks"][c]
            assert len(breaks) == len(stats) and [b.count for b in breaks[::-1]] == [st["count"] for st in stats]
            blob.append(struct.pack("<4I2f", state["n"], len(stats), len(breaks), len(bands), wt.nenbw, wt.power))
            blob.append(np.asarray([st["count"] for st in stats], np.uint64).tobytes())
            blob += [bytes(b._c()) for b in breaks]
            blob.append(np.ascontiguousarray(spectra, np.float32).tobytes())
            blob.append(np.asarray(bands, np.float32).tobytes())
        src, dst = str(d / "cases.bin"), str(d / "rows.bin")
        with open(src, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        raw, pos = open(dst, "rb").read(), 0
        for c in range(5):
            ln = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            assert ln == got["lens"][c]
            assert raw[pos + 8:pos + 8 + 4 * ln] == got["psd"][c, :ln].tobytes()
            assert raw[pos + 8 + 4 * ln:pos + 8 + 8 * ln] == got["frequencies"][c, :ln].tobytes()
            host = np.frombuffer(raw, np.float64, len(bands), pos + 8 + 8 * ln)
            print(state["name"], opts.keep_overlap, "channel", c, "device", got["band_power"][c], "host", host)
            assert host.tobytes() == got["band_power"][c].tobytes(), (c, host, got["band_power"][c])
            nonzero += int(np.count_nonzero(host))
            pos += 8 + 8 * ln + 8 * len(bands)
        assert pos == len(raw)
    assert nonzero >= 2 * 4 * 4  # four fed channels, four bands that hold bins, two option sets


def test_seventy_channels_in_one_launch(pkg, bankread, gpu_required):
    """a bank of 70 channels of which 3 are fed, all 70 selected: one launch, two with bands"""
    bank = pkg.PsdCascadeBank(64, 70)
    fed = (3, 40, 69)
    for c in fed:
        bank.process(c, pkg.noise_host(3000 + c, seed=c))
    got = bankread.bank_psd(bank, frequencies=True, bands=[(0.0, 0.5), (0.01, 0.1)])
    assert got["launches"] == 2 and bankread.bank_psd(bank)["launches"] == 1
    for c in range(70):
        p, br = bank.psd(c)
        assert got["lens"][c] == len(p) and got["breaks"][c] == br
        assert got["psd"][c, :len(p)].tobytes() == p.tobytes()
        assert (len(p) > 0) == (c in fed)
        if c not in fed:
            assert np.all(got["band_power"][c] == 0.0)
    sel = list(range(69, -1, -1)) * 2
    twice = bankread.bank_psd(bank, sel)
    assert twice["launches"] == 1 and twice["psd"].shape[0] == 140
    assert twice["psd"][0].tobytes() == got["psd"][69].tobytes() and twice["psd"][70 + 29].tobytes() == got["psd"][40].tobytes()
    bankread.release(bank)  # the buffers come back with the next call
    assert bankread.bank_psd(bank)["psd"].tobytes() == got["psd"].tobytes()
    single = pkg.PsdCascade(64)
    single.process(pkg.noise_host(3003, seed=3))
    one = bankread.bank_psd(single)
    assert one["psd"][0].tobytes() == got["psd"][3, :one["lens"][0]].tobytes() == single.psd()[0].tobytes()
    single.close()
    bank.close()


def test_errors(pkg, bankread, state):
    import torch
    bank = state["bank"]
    L = bankread._lib()
    lay = bankread.layout(bank)
    stride = lay["max_len"] - 1
    t = device_tensor(torch, 5, lay["max_len"])
    c = bankread._Call(bank, None, None)
    rc = L.psdcr_bank_psd_device(*c.head, C.c_void_p(t.data_ptr()), None, stride, None, 0, None, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and "stride" in pkg.lib().psdc_last_error(bank._h).decode()
    assert c.result()["lens"] == lay["lens"] and int(c.info.max_len) == lay["max_len"] and int(c.info.launches) == 0
    assert np.all(t.cpu().numpy() == SENTINEL)
    host = np.zeros((5, lay["max_len"]), np.float32)
    c = bankread._Call(bank, None, None)
    rc = L.psdcr_bank_psd(*c.head, host.ctypes.data, None, stride, None, 0, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and c.result()["lens"] == lay["lens"] and np.all(host == 0)
    c = bankread._Call(bank, None, None)  # room for fewer breaks than channel 0 has
    rc = L.psdcr_bank_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, 2, C.byref(c.info))
    assert rc == pkg.ERR_CAPACITY and [int(v) for v in c.lens] == lay["lens"] and int(c.nb[0]) == len(lay["breaks"][0])

    def arg_error(text, fn, *args, **kw):
        with pytest.raises(pkg.PsdError) as e:
            fn(bank, *args, **kw)
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))

    ptr = t.data_ptr()
    arg_error("channel out of range", bankread.bank_psd, [0, 5])
    arg_error("channel out of range", bankread.layout, [5])
    arg_error("channel out of range", bankread.bank_psd_device, ptr, lay["max_len"], [7])
    arg_error("more than 8 bands", bankread.bank_psd_device, ptr, lay["max_len"], bands=[(0.0, 0.1)] * 9, band_ptr=ptr)
    arg_error("bands without a band output", bankread.bank_psd_device, ptr, lay["max_len"], bands=[(0.0, 0.1)])
    arg_error("a band output without bands", bankread.bank_psd_device, ptr, lay["max_len"], band_ptr=ptr)
    arg_error("a band with NaN or lo > hi", bankread.bank_psd, bands=[(0.0, 0.1), (float("nan"), 0.2)])
    arg_error("a band with NaN or lo > hi", bankread.bank_psd, bands=[(0.2, 0.1)])
    arg_error("no output", bankread.bank_psd_device, None, lay["max_len"])
    c = bankread._Call(bank, None, None)  # a band count and a band output, but no band list
    rc = L.psdcr_bank_psd_device(*c.head, None, None, 0, None, 2, C.c_void_p(ptr), None, *c.tail)
    assert rc == pkg.ERR_ARG and pkg.lib().psdc_last_error(bank._h).decode() == "psdcr_bank_psd_device: n_bands without a band list"
    c = bankread._Call(bank, None, None)
    rc = L.psdcr_bank_layout(*c.head, None, c.nb.ctypes.data, None, 0, None)
    assert rc == pkg.ERR_ARG and pkg.lib().psdc_last_error(bank._h).decode() == "psdcr_bank_layout: null lens"
    assert np.all(t.cpu().numpy() == SENTINEL)


def test_cli_flag_gives_the_same_files(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --bank-readout reads the four traces of a frames file with one bank_psd call: the same lines, the same files"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batches, frames = 8, 700
    words = np.random.default_rng(5).integers(-20000, 20000, (4, 8 * batches * frames)).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(words, batches, seq0=1)
    path = tmp_path / "frames.bin"
    path.write_bytes(data)
    outs = []
    for extra in ([], ["--bank-readout"]):
        d = tmp_path / ("csv" + str(len(extra)))
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--file", str(path), "--frame-size", str(fs),
                            "--csv", str(d), "--integrate"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append((r.stdout, d))
    assert outs[0][0] == outs[1][0] and outs[0][0].count(" stages ") == 4 and "no samples" not in outs[0][0], outs[0][0]
    names = sorted(os.listdir(outs[0][1]))
    assert len(names) == 4 and names == sorted(os.listdir(outs[1][1]))
    for name in names:
        assert filecmp.cmp(outs[0][1] / name, outs[1][1] / name, shallow=False), name
