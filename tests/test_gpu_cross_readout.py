"""Bank read-out of the pair and matrix objects on the MI355X (include/psdcascade_crossread.h, psdcxr_*;
stabilizer-stream_amd/crossread.py): one call stitches every selected pair of a CsdCascadeBank (group of a CsmCascadeBank) on the
device.  Every f32 value, frequency, length and Break must equal what csd(unit) and Break.frequencies return, byte for byte and
field for field; the device form writes exactly lens[i] bins a row; coherence and H1 come from the f64 accumulators and are held to
numpy f64 on their f32 casts; the band sums are deterministic f64 sums checked against numpy and, bit for bit, against the host
restatement.

Shapes: n = 64 (33 bins: one tile) and n = 1024 (513 bins: the third tile of a job holds ONE element) with the Hann window,
n = 256 with the rectangular window; one bank under set_avg with a small limit and one under Mean detrend.  A bank has six pairs --
three or more live stages, an odd length fed y = 2 x, one stage of one or two segments, never fed, both streams all zeros (the NaN
paths), and a twin of the first whose last half call is fed right before the first read-out -- fed in several process calls.  The
pair object has no clone(): `twin` is a second bank fed the same calls that never sees a bank read-out."""
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
# name: (n, window, samples of pairs 0 and 5, of pair 1 and 4, of pair 2, set_avg, detrend)
SHAPES = {
    "n64": (64, "HANN", 1 << 14, 5001, 100, None, None),
    "n1024": (1024, "HANN", 1 << 18, 5000 * 16 + 1, 1600, None, None),
    "n256rect": (256, "RECTANGULAR", 1 << 16, 5000 * 4 + 1, 400, None, None),
    "n64avg": (64, "HANN", 1 << 14, 5001, 100, (7, 900), None),
    "n1024mean": (1024, "HANN", 1 << 18, 5000 * 16 + 1, 1600, None, "MEAN"),
}
LONG, DOUBLE, SHORT, EMPTY, ZEROS, TWIN = range(6)  # DOUBLE: y = 2 x
SELECTIONS = {"all": None, "permutation": [4, 2, 0, 5, 3, 1], "subset with a duplicate": [1, 5, 1], "the unfed pair alone": [EMPTY]}
PAIR_OUTS = (("sxx", 1), ("syy", 1), ("sxy", 2), ("frequencies", 1), ("coherence", 2), ("transfer", 4))  # (key, 32-bit words a bin)
DEVICE_ARG = {"frequencies": "freq"}
U = 2.0 ** -24


def all_opts(pkg):
    return [pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)
            for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 2, 10 ** 6))]


@pytest.fixture(scope="module")
def crossread(pkg):
    from stabilizer_stream_amd import crossread as mod
    return mod


def feed(pkg, bank, n, long, mid, short, last_half):
    """the calls of a bank; last_half: called right before the TWIN pair's last half call"""
    x = pkg.noise_host(long, seed=1000 + n)
    y = (0.6 * x + 0.8 * pkg.noise_host(long, seed=1500 + n)).astype(np.float32)
    piece = long // 4
    for k in range(4):
        bank.process(LONG, x[k * piece:(k + 1) * piece], y[k * piece:(k + 1) * piece])
    z = pkg.noise_host(mid, seed=2000 + n)
    for part in np.array_split(z, 3):
        bank.process(DOUBLE, part, 2.0 * part)
    s = pkg.noise_host(short, seed=3000 + n)
    bank.process(SHORT, s, s[::-1].copy())
    for part in np.array_split(np.zeros(mid, np.float32), 2):
        bank.process(ZEROS, part, part)
    for k in range(3):
        bank.process(TWIN, x[k * piece:(k + 1) * piece], y[k * piece:(k + 1) * piece])
    half = 3 * piece + piece // 2
    bank.process(TWIN, x[3 * piece:half], y[3 * piece:half])
    last_half()
    bank.process(TWIN, x[half:], y[half:])


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request, pkg, crossread, gpu_required):
    """one fed bank a shape: dict(bank, twin, first, ref).  `first` is the bank read-out made right behind the TWIN pair's last
    half call; `twin` is a second bank fed the same calls that never sees a bank read-out; ref[opts] = [(sxx, syy, sxy, breaks,
    frequencies)] of every pair from csd(p), computed once"""
    n, window, long, mid, short, avg, detrend = SHAPES[request.param]
    banks = []
    for _ in range(2):
        bank = pkg.CsdCascadeBank(n, 6, getattr(pkg.Window, window))
        if avg:
            bank.set_avg(pkg.AvgOpts(*avg))
        if detrend:
            bank.set_detrend(getattr(pkg.Detrend, detrend))
        feed(pkg, bank, n, long, mid, short, bank.sync)
        banks.append(bank)
    bank, twin = banks
    first = crossread.bank_csd(bank, frequencies=True, coherence=True, transfer=True)
    ref = {}
    for opts in all_opts(pkg) + [pkg.MergeOpts()]:
        ref[opts] = [(*r, pkg.Break.frequencies(r[3])) for r in (bank.csd(p, opts) for p in range(6))]
    yield dict(bank=bank, twin=twin, first=first, ref=ref, n=n, name=request.param, window=window)
    twin.close()
    bank.close()


def check_rows(got, ref, pairs, what):
    """a bank read-out's rows, lens and breaks against csd(p) of each selected pair"""
    sel = range(len(ref)) if pairs is None else pairs
    width = max([len(ref[p][0]) for p in sel] or [0])
    for key, dtype in (("sxx", np.float32), ("syy", np.float32), ("sxy", np.complex64), ("frequencies", np.float32)):
        assert got[key].dtype == dtype and got[key].shape == (len(sel), width), (what, key)
    for i, p in enumerate(sel):
        xx, yy, xy, br, f = ref[p]
        assert got["lens"][i] == len(xx), (what, i)
        assert got["breaks"][i] == br, (what, i)  # field for field (a frozen dataclass)
        for key, want in (("sxx", xx), ("syy", yy), ("sxy", xy), ("frequencies", f)):
            assert got[key][i, :len(xx)].tobytes() == want.tobytes(), (what, i, key)
            assert np.all(np.isnan(got[key][i, len(xx):])), (what, i, key)


def test_shape_is_what_the_cases_need(pkg, state):
    rows = next(iter(state["ref"].values()))
    live = [sum(b.count > 0 for b in r[3]) for r in rows]  # stages that hold a segment
    print(state["name"], "live stages", live, "stage-0 counts", [r[3][-1].count if r[3] else None for r in rows])
    assert live[LONG] >= 3 and live[TWIN] == live[LONG] and live[DOUBLE] >= 2 and live[SHORT] == 1 and live[EMPTY] == 0 and not rows[EMPTY][3], live
    assert 1 <= rows[SHORT][3][-1].count <= 2 and live[ZEROS] >= 2
    assert all(np.all((v == 0) | np.isnan(v)) for v in rows[ZEROS][:3])  # (NaN: a stage without a segment, included by min_count = 0)
    if state["n"] == 1024:  # a job of 513 bins: three tiles, the last of one element
        assert any(len(b.bins) == 513 for b in state["bank"].csd(LONG, pkg.MergeOpts(keep_transition_band=True))[3])


def test_first_read_out_behind_a_half_call(pkg, state):
    ref = [(*r, pkg.Break.frequencies(r[3])) for r in (state["bank"].csd(p) for p in range(6))]  # (the default options)
    check_rows(state["first"], ref, None, "first read-out")
    assert state["first"]["launches"] == 1


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_host_form_equals_csd(pkg, crossread, state, selection):
    """rows, lens, breaks and frequencies for every merge-option combination and min_count 0, 2 and 10^6"""
    pairs = SELECTIONS[selection]
    for opts in all_opts(pkg):
        got = crossread.bank_csd(state["bank"], pairs, opts, frequencies=True)
        check_rows(got, state["ref"][opts], pairs, (state["name"], selection, opts))
        included = any(b.include for p in (range(6) if pairs is None else pairs) for b in state["ref"][opts][p][3])
        assert got["launches"] == (1 if included else 0), (selection, opts)
        lay = crossread.layout(state["bank"], pairs, opts)
        assert lay["lens"] == got["lens"] and lay["breaks"] == got["breaks"] and lay["max_len"] == got["sxx"].shape[1]
        only = crossread.bank_csd(state["bank"], pairs, opts)
        assert "frequencies" not in only and "coherence" not in only and only["sxy"].tobytes() == got["sxy"].tobytes()


def test_the_read_out_changes_nothing(pkg, crossread, state):
    """csd(p) after all of the above equals what it was before them, and csd(p) of the twin bank that never saw a bank read-out"""
    crossread.bank_csd(state["bank"], frequencies=True, coherence=True, transfer=True, bands=[(0.0, 0.5)])
    for p in range(6):
        for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True)):
            a, b, before = state["bank"].csd(p, opts), state["twin"].csd(p, opts), state["ref"][opts][p]
            for k in range(3):
                assert a[k].tobytes() == b[k].tobytes() == before[k].tobytes(), (p, opts, k)
            assert a[3] == b[3] == before[3], (p, opts)


def device_tensor(torch, rows, stride, words=1, tail=13):
    t = torch.full((rows * stride * words + tail,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def check_device_rows(t, host_rows, lens, stride, words, what):
    """row i holds the host form's bytes in [0, lens[i]) bins of `words` 32-bit words; every other word, and everything behind the
    last row, is the sentinel"""
    got = t.cpu().numpy()
    want = np.full(got.shape, SENTINEL, np.int32)
    host = np.ascontiguousarray(host_rows).view(np.int32).reshape(host_rows.shape[0], -1)
    for i, ln in enumerate(lens):
        want[i * stride * words:(i * stride + ln) * words] = host[i, :ln * words]
    assert got.tobytes() == want.tobytes(), what


def device_call(torch, crossread, bank, host, pairs, opts, keys, **kw):
    """bank_csd_device into fresh sentinel tensors for `keys`; returns (result, {key: tensor}, stride)"""
    rows = host["sxx"].shape[0]
    stride = host["sxx"].shape[1] + 7
    words = dict(PAIR_OUTS)
    t = {k: device_tensor(torch, rows, stride, words[k]) for k in keys}
    got = crossread.bank_csd_device(bank, stride, pairs=pairs, opts=opts, **{DEVICE_ARG.get(k, k): v.data_ptr() for k, v in t.items()}, **kw)
    return got, t, stride


@pytest.mark.parametrize("selection", ["all", "subset with a duplicate"])
def test_device_form(pkg, crossread, state, selection):
    import torch
    pairs = SELECTIONS[selection]
    words = dict(PAIR_OUTS)
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True)):
        host = crossread.bank_csd(state["bank"], pairs, opts, frequencies=True, coherence=True, transfer=True)
        got, t, stride = device_call(torch, crossread, state["bank"], host, pairs, opts, list(words))
        assert got["lens"] == host["lens"] and got["breaks"] == host["breaks"] and got["launches"] == 1
        for k in words:
            check_device_rows(t[k], host[k], host["lens"], stride, words[k], k)
        for k in words:  # each output alone
            got, t, stride = device_call(torch, crossread, state["bank"], host, pairs, opts, [k])
            assert got["launches"] == 1
            check_device_rows(t[k], host[k], host["lens"], stride, words[k], k + " alone")


def test_done_event_form(pkg, crossread, state):
    """the call that returns early, waited for through its event; two of them back to back with different options, each into its
    own tensors (the two job-table slots), and a third and fourth behind them (a slot is reused)"""
    import torch
    opts = [pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True), pkg.MergeOpts(min_count=2),
            pkg.MergeOpts(keep_transition_band=True)]
    host = [crossread.bank_csd(state["bank"], None, o, coherence=True) for o in opts]
    events = []
    for _ in opts:
        ev = torch.cuda.Event()
        ev.record()  # (the handle exists once the event has been recorded)
        events.append(ev)
    torch.cuda.synchronize()
    got, t, stride = device_call(torch, crossread, state["bank"], host[0], None, opts[0], ["sxy", "coherence"], done_event=events[0].cuda_event)
    events[0].synchronize()
    check_device_rows(t["sxy"], host[0]["sxy"], host[0]["lens"], stride, 2, "one call")
    assert got["lens"] == host[0]["lens"] and got["launches"] == 1
    calls = [device_call(torch, crossread, state["bank"], h, None, o, ["sxy", "coherence"], done_event=ev.cuda_event)
             for h, o, ev in zip(host, opts, events)]  # back to back, no wait in between
    for k, ((_, t, stride), h, ev) in enumerate(zip(calls, host, events)):
        ev.synchronize()
        check_device_rows(t["sxy"], h["sxy"], h["lens"], stride, 2, f"sxy of call {k} of four back to back")
        check_device_rows(t["coherence"], h["coherence"], h["lens"], stride, 2, f"coherence of call {k} of four back to back")
    unfed = crossread.bank_csd_device(state["bank"], 4, sxx=calls[0][1]["sxy"].data_ptr(), pairs=[EMPTY], done_event=events[0].cuda_event)
    events[0].synchronize()  # (recorded even though nothing was launched)
    assert unfed["launches"] == 0


def placed(pkg, bank, p, breaks):
    """the raw f32 accumulators of stage_spectra(p, stage) laid along the stitched row by the Breaks: (xx, yy, xy) in f64 / c128"""
    parts = []
    for i, b in enumerate(breaks):
        if b.include:
            _, xx, yy, xy = bank.stage_spectra(p, len(breaks) - 1 - i)
            parts.append([v[b.bins.start:b.bins.stop] for v in (xx, yy, xy)])
    if not parts:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.complex128)
    xx, yy, xy = (np.concatenate([part[k] for part in parts]) for k in range(3))
    return xx.astype(np.float64), yy.astype(np.float64), xy.astype(np.complex128)


def test_coherence_and_h1(pkg, crossread, state):
    """against numpy f64 on the raw f32 accumulators of stage_spectra, placed by the Breaks.  The device works from the f64
    accumulators, the restatement from their f32 casts: each differs by at most 2^-24 relative and nothing cancels, so coherence
    (four factors and the f64 roundings) is within 5 * 2^-24 relative and each H1 component (two) within 3 * 2^-24.  NaN exactly
    where the restatement has it.  Against the public coherence() of the stitched f32 rows (two roundings a factor, not all at
    their worst at once): 6 * 2^-24."""
    bank = state["bank"]
    nan_rows = 0
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True)):
        got = crossread.bank_csd(bank, None, opts, coherence=True, transfer=True)
        assert got["coherence"].dtype == np.float64 and got["transfer"].dtype == np.complex128
        worst = np.zeros(3)
        for p in range(6):
            ln = got["lens"][p]
            xx, yy, xy = placed(pkg, bank, p, got["breaks"][p])
            assert len(xx) == ln
            den = xx * yy
            with np.errstate(divide="ignore", invalid="ignore"):
                coh = np.where(den != 0, (xy.real * xy.real + xy.imag * xy.imag) / den, np.nan)
                tr_re, tr_im = np.where(xx != 0, xy.real / xx, np.nan), np.where(xx != 0, xy.imag / xx, np.nan)
            c, t = got["coherence"][p, :ln], got["transfer"][p, :ln]
            assert np.all(np.isnan(got["coherence"][p, ln:])) and np.all(np.isnan(got["transfer"][p, ln:]))
            assert np.array_equal(np.isnan(c), np.isnan(coh)) and np.array_equal(np.isnan(t.real), np.isnan(tr_re)), p
            assert np.array_equal(np.isnan(t.imag), np.isnan(tr_im)), p
            ok = ~np.isnan(coh)
            pub = pkg.coherence(*bank.csd(p, opts)[:3])
            assert np.array_equal(np.isnan(pub), np.isnan(c)), p
            errs = [np.abs(c[ok] - coh[ok]) / coh[ok], np.abs(t.real[ok] - tr_re[ok]) / np.maximum(np.abs(tr_re[ok]), 1e-300),
                    np.abs(c[ok] - pub[ok]) / coh[ok]]
            if ok.any():
                worst = np.maximum(worst, [e.max() / U for e in errs])
            assert np.all(np.abs(c[ok] - coh[ok]) <= 5 * U * coh[ok]), (p, opts)
            assert np.all(np.abs(t.real[ok] - tr_re[ok]) <= 3 * U * np.abs(tr_re[ok])), (p, opts)
            assert np.all(np.abs(t.imag[ok] - tr_im[ok]) <= 3 * U * np.abs(tr_im[ok])), (p, opts)
            assert np.all(np.abs(c[ok] - pub[ok]) <= 6 * U * coh[ok]), (p, opts)
            nan_rows += int(ln > 0 and not ok.any())
        print(state["name"], opts.keep_overlap, "worst errors in 2^-24: coherence", worst[0], "H1 re", worst[1], "against coherence()", worst[2])
    assert nan_rows == 2  # the all-zero pair, under both option sets


def test_known_answer(pkg, crossread, state):
    """the pair fed y = 2 x: coherence 1 and H1 = 2 + 0j at every included bin, within 1e-6 (16 * 2^-24 bounds the f32 rounding of
    the segment kernels' own products); and syy = 4 sxx, sxy = 2 sxx: a swapped sxx / syy or a lost conjugate shows"""
    got = crossread.bank_csd(state["bank"], [DOUBLE, LONG], pkg.MergeOpts(), coherence=True, transfer=True, bands=[(0.0, 0.5), (0.01, 0.1)])
    ln = got["lens"][0]
    assert ln > 0
    assert np.all(np.abs(got["coherence"][0, :ln] - 1.0) <= 1e-6), np.abs(got["coherence"][0, :ln] - 1.0).max()
    assert np.all(np.abs(got["transfer"][0, :ln] - 2.0) <= 1e-6), np.abs(got["transfer"][0, :ln] - 2.0).max()
    assert np.allclose(got["syy"][0, :ln], 4.0 * got["sxx"][0, :ln], rtol=1e-5, atol=0)
    assert np.all(np.abs(crossread.band_coherence(got["band_sums"][0]) - 1.0) <= 1e-6)
    assert np.all(np.abs(crossread.band_transfer(got["band_sums"][0]) - 2.0) <= 1e-6)
    # the other pair (y = 0.6 x + 0.8 noise): partial coherence, H1 near 0.6 over the whole range (loose: few averages under set_avg)
    coh = got["coherence"][1, :got["lens"][1]]
    assert np.all((coh >= 0) & (coh <= 1 + 1e-6)) and 0.05 < np.median(coh) < 0.95
    assert abs(crossread.band_transfer(got["band_sums"][1])[0] - 0.6) < 0.3 and 0.05 < crossread.band_coherence(got["band_sums"][1])[0] < 0.95


def bands_of():
    """the whole range; most of stage 0; a decade across a seam; a single bin (k = n/4 of stage 0); none"""
    return [(0.0, 0.5), (0.0501, 0.5), (0.01, 0.1), (0.25, 0.25), (0.30001, 0.30002)]


def test_band_sums(pkg, crossread, state, tmp_path_factory):
    """Within the summation bound of numpy's trapezoids on the stitched rows; the same bits from a second call, from bands alone
    (one launch) and from the device form; and the bits of cross_band_pair_host (csrc/cross_readout.h run on the CPU by
    tests/host/cross_readout_check.cpp) on the pair's own stage_spectra rows and Breaks: every product rounded before it is added,
    thread t over the elements t, t + 256, ..., the shuffle tree, the wavefronts in order"""
    import torch
    from test_bank_readout_host import band_reference
    from test_waterfall_host import host_exe
    bank, bands, n = state["bank"], bands_of(), state["n"]
    wt = getattr(pkg.WindowTable, state["window"].lower())(n)
    d = tmp_path_factory.mktemp("cross_band_bits")
    exe = host_exe(d, "cross_readout_check", False)
    nonzero = 0
    # (min_count stays 1: a stage without a segment has the gain 0 and stitches to NaN, in csd() too)
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, keep_transition_band=True)):
        got = crossread.bank_csd(bank, None, opts, frequencies=True, bands=bands)
        assert got["launches"] == 2 and got["band_sums"].shape == (6, len(bands), 4) and got["band_sums"].dtype == np.float64
        blob = [struct.pack("<I", 6)]
        for p in range(6):
            ln = got["lens"][p]
            rows = [got["sxx"][p, :ln], got["syy"][p, :ln], got["sxy"][p, :ln].real, got["sxy"][p, :ln].imag]
            freq = got["frequencies"][p, :ln]
            for r, row in enumerate(rows):
                for b, (want, tol, count) in enumerate(band_reference(np.ascontiguousarray(row), freq, bands)):
                    assert abs(got["band_sums"][p, b, r] - want) <= tol, (p, b, r, got["band_sums"][p, b, r], want, tol)
                    if count == 0:
                        assert got["band_sums"][p, b, r] == 0.0
            breaks = got["breaks"][p]
            stages = [bank.stage_spectra(p, s) for s in range(len(breaks))]
            assert [b.count for b in breaks[::-1]] == [st[0]["count"] for st in stages]
            acc = np.array([[xx, yy, xy.real, xy.imag] for _, xx, yy, xy in stages], np.float64).reshape(len(stages), 4, n // 2 + 1)
            blob.append(struct.pack("<5I2f", n, len(stages), len(breaks), len(bands), 4, wt.nenbw, wt.power))
            blob.append(np.asarray([st[0]["count"] for st in stages], np.uint64).tobytes())
            blob += [bytes(b._c()) for b in breaks]
            blob.append(acc.tobytes())
            blob.append(np.asarray(bands, np.float32).tobytes())
        assert np.all(got["band_sums"][EMPTY] == 0.0) and np.all(got["band_sums"][ZEROS] == 0.0)
        src, dst = str(d / "cases.bin"), str(d / "rows.bin")
        with open(src, "wb") as f:
            f.write(b"".join(blob))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
        raw, pos = open(dst, "rb").read(), 0
        for p in range(6):
            ln = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            assert ln == got["lens"][p]
            rows = np.frombuffer(raw, np.float32, 4 * ln, pos + 8).reshape(4, ln)
            assert rows[0].tobytes() == got["sxx"][p, :ln].tobytes() and rows[1].tobytes() == got["syy"][p, :ln].tobytes()
            assert rows[2].tobytes() == got["sxy"][p, :ln].real.tobytes() and rows[3].tobytes() == got["sxy"][p, :ln].imag.tobytes()
            assert raw[pos + 8 + 16 * ln:pos + 8 + 20 * ln] == got["frequencies"][p, :ln].tobytes()
            host = np.frombuffer(raw, np.float64, 4 * len(bands), pos + 8 + 44 * ln).reshape(len(bands), 4)
            print(state["name"], opts.keep_overlap, "pair", p, "device", got["band_sums"][p, 0], "host", host[0])
            assert host.tobytes() == got["band_sums"][p].tobytes(), (p, host, got["band_sums"][p])
            nonzero += int(np.count_nonzero(host))
            pos += 8 + 44 * ln + 32 * len(bands)
        assert pos == len(raw)
        # the same bits from a second call, from bands alone, and from the device form with the rows
        again = crossread.bank_csd(bank, None, opts, bands=bands)
        assert again["band_sums"].tobytes() == got["band_sums"].tobytes()
        count = 6 * len(bands) * 4
        tb = torch.full((count + 3,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev = crossread.bank_csd_device(bank, 0, opts=opts, bands=bands, band_ptr=tb.data_ptr())
        assert dev["launches"] == 1
        out = tb.cpu().numpy()
        assert out[:count].tobytes() == got["band_sums"].tobytes() and np.all(out[count:] == -1.0)
        tb.fill_(-1.0)
        dev, t, stride = device_call(torch, crossread, bank, got, None, opts, ["sxx"], bands=bands, band_ptr=tb.data_ptr())
        assert dev["launches"] == 2 and tb.cpu().numpy()[:count].tobytes() == got["band_sums"].tobytes()
        check_device_rows(t["sxx"], got["sxx"], got["lens"], stride, 1, "sxx with bands")
    assert nonzero >= 2 * 3 * 4 * 3  # at least three fed pairs, four bands that hold bins, three rows that are not zero
    # the unfed pair alone: nothing is launched, the band sums are 0.0
    tb = torch.full((len(bands) * 4,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = crossread.bank_csd_device(bank, 0, pairs=[EMPTY], bands=bands, band_ptr=tb.data_ptr())
    assert dev["launches"] == 0 and np.all(tb.cpu().numpy() == 0.0)
    alone = crossread.bank_csd(bank, [EMPTY], bands=bands)
    assert alone["launches"] == 0 and alone["sxx"].shape == (1, 0) and np.all(alone["band_sums"] == 0.0)


@pytest.mark.parametrize("m", [3, 4])
def test_matrix(pkg, crossread, gpu_required, m):
    """CsmCascadeBank(64, m) with three groups, one of them unfed: bank_rows equals csd(g) row for row, byte for byte, with the
    Breaks and frequencies; the device form writes exactly lens[g] bins a row"""
    import torch
    bank = pkg.CsmCascadeBank(64, m, 3)
    for g, length in ((0, 1 << 13), (2, 777)):
        xs = [pkg.noise_host(length, seed=100 * g + c) for c in range(m)]
        xs[1] = (xs[1] + 0.5 * xs[0]).astype(np.float32)
        for lo in range(0, length, 3000):
            bank.process(g, [x[lo:lo + 3000] for x in xs])
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True), pkg.MergeOpts(min_count=10 ** 6)):
        for groups in (None, [2, 1, 0, 2]):
            got = crossread.bank_rows(bank, groups, opts, frequencies=True)
            sel = range(3) if groups is None else groups
            ref = [bank._merged(bank._L.psdc_csm_csd, g, opts, m * m) for g in sel]  # (the raw rows csd(g) makes its matrix of)
            assert got["rows"].dtype == np.float32 and got["rows"].shape == (len(sel), m * m, max(r.shape[1] for r, _ in ref))
            for i, (g, (rows, br)) in enumerate(zip(sel, ref)):
                ln = rows.shape[1]
                assert got["lens"][i] == ln and got["breaks"][i] == br and (ln > 0) == (g != 1 and opts.min_count < 10 ** 6)
                assert got["rows"][i, :, :ln].tobytes() == np.ascontiguousarray(rows).tobytes(), (g, opts)
                assert np.all(np.isnan(got["rows"][i, :, ln:])) and np.all(np.isnan(got["frequencies"][i, ln:]))
                assert got["frequencies"][i, :ln].tobytes() == pkg.Break.frequencies(br).tobytes()
                S, br2 = bank.csd(g, opts)
                assert pkg.csm_matrix(got["rows"][i, :, :ln], m).tobytes() == S.tobytes() and br2 == br
            assert got["launches"] == (1 if got["rows"].shape[2] else 0)
            lay = crossread.layout(bank, groups, opts)
            assert lay["lens"] == got["lens"] and lay["breaks"] == got["breaks"] and lay["max_len"] == got["rows"].shape[2]
            stride = got["rows"].shape[2] + 5
            tr, tf = device_tensor(torch, len(sel) * m * m, stride), device_tensor(torch, len(sel), stride)
            dev = crossread.bank_rows_device(bank, stride, tr.data_ptr(), tf.data_ptr(), groups, opts)
            assert dev["lens"] == got["lens"] and dev["launches"] == got["launches"]
            check_device_rows(tr, got["rows"].reshape(len(sel) * m * m, -1), np.repeat(got["lens"], m * m), stride, 1, "rows")
            check_device_rows(tf, got["frequencies"], got["lens"], stride, 1, "frequencies")
    with pytest.raises(pkg.PsdError) as e:
        crossread.bank_csd(bank)
    assert e.value.code == pkg.ERR_ARG
    one = pkg.CsmCascade(64, m)
    one.process([pkg.noise_host(2000, seed=c) for c in range(m)])
    assert pkg.csm_matrix(crossread.bank_rows(one)["rows"][0], m).tobytes() == one.csd()[0].tobytes()
    one.close()
    crossread.release(bank)
    bank.close()


def test_seventy_pairs_in_one_launch(pkg, crossread, gpu_required):
    """a bank of 70 pairs of which 3 are fed, all 70 selected: one launch (jobs run along x), two with bands"""
    bank = pkg.CsdCascadeBank(64, 70)
    fed = (3, 40, 69)
    for p in fed:
        x = pkg.noise_host(3000 + p, seed=p)
        bank.process(p, x, x[::-1].copy())
    got = crossread.bank_csd(bank, frequencies=True, coherence=True, bands=[(0.0, 0.5), (0.01, 0.1)])
    assert got["launches"] == 2 and crossread.bank_csd(bank)["launches"] == 1
    for p in range(70):
        xx, yy, xy, br = bank.csd(p)
        assert got["lens"][p] == len(xx) and got["breaks"][p] == br
        assert got["sxx"][p, :len(xx)].tobytes() == xx.tobytes() and got["sxy"][p, :len(xx)].tobytes() == xy.tobytes()
        assert (len(xx) > 0) == (p in fed)
        if p not in fed:
            assert np.all(got["band_sums"][p] == 0.0)
    sel = list(range(69, -1, -1)) * 2
    twice = crossread.bank_csd(bank, sel)
    assert twice["launches"] == 1 and twice["sxx"].shape[0] == 140
    assert twice["syy"][0].tobytes() == got["syy"][69].tobytes() and twice["syy"][70 + 29].tobytes() == got["syy"][40].tobytes()
    crossread.release(bank)  # the buffers come back with the next call
    assert crossread.bank_csd(bank)["sxy"].tobytes() == got["sxy"].tobytes()
    single = pkg.CsdCascade(64)
    x = pkg.noise_host(3003, seed=3)
    single.process(x, x[::-1].copy())
    one = crossread.bank_csd(single)
    assert one["sxy"][0].tobytes() == got["sxy"][3, :one["lens"][0]].tobytes() == single.csd()[2].tobytes()
    single.close()
    bank.close()


def test_errors(pkg, crossread, state):
    import torch
    bank = state["bank"]
    L = crossread._lib()
    lay = crossread.layout(bank)
    stride = lay["max_len"] - 1
    t = device_tensor(torch, 6, lay["max_len"], 4)
    c = crossread._Call(bank, None, None, ("cross",))
    rc = L.psdcxr_cross_csd_device(*c.head, None, None, None, None, None, C.c_void_p(t.data_ptr()), stride, None, 0, None, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and "stride" in pkg.lib().psdc_cross_last_error(bank._h).decode()
    assert c.result()["lens"] == lay["lens"] and int(c.info.max_len) == lay["max_len"] and int(c.info.launches) == 0
    assert np.all(t.cpu().numpy() == SENTINEL)
    host = np.zeros((6, lay["max_len"]), np.float32)
    c = crossread._Call(bank, None, None, ("cross",))
    rc = L.psdcxr_cross_csd(*c.head, host.ctypes.data, None, None, None, None, None, stride, None, 0, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and c.result()["lens"] == lay["lens"] and np.all(host == 0)
    c = crossread._Call(bank, None, None, ("cross",))  # room for fewer breaks than pair 0 has
    rc = L.psdcxr_cross_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, 2, C.byref(c.info))
    assert rc == pkg.ERR_CAPACITY and [int(v) for v in c.lens] == lay["lens"] and int(c.nb[0]) == len(lay["breaks"][0])

    def arg_error(text, fn, *args, **kw):
        with pytest.raises(pkg.PsdError) as e:
            fn(bank, *args, **kw)
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))

    ptr, width = t.data_ptr(), lay["max_len"]
    arg_error("out of range", crossread.bank_csd, [0, 6])
    arg_error("out of range", crossread.layout, [6])
    arg_error("out of range", crossread.bank_csd_device, width, sxx=ptr, pairs=[7])
    arg_error("more than 8 bands", crossread.bank_csd_device, width, sxx=ptr, bands=[(0.0, 0.1)] * 9, band_ptr=ptr)
    arg_error("bands without a band output", crossread.bank_csd_device, width, sxx=ptr, bands=[(0.0, 0.1)])
    arg_error("a band output without bands", crossread.bank_csd_device, width, sxx=ptr, band_ptr=ptr)
    arg_error("a band with NaN or lo > hi", crossread.bank_csd, bands=[(0.0, 0.1), (float("nan"), 0.2)])
    arg_error("a band with NaN or lo > hi", crossread.bank_csd, bands=[(0.2, 0.1)])
    arg_error("no output", crossread.bank_csd_device, width)
    arg_error("takes a CsmCascadeBank", crossread.bank_rows)
    c = crossread._Call(bank, None, None, ("cross",))
    rc = L.psdcxr_cross_layout(*c.head, None, c.nb.ctypes.data, None, 0, None)
    assert rc == pkg.ERR_ARG and pkg.lib().psdc_cross_last_error(bank._h).decode() == "psdcxr_cross_layout: null lens"
    c = crossread._Call(bank, None, None, ("cross",))
    rc = L.psdcxr_cross_layout(*c.head, c.lens.ctypes.data, None, c.br.ctypes.data, 16, None)
    assert rc == pkg.ERR_ARG and pkg.lib().psdc_cross_last_error(bank._h).decode() == "psdcxr_cross_layout: breaks without n_breaks"
    assert np.all(t.cpu().numpy() == SENTINEL)
    other = pkg.PsdCascadeBank(64, 2)  # another object's handle never reaches the C call
    with pytest.raises(pkg.PsdError) as e:
        crossread.bank_csd(other)
    assert e.value.code == pkg.ERR_ARG and "CsdCascadeBank" in str(e.value)
    other.close()
    before = crossread.bank_csd(bank, coherence=True)
    crossread.release(bank)
    crossread.release(bank)
    after = crossread.bank_csd(bank, coherence=True)  # the buffers are made again
    assert after["sxy"].tobytes() == before["sxy"].tobytes() and after["coherence"].tobytes() == before["coherence"].tobytes()


def test_cli_flag_gives_the_same_files(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --pair ... --bank-readout reads every pair of a frames file with one bank_csd call: the same lines, the
    same files"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batches, frames = 8, 700
    words = np.random.default_rng(5).integers(-20000, 20000, (4, 8 * batches * frames)).astype(np.int16)
    words[1] = words[0] // 2 + words[1] // 2
    data, fs = pkg.make_adcdac_frames(words, batches, seq0=1)
    path = tmp_path / "frames.bin"
    path.write_bytes(data)
    outs = []
    for extra in ([], ["--bank-readout"]):
        d = tmp_path / ("csv" + str(len(extra)))
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--file", str(path), "--frame-size", str(fs),
                            "--pair", "0:1", "--pair", "2:3", "--csv", str(d)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append((r.stdout, d))
    assert outs[0][0] == outs[1][0] and "no samples" not in outs[0][0], (outs[0][0], outs[1][0])
    names = sorted(os.listdir(outs[0][1]))
    assert len(names) >= 2 and names == sorted(os.listdir(outs[1][1]))
    for name in names:
        assert filecmp.cmp(outs[0][1] / name, outs[1][1] / name, shallow=False), name
