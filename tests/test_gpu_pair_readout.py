"""Bank read-out of the pair carrier objects on the MI355X (include/ext/psdcascade_pairread.h, psdcpr_*;
stabilizer-stream_amd/pairread.py): one call stitches every selected pair of a zoom cross, IQ cross or zoom / IQ AM/PM cross bank on
the device.  For the 8-row banks the six f32 outputs, the frequencies, lengths and Breaks must equal what csd(p) and
Break.frequencies return, byte for byte and field for field; for the 12-row banks (whose csd(p) rounds once, from f64) they equal
tests/pair_read_ref.py on the pair's own stage_rows, and cab / cba equal sidebands(p) byte for byte.  Coherence and H1 are held to
numpy's coherence() / transfer() on the f32 rows of csd(p) within derived bounds, the AM/PM cross rows and carrier records to
am_pm_cross(p) / carriers(p) within a bound of a few f64 roundings and to the restatement byte for byte; the band sums carry the
bits of the host restatement.

Shapes: n = 64 (33 bins: one tile; the zoom and the IQ class, 8 and 12 rows) and n = 1024 (513 bins: the third tile of a job holds
ONE element) with the Hann window, n = 256 with the rectangular window; one n = 64 bank under set_avg with a small limit and one
under Mean detrend.  A bank has six pairs fed in several calls: LONG (three or more live stages; both sides carry a shared AM tone at
offset 1/8 and a shared PM tone at offset 3/16 plus independent noise), ODD (an odd length, side b detuned by 1 / (8 n 64): lock_w
visibly below 1), SHORT (one stage), EMPTY (never fed), ZEROS (all zeros: the NaN paths) and TWIN (LONG again, its last half call fed
right before the first read-out).  `twin` is a second bank fed the same calls that never sees a bank read-out."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pair_read_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AC3C3  # the bit pattern the device outputs are pre-filled with
# name: (n, window, samples of LONG and TWIN, of ODD and ZEROS, of SHORT, set_avg, detrend)
SHAPES = {
    "n64": (64, "HANN", 1 << 14, 5001, 100, None, None),
    "n1024": (1024, "HANN", 1 << 18, 5000 * 16 + 1, 1600, None, None),
    "n256rect": (256, "RECTANGULAR", 1 << 16, 5000 * 4 + 1, 400, None, None),
    "n64avg": (64, "HANN", 1 << 14, 5001, 100, (7, 900), None),
    "n64mean": (64, "HANN", 1 << 14, 5001, 100, None, "MEAN"),
}
STATES = [(s, "zoom", k) for s in SHAPES for k in ("csd", "xampm")] + [("n64", "iq", k) for k in ("csd", "xampm")]
CLASSES = {("zoom", "csd"): "ZoomCsdCascadeBank", ("iq", "csd"): "IqCsdCascadeBank", ("zoom", "xampm"): "ZoomAmPmCsdCascadeBank",
           ("iq", "xampm"): "IqAmPmCsdCascadeBank"}
LONG, ODD, SHORT, EMPTY, ZEROS, TWIN = range(6)
SELECTIONS = {"all": None, "permutation": [4, 2, 0, 5, 3, 1], "subset with a duplicate": [1, 5, 1], "the unfed pair alone": [EMPTY]}
F32_KEYS = ("saa_up", "saa_lo", "sbb_up", "sbb_lo", "sab_up", "sab_lo")
# host key: (device argument, 32-bit words a bin)
CSD_OUTS = {"saa_up": ("saa_up", 1), "saa_lo": ("saa_lo", 1), "sbb_up": ("sbb_up", 1), "sbb_lo": ("sbb_lo", 1), "sab_up": ("sab_up", 2),
            "sab_lo": ("sab_lo", 2), "frequencies": ("freq", 1), "coherence_up": ("coh_up", 2), "coherence_lo": ("coh_lo", 2),
            "transfer_up": ("h1_up", 4), "transfer_lo": ("h1_lo", 4)}
AMPM_KEYS = ("s_am", "s_pm", "s_am_pm", "s_pm_am")
AMPM_OUTS = {"frequencies": ("freq", 1), "cab": ("cab", 4), "cba": ("cba", 4), **{k: (k, 4) for k in AMPM_KEYS}}
F0, F_AM, F_PM, A_AM, A_PM, AMP, THETA = 0.25, 1.0 / 8, 3.0 / 16, 0.01, 0.02, 0.5, 0.3
EPS, EPS32 = 2.0 ** -53, 2.0 ** -24
# (p_ab, w, q) of a given-carriers call, a pair each: w and q of any magnitude
GIVEN = [(0.25, np.exp(0.2j), np.exp(0.8j)), (0.3, 2.0 - 1.0j, 0.5j), (0.25, 1.0 + 0j, 1.0 + 0j), (1.0, 0.7j, -0.2 + 0j),
         (0.5, 0.3 + 0.3j, 1.0 - 1.0j), (0.25, np.exp(0.2j), np.exp(0.8j))]
ALL_CSD = dict(frequencies=True, coherence=True, transfer=True)


def all_opts(pkg):
    """the eight merge-option combinations of the sibling tests, and a min_count that excludes everything"""
    return [pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)
            for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 2))] + [pkg.MergeOpts(min_count=10 ** 6)]


def two_opts(pkg):
    return (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True))


@pytest.fixture(scope="module")
def pairread(pkg):
    from stabilizer_stream_amd import pairread as mod
    return mod


def side(pkg, iq, length, seed, detune=0.0, theta=THETA):
    """one side of a pair: a carrier of amplitude 2 AMP (real) / AMP (complex) with the shared a = A_AM cos(2 pi F_AM j) and
    phi = A_PM sin(2 pi F_PM (j - 3)) and white noise of 1e-3 of its own: real at F0 + detune for the zoom classes, complex at
    detune for the IQ classes"""
    j = np.arange(length, dtype=np.float64)
    a = A_AM * np.cos(2 * np.pi * F_AM * j)
    phi = A_PM * np.sin(2 * np.pi * F_PM * (j - 3))
    noise = 1e-3 * pkg.noise_host(length, seed=seed).astype(np.float64)
    if iq:
        z = AMP * (1 + a) * np.exp(1j * (2 * np.pi * detune * j + theta + phi))
        return (z + noise + 1j * 1e-3 * pkg.noise_host(length, seed=seed + 7)).astype(np.complex64)
    return (2 * AMP * (1 + a) * np.cos(2 * np.pi * (F0 + detune) * j + theta + phi) + noise).astype(np.float32)


def feed(pkg, bank, n, iq, long, mid, short, last_half):
    """the calls of a bank; last_half: called right before the TWIN pair's last half call"""
    if not iq:
        for p in range(6):
            bank.set_carrier(p, f0=F0)
    x, y = side(pkg, iq, long, 1000 + n), side(pkg, iq, long, 1500 + n, theta=THETA + 0.5)
    piece = long // 4
    for k in range(4):
        bank.process(LONG, x[k * piece:(k + 1) * piece], y[k * piece:(k + 1) * piece])
    xo, yo = side(pkg, iq, mid, 2000 + n), side(pkg, iq, mid, 2500 + n, detune=1.0 / (8 * n * 64), theta=THETA - 0.2)
    for pa, pb in zip(np.array_split(xo, 3), np.array_split(yo, 3)):
        bank.process(ODD, pa, pb)
    bank.process(SHORT, side(pkg, iq, short, 3000 + n), side(pkg, iq, short, 3500 + n, theta=1.0))
    for part in np.array_split(np.zeros(mid, x.dtype), 2):
        bank.process(ZEROS, part, part)
    for k in range(3):
        bank.process(TWIN, x[k * piece:(k + 1) * piece], y[k * piece:(k + 1) * piece])
    half = 3 * piece + piece // 2
    bank.process(TWIN, x[3 * piece:half], y[3 * piece:half])
    last_half()
    bank.process(TWIN, x[half:], y[half:])


_MADE = {}  # the states made so far, by their parameters: the fixtures below share them


@pytest.fixture(scope="module", autouse=True)
def close_states():
    yield
    for st in _MADE.values():
        st["twin"].close()
        st["bank"].close()
    _MADE.clear()


def own_reads(bank, kind, detrend, p, opts):
    """what the object's own per-pair read-outs return, as (bytes of every row, breaks): csd(p); for the 12-row kinds sidebands(p),
    am_pm_cross(p, carriers) and, where the pair has carriers in bin 0, am_pm_cross(p) with carriers=None"""
    calls = [bank.csd(p, opts)]
    if kind == "xampm":
        calls += [bank.sidebands(p, opts), bank.am_pm_cross(p, GIVEN[p], opts)]
        if not detrend and p not in (EMPTY, ZEROS):
            calls.append(bank.am_pm_cross(p, None, opts))
    return [([np.asarray(v).tobytes() for v in r[:-1]], r[-1]) for r in calls]


def stage_acc(bank, p):
    """the pair's own f64 stage_rows [ns][12][bins], and the stage counts (12-row kinds)"""
    stages = [bank.stage_rows(p, s) for s in range(bank.num_stages(p))]
    return np.array([r for _, r in stages], np.float64).reshape(len(stages), 12, bank.n // 2 + 1), [st[0]["count"] for st in stages]


def make_state(pkg, pairread, param):
    """one fed bank a (shape, family, kind): dict(bank, twin, first, ref, ...).  `first` is the bank read-out made right behind the
    TWIN pair's last half call; ref[opts] = [(six rows, breaks, frequencies)] of every pair from csd(p), computed once, as are the
    12-row kinds' stage rows and the pairs' other read-outs"""
    if param in _MADE:
        return _MADE[param]
    shape, family, kind = param
    n, window, long, mid, short, avg, detrend = SHAPES[shape]
    iq = family == "iq"
    banks = []
    for _ in range(2):
        bank = getattr(pkg, CLASSES[family, kind])(n, 6, getattr(pkg.Window, window))
        if avg:
            bank.set_avg(pkg.AvgOpts(*avg))
        if detrend:
            bank.set_detrend(getattr(pkg.Detrend, detrend))
        feed(pkg, bank, n, iq, long, mid, short, bank.sync)
        banks.append(bank)
    bank, twin = banks
    first = pairread.bank_csd(bank, **ALL_CSD)
    refs = {}
    for opts in all_opts(pkg) + [pkg.MergeOpts()]:
        refs[opts] = [(r[:6], r[6], pkg.Break.frequencies(r[6])) for r in (bank.csd(p, opts) for p in range(6))]
    # (taken behind `first`, as the csd(p) references are, so that `first` still finds the half call undrained; every other bank
    # read-out of this file comes after them)
    own = {opts: [own_reads(bank, kind, detrend, p, opts) for p in range(6)] for opts in two_opts(pkg)}
    acc = [stage_acc(bank, p) for p in range(6)] if kind == "xampm" else None
    wt = getattr(pkg.WindowTable, window.lower())(n)
    _MADE[param] = dict(bank=bank, twin=twin, first=first, ref=refs, own=own, acc=acc, n=n, name="-".join(param), kind=kind, detrend=detrend,
                        wt=wt)
    return _MADE[param]


@pytest.fixture(scope="module", params=STATES, ids=["-".join(s) for s in STATES])
def state(request, pkg, pairread, gpu_required):
    return make_state(pkg, pairread, request.param)


AMPM_STATES = [s for s in STATES if s[2] == "xampm"]


@pytest.fixture(scope="module", params=AMPM_STATES, ids=["-".join(s) for s in AMPM_STATES])
def ampm_state(request, pkg, pairread, gpu_required):
    """the 12-row objects among the states"""
    return make_state(pkg, pairread, request.param)


OWN_CARRIER_STATES = [s for s in AMPM_STATES if not SHAPES[s[0]][6]]


@pytest.fixture(scope="module", params=OWN_CARRIER_STATES, ids=["-".join(s) for s in OWN_CARRIER_STATES])
def own_carrier_state(request, pkg, pairread, gpu_required):
    """... that read their own carriers (no detrend)"""
    return make_state(pkg, pairread, request.param)


def same(a, b):
    """byte for byte, where NaN equals NaN (the sign and payload of a NaN are not part of the result)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())


def restated(state, p, breaks):
    """(rows [12][L], g [L]) of a 12-row pair's own stage rows laid along its Breaks"""
    acc, counts = state["acc"][p]
    return ref.placed(acc, breaks, state["n"], counts, state["wt"].nenbw, state["wt"].power)[:2]


def pairs_of(channels):
    return range(6) if channels is None else channels


def check_csd(pkg, state, got, opts, channels, what):
    """a bank_csd() result against csd(p) of each selected pair (8 rows: byte for byte; 12 rows: lens, Breaks and frequencies byte
    for byte, the f32 rows against the restatement on stage_rows), coherence and H1 against numpy on the f32 rows of csd(p) within
    9 * 2^-24 and 5 * 2^-24 a component -- each f32 value carries two roundings (the cast and the scale), four values enter the
    coherence and two a component of H1; one 2^-24 is left for the second-order terms -- with NaN in the same places, and for the
    12-row kinds byte for byte against the restatement.  Returns the largest deviations in 2^-24."""
    refs = state["ref"][opts]
    sel = pairs_of(channels)
    width = max([len(refs[p][2]) for p in sel] or [0])
    worst = np.zeros(2)
    for key in F32_KEYS + ("frequencies", "coherence_up", "coherence_lo", "transfer_up", "transfer_lo"):
        want = np.complex64 if key.startswith("sab") else np.complex128 if key.startswith("tr") else np.float64 if key.startswith("co") else np.float32
        assert got[key].dtype == want and got[key].shape == (len(sel), width), (what, key)
    for i, p in enumerate(sel):
        rows6, br, f = refs[p]
        ln = len(f)
        assert got["lens"][i] == ln and got["breaks"][i] == br, (what, i)  # field for field (a frozen dataclass)
        assert got["frequencies"][i, :ln].tobytes() == f.tobytes(), (what, i)
        for key in got:
            if isinstance(got[key], np.ndarray) and key != "band_sums":
                assert np.all(np.isnan(got[key][i, ln:])), (what, i, key)
        if state["kind"] == "csd":
            for key, want in zip(F32_KEYS, rows6):
                assert got[key][i, :ln].tobytes() == want.tobytes(), (what, i, key)
        elif ln:
            rows, g = restated(state, p, br)
            want = ref.csd_sides(rows, g)
            for key in F32_KEYS:
                w = want[key] if want[key].ndim == 1 else want[key].view(np.complex64)[:, 0]
                assert same(got[key][i, :ln], w), (what, i, key)
            for key, rk in (("coherence_up", "coh_up"), ("coherence_lo", "coh_lo")):
                assert same(got[key][i, :ln], want[rk]), (what, i, key)
            for key, rk in (("transfer_up", "h1_up"), ("transfer_lo", "h1_lo")):
                assert same(got[key][i, :ln], want[rk].view(np.complex128)[:, 0]), (what, i, key)
        if p not in (EMPTY, ZEROS):  # every fed bin's f32 value is not 0 (ZEROS: every one is, and coherence and H1 are NaN)
            assert all(np.all(r != 0) for r in rows6), (what, i)
        for s, (aa, bb, ab) in enumerate(((rows6[0], rows6[2], rows6[4]), (rows6[1], rows6[3], rows6[5]))):
            co, h1 = got[("coherence_up", "coherence_lo")[s]][i, :ln], got[("transfer_up", "transfer_lo")[s]][i, :ln]
            wc, wh = pkg.coherence(aa, bb, ab), pkg.transfer(aa, ab)
            assert np.array_equal(np.isnan(co), np.isnan(wc)) and np.array_equal(np.isnan(h1), np.isnan(wh)), (what, i, s)
            if p == ZEROS:
                assert np.all(np.isnan(co)) and np.all(np.isnan(h1))
            ok = ~np.isnan(co)
            if ok.any():
                dc = np.abs(co - wc)[ok] / wc[ok]
                parts = [(np.abs(g - w)[ok], np.abs(w)[ok]) for g, w in ((h1.real, wh.real), (h1.imag, wh.imag))]
                # (the bound is an inequality, not a quotient: a real stream at F0 = 1/4 has a real transform at offset 1/4 of stage 0,
                # the stream's Nyquist and DC bins, so Im S_ab and Im H1 are exactly 0 there on both sides)
                dh = max(float(np.max(d[w > 0] / w[w > 0])) for d, w in parts)
                worst = np.maximum(worst, [dc.max() / EPS32, dh / EPS32])
                assert np.all(dc <= 9 * EPS32) and all(np.all(d <= 5 * EPS32 * w) for d, w in parts), (what, i, s, worst)
    return worst


def test_shape_is_what_the_cases_need(pkg, state):
    rows = next(iter(state["ref"].values()))
    live = [sum(b.count > 0 for b in r[1]) for r in rows]  # stages that hold a segment
    print(state["name"], "live stages", live, "stage-0 counts", [r[1][-1].count if r[1] else None for r in rows])
    assert live[LONG] >= 3 and live[TWIN] == live[LONG] and live[ODD] >= 2 and live[SHORT] == 1 and live[EMPTY] == 0 and not rows[EMPTY][1], live
    assert live[ZEROS] >= 2
    if state["n"] == 1024:  # a job of 513 bins: three tiles, the last of one element
        assert any(len(b.bins) == 513 for b in state["bank"].csd(LONG, pkg.MergeOpts(keep_transition_band=True))[6])


def test_first_read_out_behind_a_half_call(pkg, state):
    check_csd(pkg, state, state["first"], pkg.MergeOpts(), None, "first read-out")
    assert state["first"]["launches"] == 1


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_host_form_equals_csd(pkg, pairread, state, selection):
    """the six f32 outputs, lens, breaks, frequencies, coherence and H1 for every merge-option combination; the launch counts of info
    and of stats_read; layout() gives the same lens and Breaks"""
    channels = SELECTIONS[selection]
    bank = state["bank"]
    worst = np.zeros(2)
    for opts in all_opts(pkg):
        before = bank.stats_read()["launches"]
        got = pairread.bank_csd(bank, channels, opts, **ALL_CSD)
        worst = np.maximum(worst, check_csd(pkg, state, got, opts, channels, (state["name"], selection, opts)))
        included = any(b.include for p in pairs_of(channels) for b in state["ref"][opts][p][1])
        assert got["launches"] == (1 if included else 0), (selection, opts)
        assert bank.stats_read()["launches"] - before == got["launches"]
        lay = pairread.layout(bank, channels, opts)
        assert lay["lens"] == got["lens"] and lay["breaks"] == got["breaks"] and lay["max_len"] == got["saa_up"].shape[1]
        only = pairread.bank_csd(bank, channels, opts)
        assert "frequencies" not in only and "coherence_up" not in only and only["sab_lo"].tobytes() == got["sab_lo"].tobytes()
    print(state["name"], selection, "coherence within", worst[0], "* 2^-24 (bound 9), H1 within", worst[1], "* 2^-24 (bound 5)")


def test_the_read_out_changes_nothing(pkg, pairread, state):
    """csd(p), sidebands(p), am_pm_cross(p, carriers) and am_pm_cross(p) after all of the above equal what they were before (byte for
    byte, Breaks field for field), and those of the twin bank that never saw a bank read-out"""
    bank, twin, kind = state["bank"], state["twin"], state["kind"]
    pairread.bank_csd(bank, bands=[(0.0, 0.5)], **ALL_CSD)
    if kind == "xampm":
        pairread.bank_am_pm_cross(bank, carriers=GIVEN, frequencies=True, bands=[(0.0, 0.5)])
    for p in range(6):
        for opts in two_opts(pkg):
            a, b, before = own_reads(bank, kind, state["detrend"], p, opts), own_reads(twin, kind, state["detrend"], p, opts), state["own"][opts][p]
            assert len(a) == (1 if kind == "csd" else 3 if state["detrend"] or p in (EMPTY, ZEROS) else 4)
            assert a == b == before, (p, opts)


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


def device_call(torch, fn, outs, bank, host, channels, opts, keys, **kw):
    """the device form into fresh sentinel tensors for `keys`; returns (result, {key: tensor}, stride)"""
    rows, width = host[keys[0]].shape
    stride = width + 7
    t = {k: device_tensor(torch, rows, stride, outs[k][1]) for k in keys}
    got = fn(bank, stride, pairs=channels, opts=opts, **{outs[k][0]: v.data_ptr() for k, v in t.items()}, **kw)
    return got, t, stride


@pytest.mark.parametrize("selection", ["all", "subset with a duplicate"])
def test_device_form(pkg, pairread, state, selection):
    """sentinel-filled tensors with stride > max_len: exactly [0, lens[i]) of each asked row is written, all together and each
    output alone (a thread loads only the rows its outputs need); the carrier records alone; a second call gives the same bits"""
    import torch
    channels = SELECTIONS[selection]
    sel = pairs_of(channels)
    bank = state["bank"]
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True)):
        host = pairread.bank_csd(bank, channels, opts, **ALL_CSD)
        again = pairread.bank_csd(bank, channels, opts, **ALL_CSD)
        assert all(host[k].tobytes() == again[k].tobytes() for k in CSD_OUTS)
        got, t, stride = device_call(torch, pairread.bank_csd_device, CSD_OUTS, bank, host, channels, opts, list(CSD_OUTS))
        assert got["lens"] == host["lens"] and got["breaks"] == host["breaks"] and got["launches"] == 1
        for k in CSD_OUTS:
            check_device_rows(t[k], host[k], host["lens"], stride, CSD_OUTS[k][1], k)
        for k in CSD_OUTS:  # each output alone
            got, t, stride = device_call(torch, pairread.bank_csd_device, CSD_OUTS, bank, host, channels, opts, [k])
            assert got["launches"] == 1
            check_device_rows(t[k], host[k], host["lens"], stride, CSD_OUTS[k][1], k + " alone")
        if state["kind"] != "xampm":
            continue
        car = [GIVEN[p] for p in sel]
        host = pairread.bank_am_pm_cross(bank, channels, car, opts, frequencies=True)
        got, t, stride = device_call(torch, pairread.bank_am_pm_cross_device, AMPM_OUTS, bank, host, channels, opts, list(AMPM_OUTS), carriers=car)
        assert got["lens"] == host["lens"] and got["launches"] == 1
        for k in AMPM_OUTS:
            check_device_rows(t[k], host[k], host["lens"], stride, 4 if k != "frequencies" else 1, k)
        for k in AMPM_OUTS:
            got, t, stride = device_call(torch, pairread.bank_am_pm_cross_device, AMPM_OUTS, bank, host, channels, opts, [k], carriers=car)
            assert got["launches"] == 1
            check_device_rows(t[k], host[k], host["lens"], stride, AMPM_OUTS[k][1], k + " alone")
        tc = torch.full((7 * len(sel) + 5,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        got = pairread.bank_am_pm_cross_device(bank, 0, carrier=tc.data_ptr(), pairs=channels, carriers=car, opts=opts)
        out = tc.cpu().numpy()
        assert got["launches"] == 1 and same(out[:7 * len(sel)].reshape(-1, 7), host["carrier"]) and np.all(out[7 * len(sel):] == -7.0)


def test_done_event_form(pkg, pairread, state):
    """four calls that return early, back to back with different options, each into its own tensors (the two job-table slots are
    reused), waited for through their events: the host form's bytes"""
    import torch
    bank = state["bank"]
    opts = [pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True), pkg.MergeOpts(min_count=2),
            pkg.MergeOpts(keep_transition_band=True)]
    keys = ["sbb_lo", "sab_up", "coherence_lo", "transfer_up"]
    host = [pairread.bank_csd(bank, None, o, **ALL_CSD) for o in opts]
    events = []
    for _ in opts:
        ev = torch.cuda.Event()
        ev.record()  # (the handle exists once the event has been recorded)
        events.append(ev)
    torch.cuda.synchronize()
    calls = [device_call(torch, pairread.bank_csd_device, CSD_OUTS, bank, h, None, o, keys, done_event=ev.cuda_event)
             for h, o, ev in zip(host, opts, events)]  # back to back, no wait in between
    for k, ((got, t, stride), h, ev) in enumerate(zip(calls, host, events)):
        ev.synchronize()
        assert got["lens"] == h["lens"] and got["launches"] == 1
        for key in keys:
            check_device_rows(t[key], h[key], h["lens"], stride, CSD_OUTS[key][1], f"{key} of call {k} of four back to back")
    unfed = pairread.bank_csd_device(bank, 4, saa_up=calls[0][1][keys[0]].data_ptr(), pairs=[EMPTY], done_event=events[0].cuda_event)
    events[0].synchronize()  # (recorded even though nothing was launched)
    assert unfed["launches"] == 0


def test_am_pm_cross(pkg, pairread, ampm_state):
    """cab / cba equal sidebands(p) byte for byte.  The four AM/PM rows and the carrier record equal tests/pair_read_ref.py on the
    pair's own stage_rows byte for byte.  Given carriers against am_pm_cross(p, carriers) and, under Detrend.NONE, carriers=None
    against am_pm_cross(p) on the pairs that have carriers: |got - want| <= 16 * 2^-53 * (|U| + |L| + |cab| + |cba|) / (4 P) a bin
    -- at most eight f64 roundings a side on terms of at most that size --; the record within 4 * 2^-53 relative of carriers(p)
    (hypot there, the square root of the sum of squares here).  EMPTY and ZEROS without given carriers: the record (0, NaN x 6),
    NaN AM/PM rows, cab / cba / frequencies unaffected.  Under a detrend carriers=None is refused for every output that needs them."""
    state = ampm_state
    bank, n = state["bank"], state["n"]
    routes = ([None] if not state["detrend"] else []) + [GIVEN]
    if state["detrend"]:
        import torch
        w = pairread.layout(bank)["max_len"]
        t = device_tensor(torch, 6, w, 4)
        for kw in (dict(s_pm=t.data_ptr()), dict(s_pm_am=t.data_ptr()), dict(carrier=t.data_ptr()), dict(bands=[(0.0, 0.5)], band_ptr=t.data_ptr())):
            with pytest.raises(pkg.PsdError) as e:
                pairread.bank_am_pm_cross_device(bank, w, **kw)
            assert e.value.code == pkg.ERR_ARG and "PSDC_DETREND_NONE" in str(e.value)
        assert np.all(t.cpu().numpy() == SENTINEL)  # (nothing written)
        assert pairread.bank_am_pm_cross_device(bank, w, cab=t.data_ptr())["launches"] == 1  # (no output that needs the carriers)
    for carriers in routes:
        for opts in two_opts(pkg):
            got = pairread.bank_am_pm_cross(bank, None, carriers, opts, frequencies=True)
            worst = 0.0
            for p in range(6):
                ln, rec = got["lens"][p], got["carrier"][p]
                sb = bank.sidebands(p, opts)
                assert got["breaks"][p] == sb[8] and ln == len(sb[6])
                assert got["cab"][p, :ln].tobytes() == sb[6].tobytes() and got["cba"][p, :ln].tobytes() == sb[7].tobytes(), p
                assert got["frequencies"][p, :ln].tobytes() == pkg.Break.frequencies(sb[8]).tobytes()
                for key in ("cab", "cba") + AMPM_KEYS:
                    assert np.all(np.isnan(got[key][p, ln:])), (p, key)
                acc, counts = state["acc"][p]
                if carriers is None:
                    car = ref.carriers_from_bin0(n, state["wt"].power, counts[0] if counts else None, acc[0][:, 0] if counts else None)
                else:
                    car = ref.carriers_given(*carriers[p])
                assert same(rec, np.asarray(car)), (p, rec, car)
                if carriers is None and p in (EMPTY, ZEROS):
                    assert rec[0] == 0.0 and np.all(np.isnan(rec[1:]))
                    assert all(np.all(np.isnan(got[key][p])) for key in AMPM_KEYS)
                    continue
                if carriers is None:
                    p_ab, w, q, lock_w, lock_q = bank.carriers(p)
                    for a, b in ((rec[0], p_ab), (rec[5], lock_w), (rec[6], lock_q)):
                        assert abs(a - b) <= 4 * EPS * b, (p, rec, a, b)
                    assert abs(complex(rec[1], rec[2]) - w) <= 4 * EPS and abs(complex(rec[3], rec[4]) - q) <= 4 * EPS, (p, rec, w, q)
                    if p == ODD:
                        assert rec[5] < 0.999, rec
                    elif p in (LONG, TWIN):
                        assert rec[5] > 1 - 1e-4 and rec[6] > 1 - 1e-4, rec
                    want = bank.am_pm_cross(p, None, opts)
                else:
                    assert np.isnan(rec[5]) and np.isnan(rec[6])
                    if p == EMPTY:
                        assert ln == 0
                        continue
                    want = bank.am_pm_cross(p, carriers[p], opts)
                rows, g = restated(state, p, got["breaks"][p])
                s = ref.split(rows, g, car)
                scale = (np.abs(sb[4]) + np.abs(sb[5]) + np.abs(sb[6]) + np.abs(sb[7])) / (4.0 * rec[0])
                ok = np.isfinite(scale)  # (a stage without a segment, included by min_count = 0, has no finite scale)
                for k, key in enumerate(AMPM_KEYS):
                    v = got[key][p, :ln]
                    assert same(v, s[:, 2 * k:2 * k + 2].copy().view(np.complex128)[:, 0]), (p, key)
                    assert np.array_equal(ok, np.isfinite(v)), (p, key)
                    d = np.abs(v - want[k])[ok]
                    pos = scale[ok] > 0  # (scale 0: an all-zero stream under given carriers; the differences are 0 there)
                    if pos.any():
                        worst = max(worst, float(np.max(d[pos] / (EPS * scale[ok][pos]))))
                    assert np.all(d <= 16 * EPS * scale[ok]), (p, key, worst)
            print(state["name"], "given" if carriers else "bin 0", opts.keep_overlap, "worst against am_pm_cross():", worst, "* 2^-53 of the scale")


def test_physics(pkg, pairread, own_carrier_state):
    """LONG under Detrend.NONE: the shared AM tone's bin (offset 1/8) shows in s_am and not in s_pm, the shared PM tone's bin
    (offset 3/16) the reverse, the wrong one below 1e-2 of the right one in magnitude; the band around the PM tone integrates
    Re s_pm to the tone's mean-square phase A_PM^2 / 2 = 2e-4 rad^2 within 2 % (the sibling's single-channel integral reads
    0.6 % high on the zoom banks; each side's own noise adds its cross term of either sign)"""
    state = own_carrier_state
    got = pairread.bank_am_pm_cross(state["bank"], [LONG], None, pkg.MergeOpts(), frequencies=True, bands=[(0.16, 0.22)])
    f = got["frequencies"][0, :got["lens"][0]]
    k_am, k_pm = int(np.argmin(np.abs(f - F_AM))), int(np.argmin(np.abs(f - F_PM)))
    assert f[k_am] == np.float32(F_AM) and f[k_pm] == np.float32(F_PM)
    s_am, s_pm = got["s_am"][0], got["s_pm"][0]
    print(state["name"], "AM bin", s_am[k_am], s_pm[k_am], "PM bin", s_am[k_pm], s_pm[k_pm], "band", got["band_sums"][0])
    assert abs(s_pm[k_am]) < 1e-2 * abs(s_am[k_am]) and abs(s_am[k_pm]) < 1e-2 * abs(s_pm[k_pm])
    assert got["band_sums"].dtype == np.complex128 and got["band_sums"].shape == (1, 1, 4)
    assert abs(got["band_sums"][0, 0, 1].real - A_PM ** 2 / 2) <= 0.02 * A_PM ** 2 / 2


def bands_of():
    """the whole range; most of stage 0; a decade across a seam; a single bin (k = n/4 of stage 0); none; three more"""
    return [(0.0, 0.5), (0.0501, 0.5), (0.01, 0.1), (0.25, 0.25), (0.30001, 0.30002), (1e-4, 1e-2), (0.1, 0.2), (0.0, 1e-3)]


def csd_values(got, p):
    ln = got["lens"][p]
    return np.stack([got["saa_up"][p, :ln], got["saa_lo"][p, :ln], got["sbb_up"][p, :ln], got["sbb_lo"][p, :ln], got["sab_up"][p, :ln].real,
                     got["sab_lo"][p, :ln].real, got["sab_up"][p, :ln].imag, got["sab_lo"][p, :ln].imag]).astype(np.float64)


def test_band_sums(pkg, pairread, state):
    """bit-equal to the host restatement (tests/pair_read_ref.py: bank_band_rows_host's thread stride, shuffle tree and wavefront
    order) on the read-out's own rows for 1 to 8 bands, among them a band that holds no bin; a pair with nothing included gives 0.0;
    the same bits from a second call, from bands alone (one launch) and from the device form; band_coherence() of the sums"""
    import torch
    bank, bands = state["bank"], bands_of()
    nonzero = 0
    for opts in two_opts(pkg)[:1] + (pkg.MergeOpts(keep_overlap=True, keep_transition_band=True),):
        for nb in range(1, 9):
            if nb not in (1, 5, 8) and opts != pkg.MergeOpts():
                continue
            got = pairread.bank_csd(bank, None, opts, frequencies=True, bands=bands[:nb])
            assert got["launches"] == 2 and got["band_sums"].shape == (6, nb, 8) and got["band_sums"].dtype == np.float64
            for p in range(6):
                ln = got["lens"][p]
                want = ref.band_sums(csd_values(got, p), got["frequencies"][p, :ln], bands[:nb])
                assert got["band_sums"][p].tobytes() == want.tobytes(), (state["name"], opts, nb, p, got["band_sums"][p], want)
            assert np.all(got["band_sums"][EMPTY] == 0.0) and np.all(got["band_sums"][ZEROS] == 0.0)
            if nb >= 5:
                assert np.all(got["band_sums"][:, 4] == 0.0)  # the band that holds no bin
            nonzero += int(np.count_nonzero(got["band_sums"]))
            if state["kind"] == "xampm":
                am = pairread.bank_am_pm_cross(bank, None, GIVEN, opts, frequencies=True, bands=bands[:nb])
                assert am["launches"] == 2 and am["band_sums"].shape == (6, nb, 4) and am["band_sums"].dtype == np.complex128
                for p in range(6):
                    ln = am["lens"][p]
                    vals = np.concatenate([np.stack([am[k][p, :ln].real, am[k][p, :ln].imag]) for k in AMPM_KEYS])
                    if not np.all(np.isfinite(vals)):
                        continue
                    want = ref.band_sums(vals, am["frequencies"][p, :ln], bands[:nb])
                    assert am["band_sums"][p].view(np.float64).tobytes() == want.tobytes(), (state["name"], opts, nb, p)
                assert np.all(am["band_sums"][EMPTY] == 0.0)
        co = pairread.band_coherence(got["band_sums"])
        assert co[0].shape == (6, 8) and np.all(np.isnan(co[0][EMPTY])) and np.all(co[0][LONG, :4] > 0)
        # the same bits from a second call, from bands alone, and from the device form with a row
        again = pairread.bank_csd(bank, None, opts, bands=bands)
        assert again["band_sums"].tobytes() == got["band_sums"].tobytes()
        count = 6 * 8 * 8
        tb = torch.full((count + 3,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        alone = pairread.bank_csd_device(bank, 0, opts=opts, bands=bands, band_ptr=tb.data_ptr())
        assert alone["launches"] == 1
        out = tb.cpu().numpy()
        assert out[:count].tobytes() == got["band_sums"].tobytes() and np.all(out[count:] == -1.0)
        tb.fill_(-1.0)
        stride = got["saa_up"].shape[1] + 3
        tu = device_tensor(torch, 6, stride, 2)
        both = pairread.bank_csd_device(bank, stride, coh_lo=tu.data_ptr(), opts=opts, bands=bands, band_ptr=tb.data_ptr())
        assert both["launches"] == 2 and tb.cpu().numpy()[:count].tobytes() == got["band_sums"].tobytes()
    assert nonzero >= 3 * 4 * 8  # at least three fed pairs, four bands that hold bins, eight rows that are not zero
    # a pair with nothing included: nothing is launched, the band sums are 0.0
    tb = torch.full((8 * 8,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    unfed = pairread.bank_csd_device(bank, 0, pairs=[EMPTY], bands=bands, band_ptr=tb.data_ptr())
    assert unfed["launches"] == 0 and np.all(tb.cpu().numpy() == 0.0)
    none = pairread.bank_csd(bank, [LONG, EMPTY], pkg.MergeOpts(min_count=10 ** 6), bands=bands)
    assert none["launches"] == 0 and none["saa_up"].shape == (2, 0) and np.all(none["band_sums"] == 0.0)


@pytest.mark.parametrize("kind", ["csd", "xampm"])
def test_seventy_pairs_in_one_launch(pkg, pairread, gpu_required, kind):
    """a bank of 70 pairs of which 3 are fed, all 70 selected: one launch (jobs run along x), two with bands, and the object's
    stats_read grows by the same number; the single object goes through the same call; release() and the next call"""
    bank = getattr(pkg, CLASSES["zoom", kind])(64, 70)
    fed = (3, 40, 69)
    for p in fed:
        bank.set_carrier(p, f0=F0)
        bank.process(p, side(pkg, False, 3000 + p, p), side(pkg, False, 3000 + p, 100 + p, theta=1.0))
    bank.sync()  # (the feed's own launches are counted before the first read-out)
    bands = [(0.0, 0.5), (0.01, 0.1)]
    calls = [(pairread.bank_csd, dict(frequencies=True, bands=bands), 2), (pairread.bank_csd, {}, 1)]
    if kind == "xampm":
        calls += [(pairread.bank_am_pm_cross, dict(bands=bands), 2), (pairread.bank_am_pm_cross, {}, 1)]
    res = []
    for fn, kw, launches in calls:
        before = bank.stats_read()["launches"]
        res.append(fn(bank, **kw))
        assert res[-1]["launches"] == launches and bank.stats_read()["launches"] - before == launches
    got = res[0]
    for p in range(70):
        r = bank.csd(p)
        assert got["lens"][p] == len(r[0]) and got["breaks"][p] == r[6] and (len(r[0]) > 0) == (p in fed)
        if kind == "csd":
            assert got["saa_up"][p, :len(r[0])].tobytes() == r[0].tobytes() and got["sab_lo"][p, :len(r[0])].tobytes() == r[5].tobytes()
        else:
            rec = res[2]["carrier"][p]
            assert (rec[0] > 0) == (p in fed) and np.isnan(rec[1]) == (p not in fed)
        if p not in fed:
            assert np.all(got["band_sums"][p] == 0.0)
    sel = list(range(69, -1, -1)) * 2
    twice = pairread.bank_csd(bank, sel)
    assert twice["launches"] == 1 and twice["saa_up"].shape[0] == 140
    assert twice["sbb_lo"][0].tobytes() == got["sbb_lo"][69].tobytes() and twice["sbb_lo"][70 + 29].tobytes() == got["sbb_lo"][40].tobytes()
    pairread.release(bank)  # the buffers come back with the next call
    assert pairread.bank_csd(bank)["saa_up"].tobytes() == got["saa_up"].tobytes()
    single = getattr(pkg, CLASSES["zoom", kind][:-4])(64, f0=F0)
    single.process(side(pkg, False, 3003, 3), side(pkg, False, 3003, 103, theta=1.0))
    one = pairread.bank_csd(single)
    assert one["saa_up"][0].tobytes() == got["saa_up"][3, :one["lens"][0]].tobytes()
    single.close()
    bank.close()


def test_errors(pkg, pairread, state):
    """PSDC_ERR_CAPACITY with a retry (stride, breaks_cap), and every refusal text of the header"""
    import torch
    bank, kind = state["bank"], state["kind"]
    L = pairread._lib()
    lay = pairread.layout(bank)
    stride = lay["max_len"] - 1
    t = device_tensor(torch, 6, lay["max_len"], 4)
    ptr, width = t.data_ptr(), lay["max_len"]
    last = lambda: bank._f("last_error")(bank._h).decode()  # noqa: E731
    c = pairread._Call(bank, None, None, ("csd", "ampm"))
    rc = L.psdcpr_csd_device(*c.head, None, C.c_void_p(ptr), *[None] * 9, stride, None, 0, None, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and "stride" in last()
    assert c.result()["lens"] == lay["lens"] and int(c.info.max_len) == lay["max_len"] and int(c.info.launches) == 0
    assert np.all(t.cpu().numpy() == SENTINEL)
    rc = L.psdcpr_csd_device(*c.head, None, C.c_void_p(ptr), *[None] * 9, int(c.info.max_len), None, 0, None, None, *c.tail)  # the retry
    assert rc == 0 and int(c.info.launches) == 1
    t = device_tensor(torch, 6, lay["max_len"], 4)
    ptr = t.data_ptr()
    host = np.zeros((6, lay["max_len"]), np.float32)
    c = pairread._Call(bank, None, None, ("csd", "ampm"))
    rc = L.psdcpr_csd(*c.head, host.ctypes.data, *[None] * 10, stride, None, 0, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and c.result()["lens"] == lay["lens"] and np.all(host == 0)
    c = pairread._Call(bank, None, None, ("csd", "ampm"))  # room for fewer breaks than pair 0 has, then a retry
    rc = L.psdcpr_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, 2, C.byref(c.info))
    assert rc == pkg.ERR_CAPACITY and [int(v) for v in c.lens] == lay["lens"] and int(c.nb[0]) == len(lay["breaks"][0]) > 2
    rc = L.psdcpr_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, int(c.nb.max()), C.byref(c.info))
    assert rc == 0

    def arg_error(text, fn, *args, **kw):
        with pytest.raises(pkg.PsdError) as e:
            fn(bank, *args, **kw)
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))

    arg_error("out of range", pairread.bank_csd, [0, 6])
    arg_error("out of range", pairread.layout, [6])
    arg_error("out of range", pairread.bank_csd_device, width, saa_up=ptr, pairs=[7])
    arg_error("more than 8 bands", pairread.bank_csd_device, width, saa_up=ptr, bands=[(0.0, 0.1)] * 9, band_ptr=ptr)
    arg_error("bands without a band output", pairread.bank_csd_device, width, saa_up=ptr, bands=[(0.0, 0.1)])
    arg_error("a band output without bands", pairread.bank_csd_device, width, saa_up=ptr, band_ptr=ptr)
    arg_error("a band with NaN or lo > hi", pairread.bank_csd, bands=[(0.0, 0.1), (float("nan"), 0.2)])
    arg_error("no output", pairread.bank_csd_device, width)
    c = pairread._Call(bank, None, None, ("csd", "ampm"))
    if kind == "csd":
        arg_error("takes a ZoomAmPmCsdCascade", pairread.bank_am_pm_cross)
        rc = L.psdcpr_ampm(*c.head, None, host.ctypes.data, *[None] * 7, width, None, 0, None, *c.tail)  # the C call looks at the kind itself
        assert rc == pkg.ERR_ARG and last() == "psdcpr_ampm: takes a zoom AM/PM cross or IQ AM/PM cross object"
        rc = L.psdcpr_ampm_device(*c.head, None, C.c_void_p(ptr), *[None] * 7, width, None, 0, None, None, *c.tail)
        assert rc == pkg.ERR_ARG and last() == "psdcpr_ampm_device: takes a zoom AM/PM cross or IQ AM/PM cross object"
    else:
        bad = "given carriers must be finite"
        good = list(GIVEN)
        for wrong in ((0.0, 1, 1), (-1.0, 1, 1), (1.0, 0j, 1), (1.0, 1, 0j), (float("nan"), 1, 1), (1.0, complex(float("inf"), 0), 1), (1.0, 1, complex(0, float("nan")))):
            arg_error(bad, pairread.bank_am_pm_cross, None, good[:5] + [wrong])
        arg_error(bad, pairread.bank_am_pm_cross_device, width, s_am=ptr, carriers=[(0.0, 1, 1)] * 6)
        arg_error("one (p_ab, w, q)", pairread.bank_am_pm_cross, None, good[:2])
        arg_error("no output", pairread.bank_am_pm_cross_device, width)
        arg_error("more than 8 bands", pairread.bank_am_pm_cross_device, width, carriers=good, bands=[(0.0, 0.1)] * 9, band_ptr=ptr)
        arg_error("bands without a band output", pairread.bank_am_pm_cross_device, width, cab=ptr, carriers=good, bands=[(0.0, 0.1)])
    rc = L.psdcpr_layout(*c.head, None, c.nb.ctypes.data, None, 0, None)
    assert rc == pkg.ERR_ARG and last() == "psdcpr_layout: null lens"
    rc = L.psdcpr_layout(*c.head, c.lens.ctypes.data, None, c.br.ctypes.data, 16, None)
    assert rc == pkg.ERR_ARG and last() == "psdcpr_layout: breaks without n_breaks"
    assert np.all(t.cpu().numpy() == SENTINEL) and np.all(host == 0)
    # another object of the same runtime: the binding refuses it, and so does every C call
    other = pkg.ZoomAmPmCascadeBank(64, 2)
    for fn in (pairread.layout, pairread.bank_csd, pairread.bank_am_pm_cross, pairread.release):
        with pytest.raises(pkg.PsdError) as e:
            fn(other)
        assert e.value.code == pkg.ERR_ARG
    lens = np.full(2, 55, np.uintp)
    tail = (lens.ctypes.data, None, None, 0, None)
    head = (other._h, None, 0, 0, 1, 0)
    text = ": takes a zoom cross, IQ cross or zoom / IQ AM/PM cross object"
    for name, args in (("layout", (*head, *tail)), ("csd", (*head, host.ctypes.data, *[None] * 10, width, None, 0, None, *tail)),
                       ("csd_device", (*head, C.c_void_p(ptr), *[None] * 10, width, None, 0, None, None, *tail)), ("release", (other._h,))):
        assert getattr(L, "psdcpr_" + name)(*args) == pkg.ERR_ARG
        assert pkg.lib().psdc_zampm_last_error(other._h).decode() == "psdcpr_" + name + text
    assert np.all(lens == 55) and np.all(host == 0)
    other.close()
    before = pairread.bank_csd(bank)
    pairread.release(bank)
    pairread.release(bank)
    after = pairread.bank_csd(bank)  # the buffers are made again
    assert after["saa_up"].tobytes() == before["saa_up"].tobytes() and after["sab_lo"].tobytes() == before["sab_lo"].tobytes()
