"""Bank read-out of the carrier objects on the MI355X (include/psdcascade_carrierread.h, psdczr_*;
stabilizer-stream_amd/carrierread.py): one call stitches every selected channel of a zoom, IQ, zoom / IQ SK or zoom / IQ AM/PM bank
on the device.  upper, lower, the frequencies, lengths and Breaks must equal what psd(c) and Break.frequencies return, byte for byte
and field for field; sk_upper / sk_lower equal sk(c) byte for byte; the AM/PM outputs are held to am_pm(c) / carrier(c) within a
bound of a few f64 roundings and to tests/carrier_read_ref.py on the channel's own stage_rows; the band sums are deterministic f64
sums checked against numpy and, bit for bit, against the host restatement.

Shapes: n = 64 (33 bins: one tile; the zoom and the IQ class) and n = 1024 (513 bins: the third tile of a job holds ONE element)
with the Hann window, n = 256 with the rectangular window; one n = 64 bank under set_avg with a small limit and one under Mean
detrend.  A bank has six channels fed in several calls: LONG (three or more live stages; a carrier at the tuning word with an AM tone
at offset 1/8, a PM tone delayed by three samples at offset 3/16 and noise), ODD (an odd length, the carrier detuned by
1 / (8 n 64): lock visibly below 1), SHORT (one stage of one or two segments), EMPTY (never fed), ZEROS (all zeros: the NaN paths)
and TWIN (LONG again, its last half call fed right before the first read-out).  `twin` is a second bank fed the same calls that
never sees a bank read-out."""
import ctypes as C
import itertools
import struct
import subprocess

import numpy as np
import pytest

import carrier_read_ref as ref

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
STATES = [(s, "zoom", m) for s in SHAPES for m in ("sides", "sk", "ampm")] + [("n64", "iq", m) for m in ("sides", "sk", "ampm")]
CLASSES = {("zoom", "sides"): "ZoomCascadeBank", ("iq", "sides"): "IqCascadeBank", ("zoom", "sk"): "ZoomSkCascadeBank",
           ("iq", "sk"): "IqSkCascadeBank", ("zoom", "ampm"): "ZoomAmPmCascadeBank", ("iq", "ampm"): "IqAmPmCascadeBank"}
LONG, ODD, SHORT, EMPTY, ZEROS, TWIN = range(6)
SELECTIONS = {"all": None, "permutation": [4, 2, 0, 5, 3, 1], "subset with a duplicate": [1, 5, 1], "the unfed channel alone": [EMPTY]}
OUTS = {"sides": (("upper", 1), ("lower", 1), ("frequencies", 1)),  # (key, 32-bit words a bin)
        "sk": (("upper", 1), ("lower", 1), ("frequencies", 1), ("sk_upper", 2), ("sk_lower", 2)),
        "ampm": (("upper", 1), ("lower", 1), ("frequencies", 1), ("s_am", 2), ("s_pm", 2), ("s_ampm", 4))}
DEVICE_ARG = {"frequencies": "freq"}
F0, F_AM, F_PM, A_AM, A_PM, AMP, THETA = 0.25, 1.0 / 8, 3.0 / 16, 0.01, 0.02, 0.5, 0.3
EPS = 2.0 ** -53
GIVEN = [0.5 * np.exp(0.3j), 0.25 - 0.1j, 1.0 + 0j, 0.7j, 0.3 + 0.3j, 0.5 * np.exp(0.3j)]  # the amplitudes of a given-carriers call


def all_opts(pkg):
    return [pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)
            for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 2, 10 ** 6))]


@pytest.fixture(scope="module")
def carrierread(pkg):
    from stabilizer_stream_amd import carrierread as mod
    return mod


def stream(pkg, iq, length, seed, detune=0.0):
    """a carrier of amplitude 2 AMP (real) / AMP (complex) with a = A_AM cos(2 pi F_AM j), phi = A_PM sin(2 pi F_PM (j - 3)) and
    white noise of 1e-4: real at F0 + detune for the zoom classes, complex at detune for the IQ classes.  Mean-square phase of the
    tone: A_PM^2 / 2."""
    j = np.arange(length, dtype=np.float64)
    a = A_AM * np.cos(2 * np.pi * F_AM * j)
    phi = A_PM * np.sin(2 * np.pi * F_PM * (j - 3))
    noise = 1e-4 * pkg.noise_host(length, seed=seed).astype(np.float64)
    if iq:
        z = AMP * (1 + a) * np.exp(1j * (2 * np.pi * detune * j + THETA + phi))
        return (z + noise + 1j * 1e-4 * pkg.noise_host(length, seed=seed + 7)).astype(np.complex64)
    return (2 * AMP * (1 + a) * np.cos(2 * np.pi * (F0 + detune) * j + THETA + phi) + noise).astype(np.float32)


def feed(pkg, bank, n, iq, long, mid, short, last_half):
    """the calls of a bank; last_half: called right before the TWIN channel's last half call"""
    if not iq:
        for c in range(6):
            bank.set_carrier(c, f0=F0)
    x = stream(pkg, iq, long, 1000 + n)
    piece = long // 4
    for k in range(4):
        bank.process(LONG, x[k * piece:(k + 1) * piece])
    for part in np.array_split(stream(pkg, iq, mid, 2000 + n, detune=1.0 / (8 * n * 64)), 3):
        bank.process(ODD, part)
    bank.process(SHORT, stream(pkg, iq, short, 3000 + n))
    for part in np.array_split(np.zeros(mid, x.dtype), 2):
        bank.process(ZEROS, part)
    for k in range(3):
        bank.process(TWIN, x[k * piece:(k + 1) * piece])
    half = 3 * piece + piece // 2
    bank.process(TWIN, x[3 * piece:half])
    last_half()
    bank.process(TWIN, x[half:])


def host_call(carrierread, mode, bank, channels=None, opts=None, **kw):
    return {"sides": carrierread.bank_sides, "sk": carrierread.bank_sk, "ampm": carrierread.bank_am_pm}[mode](bank, channels, opts=opts, **kw)


def device_fn(carrierread, mode):
    return {"sides": carrierread.bank_sides_device, "sk": carrierread.bank_sk_device, "ampm": carrierread.bank_am_pm_device}[mode]


_MADE = {}  # the states made so far, by their parameters: the two fixtures below share them


@pytest.fixture(scope="module", autouse=True)
def close_states():
    yield
    for st in _MADE.values():
        st["twin"].close()
        st["bank"].close()
    _MADE.clear()


def two_opts(pkg):
    return (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True))


def own_reads(bank, mode, detrend, c, opts):
    """what the object's own per-channel read-outs beyond psd(c) return, as (bytes of every row, breaks): sk(c); sidebands(c),
    am_pm(c, A) and, where the channel has a carrier in bin 0, am_pm(c) with carrier=None (carrier() and its own snapshot)"""
    calls = []
    if mode == "sk":
        calls.append(bank.sk(c, opts))
    if mode == "ampm":
        calls += [bank.sidebands(c, opts), bank.am_pm(c, GIVEN[c], opts)]
        if not detrend and c not in (EMPTY, ZEROS):
            calls.append(bank.am_pm(c, None, opts))
    return [([np.asarray(v).tobytes() for v in r[:-1]], r[-1]) for r in calls]


def make_state(pkg, carrierread, param):
    """one fed bank a (shape, family, mode): dict(bank, twin, first, ref).  `first` is the bank read-out made right behind the
    TWIN channel's last half call; ref[opts] = [(upper, lower, breaks, frequencies)] of every channel from psd(c), computed once"""
    if param in _MADE:
        return _MADE[param]
    shape, family, mode = param
    n, window, long, mid, short, avg, detrend = SHAPES[shape]
    iq = family == "iq"
    banks = []
    for _ in range(2):
        bank = getattr(pkg, CLASSES[family, mode])(n, 6, getattr(pkg.Window, window))
        if avg:
            bank.set_avg(pkg.AvgOpts(*avg))
        if detrend:
            bank.set_detrend(getattr(pkg.Detrend, detrend))
        feed(pkg, bank, n, iq, long, mid, short, bank.sync)
        banks.append(bank)
    bank, twin = banks
    given = GIVEN if detrend else None  # (bin 0 holds no carrier under a detrend)
    kw = dict(carriers=given) if mode == "ampm" else {}
    first = host_call(carrierread, mode, bank, frequencies=True, **kw)
    refs = {}
    for opts in all_opts(pkg) + [pkg.MergeOpts()]:
        refs[opts] = [(*r, pkg.Break.frequencies(r[2])) for r in (bank.psd(c, opts) for c in range(6))]
    # (taken behind `first`, as the psd(c) references are, so that `first` still finds the half call undrained; every other bank
    # read-out of this file comes after them)
    own = {opts: [own_reads(bank, mode, detrend, c, opts) for c in range(6)] for opts in two_opts(pkg)}
    _MADE[param] = dict(bank=bank, twin=twin, first=first, ref=refs, own=own, n=n, name="-".join(param), window=window, mode=mode, kw=kw,
                        given=given, detrend=detrend)
    return _MADE[param]


@pytest.fixture(scope="module", params=STATES, ids=["-".join(s) for s in STATES])
def state(request, pkg, carrierread, gpu_required):
    return make_state(pkg, carrierread, request.param)


AMPM_STATES = [s for s in STATES if s[2] == "ampm"]


@pytest.fixture(scope="module", params=AMPM_STATES, ids=["-".join(s) for s in AMPM_STATES])
def ampm_state(request, pkg, carrierread, gpu_required):
    """the AM/PM objects among the states"""
    return make_state(pkg, carrierread, request.param)


OWN_CARRIER_STATES = [s for s in AMPM_STATES if not SHAPES[s[0]][6]]


@pytest.fixture(scope="module", params=OWN_CARRIER_STATES, ids=["-".join(s) for s in OWN_CARRIER_STATES])
def own_carrier_state(request, pkg, carrierread, gpu_required):
    """... that read their own carrier (no detrend)"""
    return make_state(pkg, carrierread, request.param)


def check_rows(got, refs, channels, what):
    """a bank read-out's rows, lens and breaks against psd(c) of each selected channel"""
    sel = range(len(refs)) if channels is None else channels
    width = max([len(refs[c][0]) for c in sel] or [0])
    for key in ("upper", "lower", "frequencies"):
        assert got[key].dtype == np.float32 and got[key].shape == (len(sel), width), (what, key)
    for i, c in enumerate(sel):
        up, lo, br, f = refs[c]
        assert got["lens"][i] == len(up), (what, i)
        assert got["breaks"][i] == br, (what, i)  # field for field (a frozen dataclass)
        for key, want in (("upper", up), ("lower", lo), ("frequencies", f)):
            assert got[key][i, :len(up)].tobytes() == want.tobytes(), (what, i, key)
            assert np.all(np.isnan(got[key][i, len(up):])), (what, i, key)


def test_shape_is_what_the_cases_need(pkg, state):
    rows = next(iter(state["ref"].values()))
    live = [sum(b.count > 0 for b in r[2]) for r in rows]  # stages that hold a segment
    print(state["name"], "live stages", live, "stage-0 counts", [r[2][-1].count if r[2] else None for r in rows])
    assert live[LONG] >= 3 and live[TWIN] == live[LONG] and live[ODD] >= 2 and live[SHORT] == 1 and live[EMPTY] == 0 and not rows[EMPTY][2], live
    assert 1 <= rows[SHORT][2][-1].count <= 2 and live[ZEROS] >= 2
    if state["n"] == 1024:  # a job of 513 bins: three tiles, the last of one element
        assert any(len(b.bins) == 513 for b in state["bank"].psd(LONG, pkg.MergeOpts(keep_transition_band=True))[2])


def test_first_read_out_behind_a_half_call(pkg, state):
    refs = [(*r, pkg.Break.frequencies(r[2])) for r in (state["bank"].psd(c) for c in range(6))]  # (the default options)
    check_rows(state["first"], refs, None, "first read-out")
    assert state["first"]["launches"] == 1


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_host_form_equals_psd(pkg, carrierread, state, selection):
    """upper, lower, lens, breaks and frequencies for every merge-option combination and min_count 0, 2 and 10^6; the launch counts
    of info and of stats_read; sk_upper / sk_lower equal sk(c) byte for byte with NaN in the same places"""
    channels = SELECTIONS[selection]
    bank, mode = state["bank"], state["mode"]
    sel = range(6) if channels is None else channels
    kw = dict(carriers=[state["given"][c] for c in sel]) if state["given"] and mode == "ampm" else {}
    nans = 0
    for opts in all_opts(pkg):
        before = bank.stats_read()["launches"]
        got = host_call(carrierread, mode, bank, channels, opts, frequencies=True, **kw)
        check_rows(got, state["ref"][opts], channels, (state["name"], selection, opts))
        included = any(b.include for c in sel for b in state["ref"][opts][c][2])
        assert got["launches"] == (1 if included or mode == "ampm" else 0), (selection, opts)
        assert bank.stats_read()["launches"] - before == got["launches"]
        lay = carrierread.layout(bank, channels, opts)
        assert lay["lens"] == got["lens"] and lay["breaks"] == got["breaks"] and lay["max_len"] == got["upper"].shape[1]
        if mode == "sides":
            only = carrierread.bank_sides(bank, channels, opts)
            assert "frequencies" not in only and only["lower"].tobytes() == got["lower"].tobytes()
        if mode == "sk":
            for i, c in enumerate(sel):
                su, sl, br = bank.sk(c, opts)
                assert br == got["breaks"][i]
                for key, want in (("sk_upper", su), ("sk_lower", sl)):
                    assert got[key].dtype == np.float64 and got[key][i, :len(want)].tobytes() == want.tobytes(), (selection, opts, c, key)
                    assert np.all(np.isnan(got[key][i, len(want):]))
                nans += int(np.isnan(su).sum())
    if mode == "sk" and selection == "all":
        assert nans > 0  # SHORT (count < 2) and ZEROS (s1 == 0)


def test_the_read_out_changes_nothing(pkg, carrierread, state):
    """psd(c), sk(c), sidebands(c), am_pm(c, A) and am_pm(c) with carrier=None after all of the above equal what they were before
    (byte for byte, Breaks field for field), and those of the twin bank that never saw a bank read-out"""
    bank, twin, mode = state["bank"], state["twin"], state["mode"]
    kw = dict(bands=[(0.0, 0.5)]) if mode != "sk" else {}
    host_call(carrierread, mode, bank, frequencies=True, **kw, **state["kw"])
    for c in range(6):
        for opts in two_opts(pkg):
            a, b, before = bank.psd(c, opts), twin.psd(c, opts), state["ref"][opts][c]
            for k in range(2):
                assert a[k].tobytes() == b[k].tobytes() == before[k].tobytes(), (c, opts, k)
            assert a[2] == b[2] == before[2], (c, opts)
            a, b, before = (own_reads(bank, mode, state["detrend"], c, opts), own_reads(twin, mode, state["detrend"], c, opts),
                            state["own"][opts][c])
            assert len(a) == {"sides": 0, "sk": 1, "ampm": 2 if state["detrend"] or c in (EMPTY, ZEROS) else 3}[mode]
            assert a == b == before, (c, opts)


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


def device_call(torch, carrierread, state, host, channels, opts, keys, **kw):
    """the device form into fresh sentinel tensors for `keys`; returns (result, {key: tensor}, stride)"""
    rows = host["upper"].shape[0]
    stride = host["upper"].shape[1] + 7
    words = dict(OUTS[state["mode"]])
    t = {k: device_tensor(torch, rows, stride, words[k]) for k in keys}
    if state["mode"] == "ampm" and state["given"]:
        sel = range(6) if channels is None else channels
        kw = dict(kw, carriers=[state["given"][c] for c in sel])
    got = device_fn(carrierread, state["mode"])(state["bank"], stride, channels=channels, opts=opts,
                                                **{DEVICE_ARG.get(k, k): v.data_ptr() for k, v in t.items()}, **kw)
    return got, t, stride


@pytest.mark.parametrize("selection", ["all", "subset with a duplicate"])
def test_device_form(pkg, carrierread, state, selection):
    """sentinel-filled tensors: exactly [0, lens[i]) of each asked row is written, all together and each output alone; the carrier
    records alone; a second call gives the same bits"""
    import torch
    channels = SELECTIONS[selection]
    sel = range(6) if channels is None else channels
    words = dict(OUTS[state["mode"]])
    kw = dict(carriers=[state["given"][c] for c in sel]) if state["given"] and state["mode"] == "ampm" else {}
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True)):
        host = host_call(carrierread, state["mode"], state["bank"], channels, opts, frequencies=True, **kw)
        again = host_call(carrierread, state["mode"], state["bank"], channels, opts, frequencies=True, **kw)
        for k in list(words) + (["carrier"] if state["mode"] == "ampm" else []):
            assert host[k].tobytes() == again[k].tobytes(), k
        got, t, stride = device_call(torch, carrierread, state, host, channels, opts, list(words))
        assert got["lens"] == host["lens"] and got["breaks"] == host["breaks"] and got["launches"] == 1
        for k in words:
            check_device_rows(t[k], host[k], host["lens"], stride, words[k], k)
        for k in words:  # each output alone
            got, t, stride = device_call(torch, carrierread, state, host, channels, opts, [k])
            assert got["launches"] == 1
            check_device_rows(t[k], host[k], host["lens"], stride, words[k], k + " alone")
        if state["mode"] == "ampm":
            tc = torch.full((4 * len(sel) + 5,), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            got = carrierread.bank_am_pm_device(state["bank"], 0, carrier=tc.data_ptr(), channels=channels, opts=opts, **kw)
            out = tc.cpu().numpy()
            assert got["launches"] == 1 and out[:4 * len(sel)].tobytes() == host["carrier"].tobytes() and np.all(out[4 * len(sel):] == -7.0)


def test_done_event_form(pkg, carrierread, state):
    """four calls that return early, back to back with different options, each into its own tensors (the two job-table slots are
    reused), waited for through their events: the host form's bytes"""
    import torch
    mode = state["mode"]
    opts = [pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True), pkg.MergeOpts(min_count=2),
            pkg.MergeOpts(keep_transition_band=True)]
    keys = {"sides": ["upper", "lower"], "sk": ["lower", "sk_upper"], "ampm": ["upper", "s_pm"]}[mode]
    words = dict(OUTS[mode])
    host = [host_call(carrierread, mode, state["bank"], None, o, **state["kw"]) for o in opts]
    events = []
    for _ in opts:
        ev = torch.cuda.Event()
        ev.record()  # (the handle exists once the event has been recorded)
        events.append(ev)
    torch.cuda.synchronize()
    calls = [device_call(torch, carrierread, state, h, None, o, keys, done_event=ev.cuda_event)
             for h, o, ev in zip(host, opts, events)]  # back to back, no wait in between
    for k, ((got, t, stride), h, ev) in enumerate(zip(calls, host, events)):
        ev.synchronize()
        assert got["lens"] == h["lens"] and got["launches"] == 1
        for key in keys:
            check_device_rows(t[key], h[key], h["lens"], stride, words[key], f"{key} of call {k} of four back to back")
    unfed = carrierread.bank_sides_device(state["bank"], 4, upper=calls[0][1][keys[0]].data_ptr(), channels=[EMPTY], done_event=events[0].cuda_event)
    events[0].synchronize()  # (recorded even though nothing was launched)
    assert unfed["launches"] == 0


def scale_of(bank, c, opts):
    """(Us + Ls + 2 |comp_s|) of every bin of sidebands(c, opts)"""
    up, lo, comp, _ = bank.sidebands(c, opts)
    return up + lo + 2.0 * np.abs(comp)


def stage_acc(bank, c, breaks):
    """the channel's own f64 stage_rows [ns][4][bins], and the stage counts"""
    stages = [bank.stage_rows(c, s) for s in range(len(breaks))]
    acc = np.array([[up, lo, comp.real, comp.imag] for _, up, lo, comp in stages], np.float64).reshape(len(stages), 4, bank.n // 2 + 1)
    return acc, [st[0]["count"] for st in stages]


def test_am_pm(pkg, carrierread, ampm_state):
    """carriers=None against am_pm(c) and carrier(c), given carriers against am_pm(c, carrier=A): per bin
    |got - want| <= 32 * 2^-53 * (Us + Ls + 2 |comp_s|) / (2 P) -- the two routes differ by hypot against sqrt(re^2 + im^2) and by
    the sqrt(power) sqrt(u) detour squared again in Python, at most about 10 roundings in u and P together, and each adds at most
    5 of its own on the largest term -- and power, u, lock within 8 * 2^-53 relative.  Against tests/carrier_read_ref.py on the
    channel's own stage_rows the expected difference is 0; 2 * 2^-53 of the same scale is allowed for the device's f64 square root
    and division.  ZEROS and EMPTY: the NaN record, NaN rows, upper / lower unaffected."""
    state = ampm_state
    bank, n = state["bank"], state["n"]
    wt = getattr(pkg.WindowTable, state["window"].lower())(n)
    routes = ([None] if not state["detrend"] else []) + [GIVEN]
    if state["detrend"]:
        import torch
        w = carrierread.layout(bank)["max_len"]
        t = device_tensor(torch, 6, w, 2)
        for kw in (dict(s_pm=t.data_ptr()), dict(carrier=t.data_ptr()), dict(bands=[(0.0, 0.5)], band_ptr=t.data_ptr())):
            with pytest.raises(pkg.PsdError) as e:
                carrierread.bank_am_pm_device(bank, w, **kw)
            assert e.value.code == pkg.ERR_ARG and "PSDC_DETREND_NONE" in str(e.value)
        assert np.all(t.cpu().numpy() == SENTINEL)  # (nothing written)
        assert carrierread.bank_am_pm_device(bank, w, upper=t.data_ptr())["launches"] == 1  # (no output that needs the carrier)
    for carriers in routes:
        for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, min_count=0, keep_transition_band=True)):
            got = carrierread.bank_am_pm(bank, None, carriers, opts)
            worst = np.zeros(3)
            equal = True
            for c in range(6):
                ln = got["lens"][c]
                rec = got["carrier"][c]
                assert np.all(np.isnan(got["s_am"][c, ln:])) and np.all(np.isnan(got["s_ampm"][c, ln:]))
                if carriers is None and c in (EMPTY, ZEROS):
                    assert rec[0] == 0.0 and np.all(np.isnan(rec[1:]))
                    assert np.all(np.isnan(got["s_am"][c])) and np.all(np.isnan(got["s_pm"][c])) and np.all(np.isnan(got["s_ampm"][c]))
                    assert got["upper"][c, :ln].tobytes() == state["ref"][opts][c][0].tobytes()
                    continue
                acc, counts = stage_acc(bank, c, got["breaks"][c])
                if carriers is None:
                    power, u, lock = bank.carrier(c)
                    assert abs(rec[0] - power) <= 8 * EPS * power and abs(rec[3] - lock) <= 8 * EPS * lock, (c, rec, power, lock)
                    assert abs(complex(rec[1], rec[2]) - u) <= 8 * EPS * abs(u), (c, rec, u)
                    car = ref.carrier_from_bin0(n, wt.power, counts[0], acc[0, 0, 0], acc[0, 1, 0], acc[0, 2, 0], acc[0, 3, 0])
                    if c == ODD:
                        assert rec[3] < 0.999, rec
                    elif c in (LONG, TWIN):
                        assert rec[3] > 1 - 1e-5, rec
                    want = bank.am_pm(c, None, opts)
                else:
                    assert np.isnan(rec[3])
                    car = ref.carrier_given(carriers[c])
                    if c == EMPTY:
                        assert ln == 0 and rec[:3].tobytes() == np.asarray(car[:3]).tobytes()
                        continue
                    want = bank.am_pm(c, carriers[c], opts)
                assert np.all(np.abs(rec[:3] - np.asarray(car[:3])) <= 2 * EPS * np.maximum(np.abs(car[:3]), 1.0)), (c, rec, car)
                P = rec[0]
                scale = scale_of(bank, c, opts) / (2.0 * P)
                rows, g, _ = ref.placed(acc, got["breaks"][c], n, counts, wt.nenbw, wt.power)
                r_am, r_pm, r_x = ref.split(rows[0], rows[1], rows[2], rows[3], g, *car[:3])
                ok = np.isfinite(scale)  # (a stage without a segment, included by min_count = 0, has no finite scale)
                assert np.array_equal(ok, np.isfinite(got["s_am"][c, :ln])), c
                for k, (key, w, r) in enumerate((("s_am", want[0], r_am), ("s_pm", want[1], r_pm), ("s_ampm", want[2], r_x))):
                    v = got[key][c, :ln]
                    d1, d2 = np.abs(v - w)[ok], np.abs(v - r)[ok]
                    equal = equal and v[ok].tobytes() == r[ok].tobytes()
                    pos = ok & (scale > 0)  # (scale 0: an all-zero stream under given carriers; the differences are 0 there)
                    if pos.any():
                        worst[0] = max(worst[0], float(np.max(np.abs(v - w)[pos] / (EPS * scale[pos]))))
                        worst[1] = max(worst[1], float(np.max(np.abs(v - r)[pos] / (EPS * scale[pos]))))
                    assert np.all(d1 <= 32 * EPS * scale[ok]), (c, key, worst)
                    assert np.all(d2 <= 2 * EPS * scale[ok]), (c, key, worst)
            print(state["name"], "given" if carriers else "bin 0", opts.keep_overlap, "worst in 2^-53 of the scale: against am_pm()", worst[0],
                  "against the restatement", worst[1], "byte-equal" if equal else "not byte-equal")


def test_physics(pkg, carrierread, own_carrier_state):
    """LONG: the AM tone's bin (offset 1/8) shows in s_am and not in s_pm, the PM tone's bin (offset 3/16) the reverse, the wrong one
    below 1e-3 of the right one; the band around the PM tone integrates to the tone's mean-square phase A_PM^2 / 2 = 2e-4 rad^2.
    (The tones sit on bin centres of stage 0, where the Hann and rectangular windows put all of a line's power into the bins the
    band holds, and the trapezoid of equally spaced bins is their sum: the small-angle split errs by A_PM^2 / 8 relative, the noise
    floor and the AM tone's second harmonic of phase by less than 1e-4: 1 % is the resolution asked of the integral.  The band's
    lower edge lies two bins above the AM tone's Hann skirt at n = 64, so its s_am sum holds none of that tone.  Measured: 2.0008e-4 on
    the IQ bank, 2.0105e-4 ... 2.0121e-4 on the zoom banks; the band around the AM tone reads 5.05e-5 ... 5.06e-5 against
    A_AM^2 / 2 = 5e-5 and is printed, not asserted: am_pm(c) carries the same excess.)"""
    state = own_carrier_state
    got = carrierread.bank_am_pm(state["bank"], [LONG], None, pkg.MergeOpts(), frequencies=True, bands=[(0.16, 0.22), (0.09, 0.16)])
    f = got["frequencies"][0, :got["lens"][0]]
    k_am, k_pm = int(np.argmin(np.abs(f - F_AM))), int(np.argmin(np.abs(f - F_PM)))
    assert f[k_am] == np.float32(F_AM) and f[k_pm] == np.float32(F_PM)
    s_am, s_pm = got["s_am"][0], got["s_pm"][0]
    print(state["name"], "AM bin", s_am[k_am], s_pm[k_am], "PM bin", s_am[k_pm], s_pm[k_pm], "band", got["band_sums"][0])
    assert s_pm[k_am] < 1e-3 * s_am[k_am] and s_am[k_pm] < 1e-3 * s_pm[k_pm]
    assert abs(got["band_sums"][0, 0, 3] - A_PM ** 2 / 2) <= 0.01 * A_PM ** 2 / 2
    # (the band around the AM tone, A_AM^2 / 2 = 5e-5 from the generator, is printed above and not asserted: DESIGN.md has the readings)
    assert got["band_sums"][0, 0, 2] < 1e-3 * got["band_sums"][0, 0, 3]


def bands_of():
    """the whole range; most of stage 0; a decade across a seam; a single bin (k = n/4 of stage 0); none"""
    return [(0.0, 0.5), (0.0501, 0.5), (0.01, 0.1), (0.25, 0.25), (0.30001, 0.30002)]


def test_band_sums(pkg, carrierread, state, tmp_path_factory):
    """Within the summation bound of numpy's trapezoids on the read-out's own rows (upper and lower: the f32 rows; s_am and s_pm:
    the f64 rows); the same bits from a second call, from bands alone (one launch) and from the device form; and, for the objects
    whose stage rows can be read in f64 (SK and AM/PM), the bits of carrier_band_*_host (csrc/carrier_readout.h run on the CPU by
    tests/host/carrier_readout_check.cpp) on the channel's own stage rows and Breaks"""
    import torch
    from test_bank_readout_host import band_reference
    from test_waterfall_host import host_exe
    if state["mode"] == "sk":  # (the SK call has no bands: the sides call takes an SK object)
        call, dev, width, kw = carrierread.bank_sides, carrierread.bank_sides_device, 2, {}
    else:
        call = carrierread.bank_sides if state["mode"] == "sides" else carrierread.bank_am_pm
        dev, width, kw = device_fn(carrierread, state["mode"]), 2 if state["mode"] == "sides" else 4, state["kw"]
    bank, bands, n = state["bank"], bands_of(), state["n"]
    wt = getattr(pkg.WindowTable, state["window"].lower())(n)
    d = tmp_path_factory.mktemp("carrier_band_bits")
    exe = host_exe(d, "carrier_readout_check", False)
    nonzero = 0
    for opts in (pkg.MergeOpts(), pkg.MergeOpts(keep_overlap=True, keep_transition_band=True)):
        got = call(bank, None, opts=opts, frequencies=True, bands=bands, **kw)
        assert got["launches"] == 2 and got["band_sums"].shape == (6, len(bands), width) and got["band_sums"].dtype == np.float64
        blob = []
        for c in range(6):
            ln = got["lens"][c]
            rows = [got["upper"][c, :ln], got["lower"][c, :ln]] + ([got["s_am"][c, :ln], got["s_pm"][c, :ln]] if width == 4 else [])
            freq = got["frequencies"][c, :ln]
            for r, row in enumerate(rows):
                if not np.all(np.isfinite(row)):  # (ZEROS: no carrier, NaN rows and NaN sums where a band holds a bin)
                    assert c == ZEROS and r >= 2 and np.isnan(got["band_sums"][c, 0, r]) and got["band_sums"][c, 4, r] == 0.0
                    continue
                for b, (want, tol, count) in enumerate(band_reference(np.ascontiguousarray(row), freq, bands)):
                    assert abs(got["band_sums"][c, b, r] - want) <= tol, (c, b, r, got["band_sums"][c, b, r], want, tol)
                    if count == 0:
                        assert got["band_sums"][c, b, r] == 0.0
            nonzero += int(np.count_nonzero(np.nan_to_num(got["band_sums"][c])))
            breaks = got["breaks"][c]
            if state["mode"] == "sides":
                continue
            if state["mode"] == "sk":
                stages = [bank.stage_moments(c, s) for s in range(len(breaks))]
                acc = np.array([st[1:3] for st in stages], np.float64).reshape(len(stages), 2, n // 2 + 1)
            else:
                acc, _ = stage_acc(bank, c, breaks)
                stages = [bank.stage_rows(c, s) for s in range(len(breaks))]
            counts = [st[0]["count"] for st in stages]
            assert [b.count for b in breaks[::-1]] == counts
            given = state["given"][c] if state["given"] else 0j
            blob.append(struct.pack("<7I2f2d", n, len(stages), len(breaks), len(bands), 0 if width == 2 else 2, int(bool(state["given"])),
                                    counts[0] if counts else 0, wt.nenbw, wt.power, given.real, given.imag))
            blob.append(np.asarray(counts, np.uint64).tobytes())
            blob += [bytes(b._c()) for b in breaks]
            blob.append(acc.tobytes())
            blob.append(np.asarray(bands, np.float32).tobytes())
        assert np.all(got["band_sums"][EMPTY] == 0.0) and np.all(got["band_sums"][ZEROS, :, :2] == 0.0)
        if blob:
            src, dst = str(d / "cases.bin"), str(d / "rows.bin")
            with open(src, "wb") as f:
                f.write(struct.pack("<I", 6) + b"".join(blob))
            r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
            raw, pos = open(dst, "rb").read(), 0
            for c in range(6):
                ln = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
                assert ln == got["lens"][c]
                assert raw[pos + 8:pos + 8 + 4 * ln] == got["upper"][c, :ln].tobytes()
                assert raw[pos + 8 + 8 * ln:pos + 8 + 12 * ln] == got["frequencies"][c, :ln].tobytes()
                pos += 8 + 12 * ln + (32 * ln + 32 if width == 4 else 0)
                host = np.frombuffer(raw, np.float64, width * len(bands), pos).reshape(len(bands), width)
                print(state["name"], opts.keep_overlap, "channel", c, "device", got["band_sums"][c, 0], "host", host[0])
                nan = np.isnan(host)  # (ZEROS: the sign and payload of a NaN are not part of the result)
                assert np.array_equal(nan, np.isnan(got["band_sums"][c])) and (c == ZEROS or not nan.any())
                assert host[~nan].tobytes() == got["band_sums"][c][~nan].tobytes(), (c, host, got["band_sums"][c])
                pos += 8 * width * len(bands)
            assert pos == len(raw)
        # the same bits from a second call, from bands alone, and from the device form with a row
        again = call(bank, None, opts=opts, bands=bands, **kw)
        assert again["band_sums"].tobytes() == got["band_sums"].tobytes()
        count = 6 * len(bands) * width
        tb = torch.full((count + 3,), -1.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        alone = dev(bank, 0, opts=opts, bands=bands, band_ptr=tb.data_ptr(), **kw)
        assert alone["launches"] == 1
        out = tb.cpu().numpy()
        assert out[:count].tobytes() == got["band_sums"].tobytes() and np.all(out[count:] == -1.0)
        tb.fill_(-1.0)
        stride = got["upper"].shape[1] + 3
        tu = device_tensor(torch, 6, stride)
        both = dev(bank, stride, upper=tu.data_ptr(), opts=opts, bands=bands, band_ptr=tb.data_ptr(), **kw)
        assert both["launches"] == 2 and tb.cpu().numpy()[:count].tobytes() == got["band_sums"].tobytes()
        check_device_rows(tu, got["upper"], got["lens"], stride, 1, "upper with bands")
    assert nonzero >= 2 * 3 * 4 * 2  # at least three fed channels, four bands that hold bins, two rows that are not zero
    # the unfed channel alone: nothing is launched without a carrier record, the band sums are 0.0
    tb = torch.full((len(bands) * 2,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    unfed = carrierread.bank_sides_device(bank, 0, channels=[EMPTY], bands=bands, band_ptr=tb.data_ptr())
    assert unfed["launches"] == 0 and np.all(tb.cpu().numpy() == 0.0)
    alone = carrierread.bank_sides(bank, [EMPTY], bands=bands)
    assert alone["launches"] == 0 and alone["upper"].shape == (1, 0) and np.all(alone["band_sums"] == 0.0)


@pytest.mark.parametrize("mode", ["sides", "sk", "ampm"])
def test_seventy_channels_in_one_launch(pkg, carrierread, gpu_required, mode):
    """a bank of 70 channels of which 3 are fed, all 70 selected: one launch (jobs run along x), two with bands; the single-channel
    object goes through the same call; release() and the next call"""
    bank = getattr(pkg, CLASSES["zoom", mode])(64, 70)
    fed = (3, 40, 69)
    for c in fed:
        bank.set_carrier(c, f0=F0)
        bank.process(c, stream(pkg, False, 3000 + c, c))
    kw = dict(bands=[(0.0, 0.5), (0.01, 0.1)]) if mode != "sk" else {}
    got = host_call(carrierread, mode, bank, frequencies=True, **kw)
    assert got["launches"] == (2 if kw else 1) and host_call(carrierread, mode, bank)["launches"] == 1
    for c in range(70):
        up, lo, br = bank.psd(c)
        assert got["lens"][c] == len(up) and got["breaks"][c] == br
        assert got["upper"][c, :len(up)].tobytes() == up.tobytes() and got["lower"][c, :len(up)].tobytes() == lo.tobytes()
        assert (len(up) > 0) == (c in fed)
        if c not in fed and kw:
            assert np.all(got["band_sums"][c] == 0.0)
        if mode == "ampm":
            assert (got["carrier"][c, 0] > 0) == (c in fed) and np.isnan(got["carrier"][c, 1]) == (c not in fed)
    sel = list(range(69, -1, -1)) * 2
    twice = host_call(carrierread, mode, bank, sel)
    assert twice["launches"] == 1 and twice["upper"].shape[0] == 140
    assert twice["lower"][0].tobytes() == got["lower"][69].tobytes() and twice["lower"][70 + 29].tobytes() == got["lower"][40].tobytes()
    carrierread.release(bank)  # the buffers come back with the next call
    assert host_call(carrierread, mode, bank)["upper"].tobytes() == got["upper"].tobytes()
    single = getattr(pkg, CLASSES["zoom", mode][:-4])(64, f0=F0)
    single.process(stream(pkg, False, 3003, 3))
    one = host_call(carrierread, mode, single)
    assert one["upper"][0].tobytes() == got["upper"][3, :one["lens"][0]].tobytes() == single.psd()[0].tobytes()
    single.close()
    bank.close()


def test_errors(pkg, carrierread, state):
    import torch
    bank, mode = state["bank"], state["mode"]
    L = carrierread._lib()
    lay = carrierread.layout(bank)
    stride = lay["max_len"] - 1
    t = device_tensor(torch, 6, lay["max_len"], 4)
    c = carrierread._Call(bank, None, None, ("sides", "sk", "ampm"))
    rc = L.psdczr_sides_device(*c.head, None, C.c_void_p(t.data_ptr()), None, stride, None, 0, None, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and "stride" in bank._f("last_error")(bank._h).decode()
    assert c.result()["lens"] == lay["lens"] and int(c.info.max_len) == lay["max_len"] and int(c.info.launches) == 0
    assert np.all(t.cpu().numpy() == SENTINEL)
    host = np.zeros((6, lay["max_len"]), np.float32)
    c = carrierread._Call(bank, None, None, ("sides", "sk", "ampm"))
    rc = L.psdczr_sides(*c.head, host.ctypes.data, None, None, stride, None, 0, None, *c.tail)
    assert rc == pkg.ERR_CAPACITY and c.result()["lens"] == lay["lens"] and np.all(host == 0)
    c = carrierread._Call(bank, None, None, ("sides", "sk", "ampm"))  # room for fewer breaks than channel 0 has, then a retry
    rc = L.psdczr_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, 2, C.byref(c.info))
    assert rc == pkg.ERR_CAPACITY and [int(v) for v in c.lens] == lay["lens"] and int(c.nb[0]) == len(lay["breaks"][0]) > 2
    rc = L.psdczr_layout(*c.head, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, int(c.nb.max()), C.byref(c.info))
    assert rc == 0

    def arg_error(text, fn, *args, **kw):
        with pytest.raises(pkg.PsdError) as e:
            fn(bank, *args, **kw)
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))

    ptr, width = t.data_ptr(), lay["max_len"]
    arg_error("out of range", carrierread.bank_sides, [0, 6])
    arg_error("out of range", carrierread.layout, [6])
    arg_error("out of range", carrierread.bank_sides_device, width, upper=ptr, channels=[7])
    arg_error("more than 8 bands", carrierread.bank_sides_device, width, upper=ptr, bands=[(0.0, 0.1)] * 9, band_ptr=ptr)
    arg_error("bands without a band output", carrierread.bank_sides_device, width, upper=ptr, bands=[(0.0, 0.1)])
    arg_error("a band output without bands", carrierread.bank_sides_device, width, upper=ptr, band_ptr=ptr)
    arg_error("a band with NaN or lo > hi", carrierread.bank_sides, bands=[(0.0, 0.1), (float("nan"), 0.2)])
    arg_error("a band with NaN or lo > hi", carrierread.bank_sides, bands=[(0.2, 0.1)])
    arg_error("no output", carrierread.bank_sides_device, width)
    if mode != "sk":
        arg_error("takes a ZoomSkCascade", carrierread.bank_sk)
    if mode != "ampm":
        arg_error("takes a ZoomAmPmCascade", carrierread.bank_am_pm)
    else:
        arg_error("finite and not 0", carrierread.bank_am_pm, None, [0.5, 0.5, 0j, 0.5, 0.5, 0.5])
        arg_error("finite and not 0", carrierread.bank_am_pm_device, width, s_am=ptr, carriers=[0.5, float("nan"), 1, 1, 1, float("inf")])
        arg_error("one complex amplitude", carrierread.bank_am_pm, None, [0.5])
    # the C calls look at the object's kind themselves
    c = carrierread._Call(bank, None, None, ("sides", "sk", "ampm"))
    if mode != "sk":
        rc = L.psdczr_sk_device(*c.head, C.c_void_p(ptr), None, None, None, None, width, None, *c.tail)
        assert rc == pkg.ERR_ARG and bank._f("last_error")(bank._h).decode() == "psdczr_sk_device: takes a zoom SK or IQ SK object"
    if mode != "ampm":
        rc = L.psdczr_ampm(*c.head, None, host.ctypes.data, None, None, None, None, None, None, width, None, 0, None, *c.tail)
        assert rc == pkg.ERR_ARG and bank._f("last_error")(bank._h).decode() == "psdczr_ampm: takes a zoom AM/PM or IQ AM/PM object"
    rc = L.psdczr_layout(*c.head, None, c.nb.ctypes.data, None, 0, None)
    assert rc == pkg.ERR_ARG and bank._f("last_error")(bank._h).decode() == "psdczr_layout: null lens"
    rc = L.psdczr_layout(*c.head, c.lens.ctypes.data, None, c.br.ctypes.data, 16, None)
    assert rc == pkg.ERR_ARG and bank._f("last_error")(bank._h).decode() == "psdczr_layout: breaks without n_breaks"
    assert np.all(t.cpu().numpy() == SENTINEL) and np.all(host == 0)
    other = pkg.CsdCascadeBank(64, 2)  # another object of the same runtime: the binding refuses it, and so does the C call
    for fn in (carrierread.layout, carrierread.bank_sides, carrierread.bank_sk, carrierread.bank_am_pm):
        with pytest.raises(pkg.PsdError) as e:
            fn(other)
        assert e.value.code == pkg.ERR_ARG
    lens = np.full(2, 55, np.uintp)
    rc = L.psdczr_layout(other._h, None, 0, 0, 1, 0, lens.ctypes.data, None, None, 0, None)
    assert rc == pkg.ERR_ARG and "takes a zoom, IQ" in pkg.lib().psdc_cross_last_error(other._h).decode() and np.all(lens == 55)
    other.close()
    before = host_call(carrierread, mode, bank, **state["kw"])
    carrierread.release(bank)
    carrierread.release(bank)
    after = host_call(carrierread, mode, bank, **state["kw"])  # the buffers are made again
    assert after["upper"].tobytes() == before["upper"].tobytes() and after["lower"].tobytes() == before["lower"].tobytes()
