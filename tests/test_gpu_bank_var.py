"""Var read-out on the MI355X (include/psdcascade_var.h, psdcv_*; stabilizer-stream_amd/bankvar.py): one call gives the AVAR / MVAR /
FVAR curves of every selected channel of a PsdCascadeBank from its accumulators.  Every value is held to the numpy f64 restatement
of the definition (tests/bank_var_ref.py) on the rows that psd(c) and Break.frequencies return, within (L + 64) 2^-52 sum |t|, NaN
exactly where the restatement gives NaN; the host form, the device form, a second call and the rows form on the output of
bank_psd_device give the same bytes.

Shapes: the two smallest of tests/test_gpu_bank_readout.py -- n = 64 (generic kernels) and n = 1024 (fused kernels), a bank of five
channels: three or more stages, an odd length, one stage of one or two segments, never fed, and one with half a call in host
staging when the first read-out is made."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import bank_var_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25  # what the device outputs are pre-filled with (a variance is >= 0 or NaN)
# name: (n, samples of channels 0 and 4, of channel 1, of channel 2)
SHAPES = {"n64": (64, 1 << 14, 5000, 100), "n1024": (1024, 1 << 18, 5000 * 16, 1600)}
EMPTY = 3  # the channel that is never fed
SELECTIONS = {"all": None, "permutation": [4, 2, 0, 3, 1], "subset with a duplicate": [1, 4, 1], "the empty channel alone": [EMPTY]}
TAUS = [0.5, 1, 2.7, 64, 1e3, 1e6, 3e7]  # lim = inf, a cut inside every stage, no term at all
TILE = 4  # VAR_TAU_TILE of csrc/bank_var.h


def all_opts(pkg):
    return [pkg.MergeOpts(keep_overlap=ko, min_count=mc, keep_transition_band=ktb)
            for ko, ktb, mc in itertools.product((False, True), (False, True), (0, 2))]


@pytest.fixture(scope="module")
def bankvar(pkg):
    from stabilizer_stream_amd import bankvar as mod
    return mod


def as_dict(v):
    return dict(x_exp=v.x_exp, sinx_exp=v.sinx_exp, clip=v.clip, dc_cut=v.dc_cut)


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request, pkg, bankvar, gpu_required):
    """one fed bank a shape: dict(bank, first, rows, want).  `first` is the Var read-out made while channel 4 had half a call in host
    staging; rows[opts] = [(psd, breaks, frequencies)] of every channel from psd(c), computed once; want(opts, c, var, tau) is the
    restatement on those rows, computed once a key"""
    n, long, mid, short = SHAPES[request.param]
    bank = pkg.PsdCascadeBank(n, 5)
    x = pkg.noise_host(long, seed=1000 + n)
    piece = long // 4
    for k in range(4):
        bank.process(0, x[k * piece:(k + 1) * piece])
    for part in np.array_split(pkg.noise_host(mid, seed=2000 + n), 3):
        bank.process(1, part)
    bank.process(2, pkg.noise_host(short, seed=3000 + n))
    for k in range(3):
        bank.process(4, x[k * piece:(k + 1) * piece])
    bank.process(4, x[3 * piece:3 * piece + piece // 2])
    bank.flush()
    bank.process(4, x[3 * piece + piece // 2:])  # half a call: in host staging when the read-out below is made
    first = bankvar.bank_var(bank, TAUS)
    rows = {}
    for opts in all_opts(pkg) + [pkg.MergeOpts()]:
        rows[opts] = [(p, br, pkg.Break.frequencies(br)) for p, br in (bank.psd(c, opts) for c in range(5))]
    cache = {}

    def want(opts, c, var, tau):
        key = (opts, c, var, float(np.float32(tau)))
        if key not in cache:
            p, _, f = rows[opts][c]
            cache[key] = ref.var_ref(p, f, tau, **as_dict(var))
        return cache[key]

    yield dict(bank=bank, first=first, rows=rows, want=want, n=n, name=request.param)
    bank.close()


def check(state, got, opts, channels, vs, taus, what):
    """got: float64 [S][V][T] against the restatement; returns the largest |error| / tolerance"""
    sel = range(5) if channels is None else channels
    assert got.dtype == np.float64 and got.shape == (len(sel), len(vs), len(taus)), what
    worst = 0.0
    for i, c in enumerate(sel):
        L = len(state["rows"][opts][c][0])
        for v, var in enumerate(vs):
            for j, tau in enumerate(taus):
                w, sum_abs, E = state["want"](opts, c, var, tau)
                g = got[i, v, j]
                if np.isnan(w) or np.isnan(g):
                    assert np.isnan(w) and np.isnan(g), (what, c, var, tau, g, w)
                    continue
                tol = ref.tolerance(L, sum_abs)
                assert abs(g - w) <= tol, (what, c, var, tau, g, w, tol, E)
                if E <= var.dc_cut:
                    assert g == 0.0, (what, c, var, tau)
                worst = max(worst, abs(g - w) / tol if tol else 0.0)
    return worst


def three(bankvar):
    return [bankvar.Var.avar(), bankvar.Var.mvar(), bankvar.Var.fvar()]


def test_shape_is_what_the_cases_need(pkg, state):
    rows = state["rows"][pkg.MergeOpts()]
    live = [sum(b.count > 0 for b in br) for _, br, _ in rows]
    assert live[0] >= 3 and live[4] == live[0] and live[1] >= 2 and live[2] == 1 and live[EMPTY] == 0 and not rows[EMPTY][1], live
    # the taus do what they are there for on channel 0: no limit, a cut inside every stage, no term at all
    p, br, f = rows[0]
    cuts = [ref.limit(f, t, 1.0, 2) for t in TAUS]
    assert cuts[0] == cuts[1] == len(p) and cuts[-1] == 2 and len(set(cuts)) >= 5, cuts


def test_first_read_out_with_samples_in_host_staging(pkg, bankvar, state):
    got = state["first"]
    assert got["launches"] == 1 and got["var"].shape == (5, len(TAUS))
    rows = state["rows"][pkg.MergeOpts()]
    assert got["lens"] == [len(p) for p, _, _ in rows] and list(got["breaks"]) == [br for _, br, _ in rows]
    check(state, got["var"][:, None, :], pkg.MergeOpts(), None, [bankvar.Var()], TAUS, "first read-out")


@pytest.mark.parametrize("selection", list(SELECTIONS))
def test_bank_form(pkg, bankvar, state, selection):
    """all eight keep_overlap x keep_transition_band x min_count combinations, AVAR + MVAR + FVAR in one call"""
    channels = SELECTIONS[selection]
    sel = range(5) if channels is None else channels
    worst = 0.0
    for opts in all_opts(pkg):
        got = bankvar.bank_var(state["bank"], TAUS, three(bankvar), channels, opts)
        rows = state["rows"][opts]
        assert got["lens"] == [len(rows[c][0]) for c in sel] and list(got["breaks"]) == [rows[c][1] for c in sel], (selection, opts)
        included = any(b.include for c in sel for b in rows[c][1])
        assert got["launches"] == (1 if included else 0), (selection, opts)
        worst = max(worst, check(state, got["var"], opts, channels, three(bankvar), TAUS, (state["name"], selection, opts)))
        for i, c in enumerate(sel):
            if c == EMPTY:
                assert np.all(got["var"][i] == 0.0) and not np.any(np.signbit(got["var"][i]))
    print(state["name"], selection, "largest |error| / tolerance", worst)
    if channels == [EMPTY]:
        assert got["launches"] == 0 and got["var"].shape == (1, 3, len(TAUS))


def test_descriptors(pkg, bankvar, state):
    """AVAR, MVAR, FVAR singly give the bytes they have in the call of all three; dc_cut 0, 1, 2, L and L + 5"""
    bank, opts = state["bank"], pkg.MergeOpts()
    all3 = bankvar.bank_var(bank, TAUS, three(bankvar))["var"]
    for v, var in enumerate(three(bankvar)):
        one = bankvar.bank_var(bank, TAUS, var)
        assert one["var"].shape == (5, len(TAUS)) and one["launches"] == 1
        assert one["var"].tobytes() == all3[:, v, :].tobytes(), var
        check(state, one["var"][:, None, :], opts, None, [var], TAUS, var)
    L = len(state["rows"][opts][0][0])
    cuts = [bankvar.Var(dc_cut=d) for d in (0, 1, 2, L, L + 5)]
    got = np.concatenate([bankvar.bank_var(bank, TAUS, cuts[:4])["var"], bankvar.bank_var(bank, TAUS, cuts[4:])["var"]], axis=1)
    check(state, got, opts, None, cuts, TAUS, "dc_cut")
    assert np.all(np.isnan(got[0, 0])) and np.all(got[0, 3:] == 0.0) and np.all(got[0, 2, :-1] > 0.0)  # f[0] = 0: 0 * inf
    assert got[:, 2, :].tobytes() == all3[:, 0, :].tobytes()
    others = [bankvar.Var(3, 1, bankvar.FLT_MAX, 1), bankvar.Var(-16, 16, 1e-3, 4), bankvar.Var(0, 0, -1.0, 0), bankvar.Var(1, 2)]
    mixed = bankvar.bank_var(bank, TAUS, others)
    check(state, mixed["var"], opts, None, others, TAUS, "other exponents and clips")
    w, sum_abs, _ = state["want"](opts, 0, others[0], TAUS[2])
    assert abs(w) < 0.999 * sum_abs  # an odd power of the sine: terms of both signs
    assert np.all(mixed["var"][:, 2, :] == 0.0)  # a negative clip: nothing is included


def test_tau_counts(pkg, bankvar, state):
    """T = 1, T one above a multiple of the tau tile, and on n64 T = 4096"""
    for count in [1, 2 * TILE + 1] + ([4096] if state["name"] == "n64" else []):
        taus = np.logspace(-0.3, 7.5, count).astype(np.float32) if count > 1 else np.asarray([2.7], np.float32)
        vs = three(bankvar) if count < 4096 else [bankvar.Var.avar()]
        got = bankvar.bank_var(state["bank"], taus, vs)
        assert got["launches"] == 1
        print(state["name"], "T", count, "largest |error| / tolerance", check(state, got["var"], pkg.MergeOpts(), None, vs, taus, ("T", count)))


def device_out(torch, count, tail=5):
    t = torch.full((count + tail,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def test_forms_agree_and_nothing_else_is_written(pkg, bankvar, state):
    """host form = device form = a second call, byte for byte; the device form writes [S][V][T] and nothing behind it"""
    import torch
    bank, vs = state["bank"], three(bankvar)
    for channels, opts in ((None, pkg.MergeOpts()), ([1, 4, 1], pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True)),
                           ([EMPTY], pkg.MergeOpts())):
        S = 5 if channels is None else len(channels)
        host = bankvar.bank_var(bank, TAUS, vs, channels, opts)
        again = bankvar.bank_var(bank, TAUS, vs, channels, opts)
        assert host["var"].tobytes() == again["var"].tobytes()
        count = S * len(vs) * len(TAUS)
        t = device_out(torch, count)
        dev = bankvar.bank_var_device(bank, t.data_ptr(), TAUS, vs, channels, opts)
        out = t.cpu().numpy()
        assert out[:count].tobytes() == host["var"].tobytes(), (channels, opts)
        assert np.all(out[count:] == SENTINEL)
        assert dev["lens"] == host["lens"] and dev["breaks"] == host["breaks"] and dev["launches"] == host["launches"] == (0 if channels == [EMPTY] else 1)
        if channels == [EMPTY]:
            assert np.all(out[:count] == 0.0)
    # a T beside the tile, one descriptor: the last tile stores one tau
    taus = np.logspace(0, 5, 3 * TILE + 1)
    host = bankvar.bank_var(bank, taus)
    t = device_out(torch, host["var"].size)
    bankvar.bank_var_device(bank, t.data_ptr(), taus)
    out = t.cpu().numpy()
    assert out[:host["var"].size].tobytes() == host["var"].tobytes() and np.all(out[host["var"].size:] == SENTINEL)


def test_done_event_form(pkg, bankvar, state):
    """the call that returns early: two back to back into tensors of their own (the two table slots), then a third (a slot reused)"""
    import torch
    bank = state["bank"]
    args = [(three(bankvar), pkg.MergeOpts()), ([bankvar.Var.mvar()], pkg.MergeOpts(keep_overlap=True, min_count=0)),
            ([bankvar.Var.fvar(), bankvar.Var.avar(1)], pkg.MergeOpts(min_count=2))]
    host = [bankvar.bank_var(bank, TAUS, vs, None, o)["var"] for vs, o in args]
    tensors = [device_out(torch, h.size) for h in host]
    events = []
    for _ in args:
        ev = torch.cuda.Event()
        ev.record()  # (the handle exists once the event has been recorded)
        events.append(ev)
    torch.cuda.synchronize()
    for t, (vs, o), ev in zip(tensors, args, events):  # back to back, no wait in between
        got = bankvar.bank_var_device(bank, t.data_ptr(), TAUS, vs, None, o, done_event=ev.cuda_event)
        assert got["launches"] == 1
    for k, (t, h, ev) in enumerate(zip(tensors, host, events)):
        ev.synchronize()
        out = t.cpu().numpy()
        assert out[:h.size].tobytes() == h.tobytes() and np.all(out[h.size:] == SENTINEL), f"call {k} of three back to back"


def test_rows_form_on_the_bank_read_out(pkg, bankvar, state):
    """rows_var_device on what bank_psd_device(frequencies) of the same handle left on the device, chained by the stream alone (both
    calls return early; one event at the end): bank_var_device's bytes.  Then the reference's five-element vector, uploaded"""
    import torch
    from stabilizer_stream_amd import bankread
    bank, vs = state["bank"], three(bankvar)
    for channels, opts in ((None, pkg.MergeOpts()), ([4, 2, 0, 3, 1], pkg.MergeOpts(keep_overlap=True, min_count=2, keep_transition_band=True))):
        S = 5
        want = bankvar.bank_var(bank, TAUS, vs, channels, opts)
        stride = max(want["lens"]) + 3
        tp = torch.full((S, stride), float("nan"), dtype=torch.float32, device="cuda")
        tf = torch.full((S, stride), float("nan"), dtype=torch.float32, device="cuda")
        count = want["var"].size
        t = device_out(torch, count)
        e1, e2 = torch.cuda.Event(), torch.cuda.Event()
        e1.record()
        e2.record()
        torch.cuda.synchronize()
        lay = bankread.bank_psd_device(bank, tp.data_ptr(), stride, channels, opts, freq_ptr=tf.data_ptr(), done_event=e1.cuda_event)
        got = bankvar.rows_var_device(bank, tp.data_ptr(), tf.data_ptr(), stride, lay["lens"], TAUS, t.data_ptr(), vs, done_event=e2.cuda_event)
        e2.synchronize()
        assert got["launches"] == 1 and lay["lens"] == want["lens"]
        out = t.cpu().numpy()
        assert out[:count].tobytes() == want["var"].tobytes(), (channels, opts)
        assert np.all(out[count:] == SENTINEL)
    tp = torch.tensor(ref.REF_P, dtype=torch.float32, device="cuda")
    tf = torch.tensor(ref.REF_F, dtype=torch.float32, device="cuda")
    t = device_out(torch, 2)
    torch.cuda.synchronize()
    assert bankvar.rows_var_device(bank, tp.data_ptr(), tf.data_ptr(), 5, [5], [ref.REF_TAU], t.data_ptr(), [bankvar.Var(), bankvar.Var(dc_cut=0)])["launches"] == 1
    out = t.cpu().numpy()
    w, sum_abs, _ = ref.var_ref(ref.REF_P, ref.REF_F, ref.REF_TAU)
    print("the reference's vector:", out[0], "restatement", w)
    assert abs(out[0] - ref.REF_F64) <= 1e-9 and abs(out[0] - w) <= ref.tolerance(5, sum_abs) and np.isnan(out[1])
    # rows of length 0, and no row at all
    t = device_out(torch, 2)
    assert bankvar.rows_var_device(bank, tp.data_ptr(), tf.data_ptr(), 5, [0, 0], [1.0], t.data_ptr())["launches"] == 1
    assert np.all(t.cpu().numpy()[:2] == 0.0)
    assert bankvar.rows_var_device(bank, tp.data_ptr(), tf.data_ptr(), 5, [], [1.0], t.data_ptr())["launches"] == 0


def test_errors(pkg, bankvar, state):
    import torch
    from stabilizer_stream_amd import bankread
    bank = state["bank"]
    L = bankvar._lib()
    t = device_out(torch, 64)
    ptr = t.data_ptr()
    before = bankvar.bank_var(bank, TAUS)["var"].tobytes()

    def arg_error(text, fn, *args, **kw):
        with pytest.raises(pkg.PsdError) as e:
            fn(bank, *args, **kw)
        assert e.value.code == pkg.ERR_ARG and text in str(e.value), (text, str(e.value))

    V = bankvar.Var
    for fn, lead in ((bankvar.bank_var, ()), (bankvar.bank_var_device, (ptr,))):
        arg_error("n_vars must be 1 ... 4", fn, *lead, TAUS, [])
        arg_error("n_vars must be 1 ... 4", fn, *lead, TAUS, [V()] * 5)
        arg_error("n_taus must be 1 ... 4096", fn, *lead, [])
        arg_error("n_taus must be 1 ... 4096", fn, *lead, np.ones(4097))
        arg_error("an exponent beyond +-16", fn, *lead, TAUS, V(x_exp=17))
        arg_error("an exponent beyond +-16", fn, *lead, TAUS, [V(), V(sinx_exp=-17)])
        arg_error("a NaN clip", fn, *lead, TAUS, V(clip=float("nan")))
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            arg_error("a tau that is NaN, infinite or <= 0", fn, *lead, [1.0, bad])
        arg_error("channel out of range", fn, *lead, TAUS, None, [0, 5])
    arg_error("null output", bankvar.bank_var_device, None, TAUS)
    rows = (ptr, ptr, 8)
    arg_error("a row longer than the stride", bankvar.rows_var_device, *rows, [8, 9], TAUS, ptr)
    arg_error("more than PSDCR_MAX_ROWS rows", bankvar.rows_var_device, *rows, [1] * 65537, TAUS, ptr)
    arg_error("null rows", bankvar.rows_var_device, None, ptr, 8, [1], TAUS, ptr)
    arg_error("null rows", bankvar.rows_var_device, ptr, None, 8, [1], TAUS, ptr)
    arg_error("null output", bankvar.rows_var_device, *rows, [1], TAUS, None)
    arg_error("n_vars must be 1 ... 4", bankvar.rows_var_device, *rows, [1], TAUS, ptr, [])
    arg_error("n_taus must be 1 ... 4096", bankvar.rows_var_device, *rows, [1], [], ptr)
    arg_error("a tau that is NaN, infinite or <= 0", bankvar.rows_var_device, *rows, [1], [0.0], ptr)
    arg_error("an exponent beyond +-16", bankvar.rows_var_device, *rows, [1], TAUS, ptr, V(x_exp=-17))
    arg_error("a NaN clip", bankvar.rows_var_device, *rows, [1], TAUS, ptr, V(clip=float("nan")))
    # NULL vars, taus and lens through the C interface; a breaks_cap that is too small
    rec, nv, taus, nt, _ = bankvar._what(None, TAUS)
    out = np.full(5 * nt, SENTINEL)
    for what, text in (((None, nv, taus.ctypes.data, nt), "null vars"), ((rec.ctypes.data, nv, None, nt), "null taus")):
        c = bankread._Call(bank, None, None)
        assert L.psdcv_bank_var(*c.head, *what, out.ctypes.data, *c.tail) == pkg.ERR_ARG
        assert pkg.lib().psdc_last_error(bank._h).decode() == "psdcv_bank_var: " + text
        c = bankread._Call(bank, None, None)
        assert L.psdcv_bank_var_device(*c.head, *what, C.c_void_p(ptr), None, *c.tail) == pkg.ERR_ARG
        assert pkg.lib().psdc_last_error(bank._h).decode() == "psdcv_bank_var_device: " + text
    c = bankread._Call(bank, None, None)
    assert L.psdcv_bank_var(*c.head, rec.ctypes.data, nv, taus.ctypes.data, nt, None, *c.tail) == pkg.ERR_ARG
    assert pkg.lib().psdc_last_error(bank._h).decode() == "psdcv_bank_var: null output"
    c = bankread._Call(bank, None, None)
    assert L.psdcv_bank_var(*c.head, rec.ctypes.data, nv, taus.ctypes.data, nt, out.ctypes.data, None, None, None, 0, None) == pkg.ERR_ARG
    assert pkg.lib().psdc_last_error(bank._h).decode() == "psdcv_bank_var: null lens"
    assert L.psdcv_rows_var_device(bank._h, C.c_void_p(ptr), C.c_void_p(ptr), 8, None, 1, rec.ctypes.data, nv, taus.ctypes.data, nt, C.c_void_p(ptr),
                                   None, None) == pkg.ERR_ARG
    assert pkg.lib().psdc_last_error(bank._h).decode() == "psdcv_rows_var_device: null lens"
    lay = bankread.layout(bank)
    for name, extra in (("psdcv_bank_var", (out.ctypes.data,)), ("psdcv_bank_var_device", (C.c_void_p(ptr), None))):
        c = bankread._Call(bank, None, None)  # room for fewer breaks than channel 0 has
        rc = getattr(L, name)(*c.head, rec.ctypes.data, nv, taus.ctypes.data, nt, *extra, c.lens.ctypes.data, c.nb.ctypes.data, c.br.ctypes.data, 2,
                              C.byref(c.info))
        assert rc == pkg.ERR_CAPACITY and "breaks_cap" in pkg.lib().psdc_last_error(bank._h).decode()
        assert [int(v) for v in c.lens] == lay["lens"] and int(c.nb[0]) == len(lay["breaks"][0]) and int(c.info.launches) == 0
        assert int(c.info.max_len) == lay["max_len"]
    assert np.all(out == SENTINEL) and np.all(t.cpu().numpy() == SENTINEL)
    assert bankvar.bank_var(bank, TAUS)["var"].tobytes() == before
    with pytest.raises(pkg.PsdError):
        bankvar.bank_var(bank, TAUS, ["avar"])


def test_cli_var_curves(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --bank-readout --var: a header and one `tau,deviation` line a tau for every trace and kind, from one call"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batches, frames = 8, 700
    words = np.random.default_rng(5).integers(-20000, 20000, (4, 8 * batches * frames)).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(words, batches, seq0=1)
    path = tmp_path / "frames.bin"
    path.write_bytes(data)
    cli = [sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--file", str(path), "--frame-size", str(fs)]
    r = subprocess.run(cli + ["--bank-readout", "--var", "avar:4", "--var", "fvar"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    heads = [k for k, ln in enumerate(lines) if " avar taus " in ln or " fvar taus " in ln]
    assert len(heads) == 8, r.stdout[-2000:]
    count = int(lines[heads[0]].split(" taus ")[1].split()[0])
    assert count >= 8
    curves = {}
    for k in heads:
        xy = np.asarray([[float(v) for v in ln.split(",")] for ln in lines[k + 1:k + 1 + count]])
        assert xy.shape == (count, 2) and xy[0, 0] == 1.0 and np.all(np.diff(xy[:, 0]) > 0) and np.all(xy[:, 1] >= 0.0), lines[k]
        curves[lines[k].split(" taus ")[0]] = xy
    a, f = curves[[c for c in curves if c.endswith("avar")][0]], curves[[c for c in curves if c.endswith("fvar")][0]]
    assert np.all(f[:, 1] <= a[:, 1]) and np.any(f[:, 1] < a[:, 1]) and a[0, 1] > 0.0  # the main lobe alone holds less (every term is >= 0)
    r = subprocess.run(cli + ["--var", "avar"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--var needs --bank-readout" in r.stderr
