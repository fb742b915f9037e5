"""Cross-spectral matrix cascade on the GPU (psdc_csm_*, csrc/csm.hip) against the oracle, the f64 restatement of
tests/test_cross_host.py and the pair object.  Semantics: include/psdcascade.h, "cross-spectral matrix cascade".
Tolerances are the pair tests' own: 1e-5 pure on the diagonals, 1e-5 sqrt(S_aa S_bb) off the diagonal (atol_frac 1e-6 where a
detrend nulls bins), 2e-6 between two chunkings, 0 between identical calls."""
import numpy as np
import pytest

from conftest import assert_psd_close
from test_cross_host import U32_MAX, restate, stitch_rows
from test_gpu_cross import DETRENDS, _passband_bins, assert_breaks, assert_sxy_close, noise, oracle_psd, window_of

pytestmark = pytest.mark.gpu

GAINS = [1.0, 0.6, -0.4, 0.25]


def channels(m, length, seed):
    """correlated noise channels: x_c = a_c x_0 + noise"""
    x0 = noise(length, seed)
    return [x0] + [(GAINS[c] * x0 + 0.8 * noise(length, seed + 10 * c)).astype(np.float32) for c in range(1, m)]


def assert_same_matrix(a, b, tol, what=""):
    (sa, ba), (sb, bb) = a, b
    assert ba == bb, what
    if tol == 0:
        assert sa.tobytes() == sb.tobytes(), what
        return
    m = sa.shape[0]
    for i in range(m):
        assert np.all(np.abs(sa[i, i].real - sb[i, i].real) <= tol * sb[i, i].real), (what, i)
        for j in range(i + 1, m):
            assert_sxy_close(sa[i, j], sb[i, j], sb[i, i].real, sb[j, j].real, tol, f"{what} S[{i},{j}]")


def assert_hermitian(S):
    m = S.shape[0]
    for a in range(m):
        assert np.all(S[a, a].imag == 0)
        for b in range(m):
            assert np.array_equal(S[b, a], np.conj(S[a, b]))


PARITY = [
    (64, 2, "hann", "none", None, 1 << 17),
    (64, 4, "rect", "mean", None, 1 << 17),
    (256, 3, "custom", "span", (U32_MAX, 1000), 1 << 18),
    (256, 4, "hann", "midpoint", (40, U32_MAX), 1 << 18),
    (1024, 4, "hann", "none", None, 1 << 19),
    (1024, 3, "custom", "mean", None, 1 << 19),
    (1024, 2, "rect", "span", (100, U32_MAX), 1 << 19),
    (2048, 4, "hann", "mean", None, 1 << 19),
    (2048, 3, "rect", "none", None, 1 << 19),
    (2048, 2, "custom", "midpoint", None, 1 << 19),
    (4096, 2, "hann", "none", None, 1 << 20),
    (4096, 3, "hann", "span", None, 1 << 20),
    (128, 3, "hann", "none", None, 1 << 17),
    (512, 4, "hann", "none", (U32_MAX, 500), 1 << 18),
]


@pytest.mark.parametrize("n,m,wkind,detrend,avg,length", PARITY)
def test_csm_parity(pkg, ora, gpu_required, n, m, wkind, detrend, avg, length):
    win, owin = window_of(pkg, n, wkind)
    wt = win if isinstance(win, pkg.WindowTable) else pkg.WindowTable._kind(n, win)
    avg = avg or (U32_MAX, U32_MAX)
    xs = channels(m, length, n + m)
    g = pkg.CsmCascade(n, m, window=win)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    g.process(xs)
    S, br = g.csd()
    assert S.shape[:2] == (m, m) and S.dtype == np.complex64
    assert_hermitian(S)
    # diagonals: the oracle's PsdCascade of each channel
    for a in range(m):
        pa, ba = oracle_psd(ora, n, owin, xs[a], detrend, avg)
        if a == 0:
            assert_breaks(br, ba)
        if detrend == "none":
            assert_psd_close(S[a, a].real, pa, f"S[{a},{a}] n={n} m={m}", pure=True)
        else:
            assert_psd_close(S[a, a].real, pa, f"S[{a},{a}] n={n} m={m} {detrend}",
                             ref_f32=oracle_psd(ora, n, owin, xs[a], detrend, avg, "f32")[0])
    # off-diagonals: the f64 restatement of every pair
    for a in range(m):
        for b in range(a + 1, m):
            st = restate(ora, xs[a], xs[b], n, owin, detrend, avg, "f64")
            rx, ry, rxy, rbr = stitch_rows(pkg, n, wt, st, pkg.MergeOpts())
            assert rbr == br
            assert_sxy_close(S[a, b], rxy, rx, ry, 1e-5, f"S[{a},{b}] n={n} m={m} {wkind} {detrend}",
                             atol_frac=0.0 if detrend == "none" else 1e-6)
    # stage counts and Breaks equal those of the auto-PSD object fed channel 0
    p = pkg.PsdCascadeBank(n, 1, win)
    p.set_detrend(DETRENDS[detrend])
    p.set_avg(pkg.AvgOpts(*avg))
    p.process(0, xs[0])
    _, pbr = p.psd(0)
    assert pbr == br and g.num_stages() == p.num_stages(0)
    for k in range(g.num_stages()):
        info, Sk = g.stage_spectra(k)
        pi = p.stage_info(0, k)
        assert (info["count"], info["pending"]) == (pi["count"], pi["pending"]), k
        assert_hermitian(Sk)


@pytest.mark.parametrize("n,m", [(512, 3), (1024, 4), (2048, 4), (256, 4)])
def test_csm_against_pairs(pkg, gpu_required, n, m):
    """every S_ab within the pair tests' chunking bound of CsdCascade.csd() fed (x_a, x_b); Breaks equal"""
    xs = channels(m, (1 << 19) + 777, 40 + m)
    g = pkg.CsmCascade(n, m)
    g.process(xs)
    S, br = g.csd()
    for a in range(m):
        for b in range(a + 1, m):
            c = pkg.CsdCascade(n)
            c.process(xs[a], xs[b])
            sxx, syy, sxy, cbr = c.csd()
            assert cbr == br
            assert np.all(np.abs(S[a, a].real - sxx) <= 2e-6 * sxx), (a, b)
            assert np.all(np.abs(S[b, b].real - syy) <= 2e-6 * syy), (a, b)
            assert_sxy_close(S[a, b], sxy, sxx, syy, 2e-6, f"S[{a},{b}] against the pair object")


def test_csm_scale(pkg, ora, gpu_required):
    """Channels 1e4 apart in scale keep their own relative accuracy."""
    n, length = 1024, 1 << 19
    x = noise(length, 11)
    xs = [x, (1e-4 * (0.5 * x + noise(length, 12))).astype(np.float32), (1e4 * (0.3 * x + noise(length, 13))).astype(np.float32)]
    g = pkg.CsmCascade(n, 3)
    g.process(xs)
    S, _ = g.csd()
    for a in range(3):
        pa, _ = oracle_psd(ora, n, "hann", xs[a], "none", (U32_MAX, U32_MAX))
        assert_psd_close(S[a, a].real, pa, f"S[{a},{a}]", pure=True)
    st = restate(ora, xs[1], xs[2], n, "hann", "none", (U32_MAX, U32_MAX), "f64")
    rx, ry, rxy, _ = stitch_rows(pkg, n, pkg.WindowTable.hann(n), st, pkg.MergeOpts())
    assert_sxy_close(S[1, 2], rxy, rx, ry, 1e-5, "S[1,2] of channels 1e8 apart")


def fir_case(length, seed=8):
    """two correlated inputs (coherence 0.5) through two known FIRs into one output plus noise.
    Output noise 0.01, not 0.05: a conditioned H1 estimate over nd averages scatters by sigma / sqrt((1 - coh) nd) a bin
    (Bendat & Piersol, random error of a conditioned frequency response), and the check keeps bins from count 16 on, so
    sigma = 0.05 alone gives 0.05 / sqrt(0.5 x 16) = 0.018, above the bound of 0.02 x 0.74 = 0.015 whatever the library
    computes; 0.01 gives 0.0035, a quarter of the bound, which leaves the bound to test the spectra."""
    x0 = noise(length, seed).astype(np.float64)
    x1 = 0.7 * x0 + 0.7 * noise(length, seed + 1)
    t0, t1 = np.array([0.5, 0.3, -0.2, 0.1]), np.array([0.4, -0.3, 0.2])
    y = np.convolve(x0, t0)[:length] + np.convolve(x1, t1)[:length] + 0.01 * noise(length, seed + 2)
    return [x0.astype(np.float32), x1.astype(np.float32), y.astype(np.float32)], t0, t1


def test_csm_mimo_fir_response(pkg, gpu_required):
    """mimo_transfer follows both responses within test_cross_fir_response's bounds where the single-input transfer() of input 0
    misses its own by more than three times that bound (it tends to H0 + 0.7 H1)."""
    n = 1024
    xs, t0, t1 = fir_case(1 << 21)
    g = pkg.CsmCascade(n, 3)
    g.process(xs)
    S, br = g.csd()
    f = pkg.Break.frequencies(br).astype(np.float64)
    keep = _passband_bins(br, f)
    assert keep.sum() > 500
    H = pkg.mimo_transfer(S, [0, 1], [2])
    worst_single = 0.0
    for i, taps in enumerate((t0, t1)):
        htrue = np.exp(-2j * np.pi * np.outer(f, np.arange(taps.size))) @ taps
        h = H[0, i]
        bound = 0.02 * np.max(np.abs(htrue))
        err = np.max(np.abs(np.abs(h[keep]) - np.abs(htrue[keep])))
        print(f"input {i}: max | |H| - |Htrue| | = {err:.4g} (bound {bound:.4g})")
        assert err <= bound
        big = keep & (np.abs(htrue) > 0.2)
        dph = np.max(np.abs(np.angle(h[big] / htrue[big])))
        print(f"input {i}: max phase error {dph:.4g} rad (bound 0.02)")
        assert dph <= 0.02
        if i == 0:
            h1 = pkg.transfer(S[0, 0].real, S[0, 2])
            worst_single = np.max(np.abs(h1[keep] - htrue[keep]))
            print(f"single-input H1 of input 0 misses by {worst_single:.4g}")
            assert worst_single > 3 * bound
    mc = pkg.multiple_coherence(S, [0, 1], 2)
    assert np.all(mc[keep] > 0.9) and np.all(mc[keep] <= 1 + 1e-6)


def test_csm_chunking_determinism_reset(pkg, gpu_required):
    import torch
    n, m = 512, 4
    length = (1 << 21) + 1234
    xs = channels(m, length, 21)
    one = pkg.CsmCascade(n, m)
    one.process(xs)
    ref = one.csd()
    rng = np.random.default_rng(4)
    a = pkg.CsmCascade(n, m)
    i = 0
    sizes = [7, 5, 512, 1 << 20, 3, 5, 999]
    while i < length:
        c = sizes.pop(0) if sizes else int(rng.choice([5, 513, 1 << 20]))
        a.process([x[i:i + c] for x in xs])
        i += c
    assert_same_matrix(a.csd(), ref, 2e-6, "host chunks")
    dx = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()
    cuts = [0, 5, 12, 12 + 512, 12 + 512 + (1 << 20), length]

    def feed(obj):
        for s, e in zip(cuts[:-1], cuts[1:]):
            obj.process_device([d.data_ptr() + 4 * s for d in dx], e - s)

    b = pkg.CsmCascade(n, m)
    feed(b)
    got_b = b.csd()
    assert_same_matrix(got_b, ref, 2e-6, "device chunks")
    c = pkg.CsmCascade(n, m)
    feed(c)
    assert_same_matrix(c.csd(), got_b, 0, "same calls")
    c.set_detrend(3)
    c.process([x[:100000] for x in xs])
    c.reset()
    feed(c)
    assert_same_matrix(c.csd(), got_b, 0, "reset + replay")
    assert c.stats_read()["sample_times_in"] == length


def test_csm_groups_and_streams(pkg, gpu_required):
    import torch
    n, m = 256, 3
    lens = [300_000, 123_457, 1 << 18, 77_777]
    xs = [channels(m, ln, 100 + i) for i, ln in enumerate(lens)]
    bank = pkg.CsmCascadeBank(n, m, 4)
    pos = [0] * 4
    step = [10_000, 33_333, 65_536, 7_777]
    while any(pos[i] < lens[i] for i in range(4)):
        for i in range(4):
            if pos[i] < lens[i]:
                e = min(lens[i], pos[i] + step[i])
                bank.process(i, [x[pos[i]:e] for x in xs[i]])
                pos[i] = e
    for i in range(4):
        single = pkg.CsmCascade(n, m)
        single.process(xs[i])
        assert_same_matrix(bank.csd(i), single.csd(), 2e-6, f"group {i}")
    with pytest.raises(pkg.PsdError) as e:
        bank.process(4, [x[:10] for x in xs[0]])
    assert e.value.code == pkg.ERR_ARG and "out of range" in str(e.value) and "group 4" in str(e.value)
    with pytest.raises(pkg.PsdError):
        bank.process(0, [xs[0][0][:10], xs[0][1][:10]])  # two channels for m = 3
    with pytest.raises(pkg.PsdError) as e:
        bank.set_detrend(4)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED
    # a producer on a torch stream, handed over with an event
    ln = 1 << 20
    hx = [noise(ln, 300 + c) for c in range(m)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tx = [torch.from_numpy(h).pin_memory().cuda(non_blocking=True) * 1.0 for h in hx]
        ev = torch.cuda.Event()
        ev.record(s)
    g = pkg.CsmCascade(n, m)
    g.process_device([t.data_ptr() for t in tx], ln, after=ev.cuda_event)
    got = g.csd()
    h = pkg.CsmCascade(n, m)
    h.process(hx)
    assert_same_matrix(got, h.csd(), 2e-6, "after=")
    s.synchronize()


def test_csm_launch_count_and_size(pkg, gpu_required):
    import torch
    n, m = 1024, 4
    ln = 1 << 22
    d = [torch.randn(ln, device="cuda") for _ in range(m)]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    g = pkg.CsmCascade(n, m)
    for _ in range(512):  # 2^31 sample times: eight stages
        g.process_device(ptrs, ln)
    g.stats_read(reset=True)
    for _ in range(8):
        g.process_device(ptrs, ln)
    assert g.stats_read()["launches"] <= 3 * 8
    g.sync()
    assert g.num_stages() >= 8
    g.close()
    # full size: 2^26 samples a channel in one call, diagonal 0 against the auto-PSD object
    big = 1 << 26
    bx = torch.randn(big, device="cuda")
    bs = [bx] + [(0.5 * bx + torch.randn(big, device="cuda")) for _ in range(m - 1)]
    torch.cuda.synchronize()
    c = pkg.CsmCascade(n, m)
    c.process_device([t.data_ptr() for t in bs], big)
    S, br = c.csd()
    p = pkg.PsdCascadeBank(n, 1)
    p.process_device(0, bx.data_ptr(), big)
    pp, pbr = p.psd(0)
    assert pbr == br and len(br) >= 7
    assert_psd_close(S[0, 0].real, pp, "S[0,0] vs PsdCascade at 2^26", pure=True)
    coh = pkg.coherence(S[0, 0].real, S[1, 1].real, S[0, 1])
    assert abs(np.median(coh) - 0.2) < 0.02  # |0.5|^2 / 1.25
    assert_hermitian(S)
