"""Cross-spectral density cascade on the GPU (psdc_cross_*, csrc/cross.hip) against the oracle and the restatement of
tests/test_cross_host.py.  Semantics: include/psdcascade.h, "cross-spectral density cascade"."""
import numpy as np
import pytest

from conftest import assert_psd_close
from test_cross_host import U32_MAX, restate, stitch_rows

pytestmark = pytest.mark.gpu


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def window_of(pkg, n, kind):
    if kind == "hann":
        return pkg.Window.HANN, "hann"
    if kind == "rect":
        return pkg.Window.RECTANGULAR, "rect"
    wt = pkg.WindowTable.hann(n)
    w = np.sqrt(wt.win).astype(np.float32)  # a caller's table: sqrt-Hann, overlap n/4
    return pkg.WindowTable(w, 0.5, 1.2, n // 4), (w, 0.5, 1.2, n // 4)


def oracle_psd(ora, n, owin, x, detrend, avg, prec="f64"):
    ref = ora.PsdCascade(n, prec, window=owin)
    ref.set_detrend(detrend)
    ref.set_avg(*avg)
    ref.process(x)
    p, br, _ = ref.psd()
    return p, br


def assert_breaks(br, ref_br):
    assert len(br) == len(ref_br)
    for b, r in zip(br, ref_br):
        assert (b.count, b.pending, b.bins.start, b.bins.stop, b.start, b.processed) == (
            r["count"], r["pending"], r["bins_start"], r["bins_end"], r["start"], r["processed"]), (b, r)


def assert_sxy_close(got, ref, sxx, syy, tol, what="", atol_frac=0.0):
    """|got - ref| <= tol sqrt(Sxx Syy) per bin (+ atol_frac of its mean: bins a detrend nulls, as ATOL_FRAC in conftest.py)"""
    bound = tol * np.sqrt(np.asarray(sxx, np.float64) * np.asarray(syy, np.float64))
    bound = bound + atol_frac * np.mean(bound) / tol
    err = np.abs(np.asarray(got, np.complex128) - np.asarray(ref, np.complex128))
    worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), f"{what}: Sxy bin {worst} error {err[worst]:.3g} > {bound[worst]:.3g}"


DETRENDS = {"none": 0, "midpoint": 1, "span": 2, "mean": 3}


@pytest.mark.parametrize("n,wkind,detrend,avg,length", [
    (64, "hann", "none", None, 1 << 17),
    (256, "rect", "mean", None, 1 << 18),
    (512, "custom", "span", (U32_MAX, 1000), 1 << 18),
    (1024, "hann", "midpoint", (100, U32_MAX), 1 << 19),
    (4096, "hann", "none", None, 1 << 20),
    (1024, "custom", "mean", None, 1 << 19),
    (256, "hann", "span", (40, U32_MAX), 1 << 18),
])
def test_cross_parity(pkg, ora, gpu_required, n, wkind, detrend, avg, length):
    win, owin = window_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    x = noise(length, n)
    y = (0.6 * x + 0.8 * noise(length, n + 7)).astype(np.float32)
    g = pkg.CsdCascade(n, window=win)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    g.process(x, y)
    sxx, syy, sxy, br = g.csd()
    px, bx = oracle_psd(ora, n, owin, x, detrend, avg)
    py, _ = oracle_psd(ora, n, owin, y, detrend, avg)
    assert_breaks(br, bx)
    if detrend == "none":
        assert_psd_close(sxx, px, f"Sxx n={n}", pure=True)
        assert_psd_close(syy, py, f"Syy n={n}", pure=True)
    else:  # a detrend nulls the lowest bins: the widened bound, held to the reference's own f32 arithmetic there
        assert_psd_close(sxx, px, f"Sxx n={n} {detrend}", ref_f32=oracle_psd(ora, n, owin, x, detrend, avg, "f32")[0])
        assert_psd_close(syy, py, f"Syy n={n} {detrend}", ref_f32=oracle_psd(ora, n, owin, y, detrend, avg, "f32")[0])
    st = restate(ora, x, y, n, owin, detrend, avg, "f64")
    rx, ry, rxy, rbr = stitch_rows(pkg, n, win if isinstance(win, pkg.WindowTable) else pkg.WindowTable._kind(n, win), st,
                                   pkg.MergeOpts())
    assert rbr == br
    assert_sxy_close(sxy, rxy, rx, ry, 1e-5, f"n={n} {wkind} {detrend}", atol_frac=0.0 if detrend == "none" else 1e-6)
    # stage counts and Breaks equal those of the auto-PSD object fed x
    b = pkg.PsdCascadeBank(n, 1, win)
    b.set_detrend(DETRENDS[detrend])
    b.set_avg(pkg.AvgOpts(*avg))
    b.process(0, x)
    _, bbr = b.psd(0)
    assert bbr == br and g.num_stages() == b.num_stages(0)


@pytest.mark.parametrize("ratio", [1e-4, 1e4])
def test_cross_scale(pkg, ora, gpu_required, ratio):
    """Channels 1e4 apart in scale: each keeps its own relative accuracy (no packing of x + i y)."""
    n = 1024
    x = noise(1 << 19, 11)
    y = (ratio * (0.5 * x + noise(1 << 19, 12))).astype(np.float32)
    g = pkg.CsdCascade(n)
    g.process(x, y)
    sxx, syy, sxy, br = g.csd()
    px, _ = oracle_psd(ora, n, "hann", x, "none", (U32_MAX, U32_MAX))
    py, _ = oracle_psd(ora, n, "hann", y, "none", (U32_MAX, U32_MAX))
    assert_psd_close(sxx, px, "Sxx", pure=True)
    assert_psd_close(syy, py, "Syy", pure=True)


def test_cross_identity(pkg, gpu_required):
    n = 512
    x = noise(1 << 19, 3)
    g = pkg.CsdCascade(n)
    g.process(x, x)
    sxx, syy, sxy, _ = g.csd()
    assert np.all(np.abs(sxy.real - sxx) <= 1e-6 * sxx)
    assert np.all(np.abs(sxy.imag) <= 1e-6 * sxx)
    assert np.all(np.abs(syy - sxx) <= 1e-6 * sxx)  # (the two channels' sums need not be formed in the same order)
    coh = pkg.coherence(sxx, syy, sxy)
    assert np.all(np.abs(coh - 1) <= 1e-5)


def _passband_bins(br, freqs, min_count=16):
    keep = np.zeros(freqs.size, bool)
    for b in br:
        if b.include and b.count >= min_count:
            keep[b.start:b.start + (b.bins.stop - b.bins.start)] = True
    return keep


def test_cross_delay_phase(pkg, gpu_required):
    """y = x delayed by 3 samples: arg H = -2 pi f 3."""
    n, d = 1024, 3
    x = noise(1 << 21, 5)
    y = np.concatenate([np.zeros(d, np.float32), x[:-d]])
    g = pkg.CsdCascade(n)
    g.process(x, y)
    sxx, syy, sxy, br = g.csd()
    f = pkg.Break.frequencies(br).astype(np.float64)
    keep = _passband_bins(br, f)
    assert keep.sum() > 500
    ph = np.angle(pkg.transfer(sxx, sxy) * np.exp(2j * np.pi * f * d))
    assert np.max(np.abs(ph[keep])) <= 0.01


def test_cross_fir_response(pkg, gpu_required):
    """y = FIR(x): |H| and arg H follow the filter's response (noise-free, so only the window's leakage and the averages'
    scatter remain: 0.02 of the response's peak, 0.02 rad where |H| > 0.2)."""
    n = 1024
    taps = np.array([0.5, 0.3, -0.2, 0.1])
    x = noise(1 << 21, 8)
    y = np.convolve(x.astype(np.float64), taps)[:x.size].astype(np.float32)
    g = pkg.CsdCascade(n)
    g.process(x, y)
    sxx, syy, sxy, br = g.csd()
    f = pkg.Break.frequencies(br).astype(np.float64)
    keep = _passband_bins(br, f)
    htrue = np.exp(-2j * np.pi * np.outer(f, np.arange(taps.size))) @ taps
    h = pkg.transfer(sxx, sxy)
    assert np.max(np.abs(np.abs(h[keep]) - np.abs(htrue[keep]))) <= 0.02 * np.max(np.abs(htrue))
    big = keep & (np.abs(htrue) > 0.2)
    dph = np.angle(h[big] / htrue[big])
    assert np.max(np.abs(dph)) <= 0.02
    assert np.all(pkg.coherence(sxx, syy, sxy)[keep] > 0.99)


def assert_same_csd(a, b, tol, what=""):
    assert a[3] == b[3], what
    if tol == 0:
        for u, v in zip(a[:3], b[:3]):
            assert u.tobytes() == v.tobytes(), what
        return
    assert np.all(np.abs(a[0] - b[0]) <= tol * b[0]), what
    assert np.all(np.abs(a[1] - b[1]) <= tol * b[1]), what
    assert_sxy_close(a[2], b[2], b[0], b[1], tol, what)


def test_cross_chunking_determinism_reset(pkg, gpu_required):
    import torch
    n = 512
    length = (1 << 21) + 1234
    x = noise(length, 21)
    y = (0.3 * x + noise(length, 22)).astype(np.float32)
    one = pkg.CsdCascade(n)
    one.process(x, y)
    ref = one.csd()
    rng = np.random.default_rng(4)

    def feed_host(obj):
        i = 0
        for c in [7, 5, 512, 1 << 20, 3, 5, 999]:
            obj.process(x[i:i + c], y[i:i + c])
            i += c
        while i < length:
            c = int(rng.choice([5, 513, 1 << 20]))
            obj.process(x[i:i + c], y[i:i + c])
            i += c

    a = pkg.CsdCascade(n)
    feed_host(a)
    assert_same_csd(a.csd(), ref, 2e-6, "host chunks")
    # device chunks
    dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    b = pkg.CsdCascade(n)
    cuts = [0, 5, 12, 12 + 512, 12 + 512 + (1 << 20), length]
    for s, e in zip(cuts[:-1], cuts[1:]):
        b.process_device(dx.data_ptr() + 4 * s, dy.data_ptr() + 4 * s, e - s)
    got_b = b.csd()
    assert_same_csd(got_b, ref, 2e-6, "device chunks")
    # same calls, same bits
    c = pkg.CsdCascade(n)
    for s, e in zip(cuts[:-1], cuts[1:]):
        c.process_device(dx.data_ptr() + 4 * s, dy.data_ptr() + 4 * s, e - s)
    assert_same_csd(c.csd(), got_b, 0, "same calls")
    # reset + replay == fresh
    c.set_detrend(3)
    c.process(x[:100000], y[:100000])
    c.reset()
    for s, e in zip(cuts[:-1], cuts[1:]):
        c.process_device(dx.data_ptr() + 4 * s, dy.data_ptr() + 4 * s, e - s)
    assert_same_csd(c.csd(), got_b, 0, "reset + replay")
    assert c.stats_read()["pairs_in"] == length


def test_cross_pairs_and_streams(pkg, gpu_required):
    import torch
    n = 256
    lens = [300_000, 123_457, 1 << 18, 77_777]
    xs = [noise(m, 100 + i) for i, m in enumerate(lens)]
    ys = [(0.5 * xs[i] + noise(m, 200 + i)).astype(np.float32) for i, m in enumerate(lens)]
    bank = pkg.CsdCascadeBank(n, 4)
    pos = [0] * 4
    step = [10_000, 33_333, 65_536, 7_777]
    while any(pos[i] < lens[i] for i in range(4)):
        for i in range(4):
            if pos[i] < lens[i]:
                e = min(lens[i], pos[i] + step[i])
                bank.process(i, xs[i][pos[i]:e], ys[i][pos[i]:e])
                pos[i] = e
    for i in range(4):
        single = pkg.CsdCascade(n)
        single.process(xs[i], ys[i])
        assert_same_csd(bank.csd(i), single.csd(), 2e-6, f"pair {i}")
    with pytest.raises(pkg.PsdError) as e:
        bank.process(4, xs[0][:10], ys[0][:10])
    assert e.value.code == pkg.ERR_ARG and "out of range" in str(e.value)
    # a producer on a torch stream, handed over with an event
    m = 1 << 20
    hx, hy = noise(m, 300), noise(m, 301)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tx = torch.from_numpy(hx).pin_memory().cuda(non_blocking=True) * 1.0
        ty = torch.from_numpy(hy).pin_memory().cuda(non_blocking=True) * 1.0
        ev = torch.cuda.Event()
        ev.record(s)
    g = pkg.CsdCascade(n)
    g.process_device(tx.data_ptr(), ty.data_ptr(), m, after=ev.cuda_event)
    got = g.csd()
    h = pkg.CsdCascade(n)
    h.process(hx, hy)
    assert_same_csd(got, h.csd(), 2e-6, "after=")
    s.synchronize()


def test_cross_launch_count_and_size(pkg, gpu_required):
    import torch
    n = 1024
    m = 1 << 22
    dx = torch.randn(m, device="cuda")
    dy = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.CsdCascade(n)
    for _ in range(512):  # 2^31 pairs: eight stages
        g.process_device(dx.data_ptr(), dy.data_ptr(), m)
    # eight more calls without a sync: each round has the segments of stage 0 AND those the decimators of the calls before
    # brought to stages 1, 2, 3, ... -- one launch per (pair, stage) would read 8 x (stages with work), not <= 3 a call
    g.stats_read(reset=True)
    for _ in range(8):
        g.process_device(dx.data_ptr(), dy.data_ptr(), m)
    assert g.stats_read()["launches"] <= 3 * 8
    g.sync()
    assert g.num_stages() >= 8
    # config size: 2^26 pairs in one call, against the auto-PSD object fed x
    big = 1 << 26
    bx = torch.randn(big, device="cuda")
    by = (0.5 * bx + torch.randn(big, device="cuda"))
    torch.cuda.synchronize()
    c = pkg.CsdCascade(n)
    c.process_device(bx.data_ptr(), by.data_ptr(), big)
    sxx, syy, sxy, br = c.csd()
    p = pkg.PsdCascadeBank(n, 1)
    p.process_device(0, bx.data_ptr(), big)
    pp, pbr = p.psd(0)
    assert pbr == br and len(br) >= 7
    assert_psd_close(sxx, pp, "Sxx vs PsdCascade at 2^26", pure=True)
    coh = pkg.coherence(sxx, syy, sxy)
    assert abs(np.median(coh) - 0.2) < 0.02  # |0.5|^2 / (1.25)
