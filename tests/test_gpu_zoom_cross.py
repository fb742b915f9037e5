"""Zoom cross cascade on the GPU (psdc_zcsd_*, csrc/zoom_cross.hip) against the f64 restatement of
tests/test_zoom_cross_host.py and its complex64 sibling, and against the objects that exist (ZoomCascade, CsdCascade) where they
are comparable.  Semantics: include/psdcascade.h, "zoom cross cascade"."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS, assert_breaks, assert_sxy_close
from test_zoom_cross_host import pair_input, restate_zoom_cross, stitch_zoom_cross
from test_zoom_host import M64, U32_MAX, carrier_ftw, emul, mix_f32, mix_f64, noise, windows_of  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, window, detrend, avg, carriers (a, b), length).  64: many teams a workgroup, last tiles with idle teams; 2048: a team of two
# wavefronts and an odd segment count (261); 4096 (if supported): one workgroup a team.
PARITY_CASES = [
    (64, "hann", "none", None, (("bin", 5), ("bin", 5)), (1 << 16) + 37),
    (256, "rect", "mean", None, (0.2345678901234567, 0.2345678901234567), 1 << 17),
    (512, "custom", "span", (U32_MAX, 1000), (0.7131313131313131, 0.3141592653589793), 1 << 17),
    (1024, "hann", "midpoint", (100, U32_MAX), (0.8660254037844386, 0.8660254037844386), 1 << 18),
    (2048, "hann", "none", None, (0.6180339887498949, 0.6180339887498949), (1 << 18) + 2048 * 3),
    (4096, "hann", "none", None, (0.0, 0.0), 1 << 19),
]


def make(pkg, n, ftw, window=None, phase0=(0, 0), detrend=None, avg=None):
    g = pkg.ZoomCsdCascade(n, window=window if window is not None else pkg.Window.HANN)
    for side in (0, 1):
        g.set_carrier(ftw=ftw[side], phase0=phase0[side], side=side)
    if detrend is not None:
        g.set_detrend(detrend)
    if avg is not None:
        g.set_avg(pkg.AvgOpts(*avg))
    return g


def assert_cross_rows(got, ref, tol, what, atol_frac=0.0):
    """the two complex rows of a csd() tuple against a reference tuple: tol sqrt(S_aa S_bb) of the reference, side by side"""
    assert_sxy_close(got[4], ref[4], ref[0], ref[2], tol, what + " S_ab upper", atol_frac=atol_frac)
    assert_sxy_close(got[5], ref[5], ref[1], ref[3], tol, what + " S_ab lower", atol_frac=atol_frac)


def same_csd(a, b, tol, what=""):
    """the chunking bound on all rows: the auto rows relative, the cross rows relative to sqrt(S_aa S_bb); tol 0: equal bits"""
    assert a[6] == b[6], what
    if tol == 0:
        for u, v in zip(a[:6], b[:6]):
            assert u.tobytes() == v.tobytes(), what
        return
    for u, v in zip(a[:4], b[:4]):
        assert np.all(np.abs(u - v) <= tol * v), what
    assert_cross_rows(a, b, tol, what)


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_zoom_cross_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, avg, carriers, length = PARITY_CASES[case]
    if not pkg.zcsd_supported(n):
        assert n == 4096  # the one size that may be refused
        with pytest.raises(pkg.PsdError) as e:
            pkg.ZoomCsdCascade(n)
        assert e.value.code == pkg.ERR_ARG and "n = 4096" in str(e.value)
        return
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    a, b = pair_input(length, 2000 + n)
    ftw = tuple(carrier_ftw(pkg, n, c) for c in carriers)
    g = make(pkg, n, ftw, pwin, detrend=DETRENDS[detrend], avg=avg)
    g.process(a, b)
    got = g.csd()
    ref = stitch_zoom_cross(pkg, n, pwin, restate_zoom_cross(ora, a, b, n, ftw, (0, 0), owin, detrend, avg))
    assert got[6] == ref[6]
    names = ("S_aa upper", "S_aa lower", "S_bb upper", "S_bb lower")
    if detrend == "none":
        for name, u, v in zip(names, got[:4], ref[:4]):
            rel = assert_psd_close(u, v, f"zoom cross {name} case {case}", pure=True)
            print(f"case {case} {name}: worst relative error {rel:.3g}")
        assert_cross_rows(got, ref, 1e-5, f"case {case}")
    else:  # a detrend nulls bin 0: the widened bound, held to the complex64 sibling's own f32 arithmetic there
        iq = (mix_f32(emul, a, ftw[0]), mix_f32(emul, b, ftw[1]))
        sib = stitch_zoom_cross(pkg, n, pwin, restate_zoom_cross(ora, a, b, n, ftw, (0, 0), owin, detrend, avg, "f32", iq=iq))
        for name, u, v, s in zip(names, got[:4], ref[:4], sib[:4]):
            assert_psd_close(u, v, f"zoom cross {name} case {case} {detrend}", ref_f32=s)
        assert_cross_rows(got, ref, 1e-5, f"case {case} {detrend}", atol_frac=1e-6)
    err = max(float(np.max(np.abs(got[4 + i] - ref[4 + i]) / np.sqrt(ref[i].astype(np.float64) * ref[2 + i]))) for i in (0, 1))
    print(f"case {case} S_ab: worst error / sqrt(S_aa S_bb) {err:.3g}")
    # Breaks are those of a ZoomCascade fed a, and of the oracle's cascade
    z = pkg.ZoomCascade(n, ftw=ftw[0], window=pwin)
    z.set_detrend(DETRENDS[detrend])
    z.set_avg(pkg.AvgOpts(*avg))
    z.process(a)
    assert z.psd()[2] == got[6] and z.num_stages() == g.num_stages()
    o = ora.PsdCascade(n, "f64", window=owin)
    o.set_detrend(detrend)
    o.set_avg(*avg)
    o.process(a)
    assert_breaks(got[6], o.psd()[1])
    if case == 0:  # the raw rows of a stage, in the header's order: a fresh object fed the stream's head against the restatement
        head = n * 40
        st0 = restate_zoom_cross(ora, a[:head], b[:head], n, ftw, (0, 0), owin, detrend, avg)[0]
        h = make(pkg, n, ftw, pwin, detrend=DETRENDS[detrend], avg=avg)
        h.process(a[:head], b[:head])
        info, rows = h.stage_spectra(0)
        assert rows.shape == (8, n // 2 + 1) and info["count"] == st0["count"] and info["pending"] == st0["pending"]
        for r in range(8):
            bound = 1e-5 * (st0["rows"][r] if r < 4 else np.sqrt(st0["rows"][r % 2] * st0["rows"][2 + r % 2]))
            assert np.all(np.abs(rows[r] - st0["rows"][r]) <= bound), r


def test_zoom_cross_against_existing_objects(pkg, gpu_required):
    """The auto rows are two ZoomCascades' (2e-6, the chunking bound of the header: the partial sums are ordered differently);
    ftw = 0: S_ab upper is CsdCascade's Sxy of (a, b) at 1e-5 sqrt(S_aa S_bb); the same stream and carrier on both sides:
    S_ab = S_aa."""
    n, length = 512, 1 << 18
    a, b = pair_input(length, 91)
    ftw = (pkg.zoom_ftw(0.2718281828459045)[0], pkg.zoom_ftw(0.6180339887498949)[0])
    ph = (0x0123456789ABCDEF, 1 << 62)
    g = make(pkg, n, ftw, phase0=ph)
    g.process(a, b)
    got = g.csd()
    for side, x in enumerate((a, b)):
        z = pkg.ZoomCascade(n, ftw=ftw[side], phase0=ph[side])
        z.process(x)
        up, lo, br = z.psd()
        assert br == got[6]
        for name, u, v in (("upper", got[2 * side], up), ("lower", got[2 * side + 1], lo)):
            rel = float(np.max(np.abs(u - v) / v))
            print(f"side {side} {name} against ZoomCascade: {rel:.3g}")
            assert rel <= 2e-6, (side, name, rel)
    g0 = make(pkg, n, (0, 0))
    g0.process(a, b)
    got0 = g0.csd()
    c = pkg.CsdCascade(n)
    c.process(a, b)
    sxx, syy, sxy, cbr = c.csd()
    assert cbr == got0[6]
    assert_sxy_close(got0[4], sxy, sxx, syy, 1e-5, "ftw = 0: S_ab upper against CsdCascade")
    assert_psd_close(got0[0], sxx, "ftw = 0: S_aa upper against CsdCascade", pure=True)
    assert_psd_close(got0[2], syy, "ftw = 0: S_bb upper against CsdCascade", pure=True)
    s = make(pkg, n, (ftw[0], ftw[0]), phase0=(ph[0], ph[0]))
    s.process(a, a)
    aup, alo, bup, blo, xup, xlo, _ = s.csd()
    for auto, x in ((aup, xup), (alo, xlo)):
        assert np.all(np.abs(x.real - auto) <= 1e-6 * auto) and np.all(np.abs(x.imag) <= 1e-6 * auto)
    assert np.all(np.abs(pkg.coherence(aup, bup, xup) - 1.0) <= 1e-5) and np.all(np.abs(pkg.coherence(alo, blo, xlo) - 1.0) <= 1e-5)
    # the helpers take the rows as they are
    off, dens = pkg.two_sided(got[0], got[1], got[6])
    assert off.size == dens.size and np.all(np.diff(off) > 0)
    h1 = pkg.transfer(got[0], got[4])
    assert h1.shape == got[4].shape and np.all(np.isfinite(h1))


def test_zoom_cross_conjugate_carriers(pkg, ora, gpu_required):
    """The recipe of the header: the same stream with ftw and -ftw, phase0 = 0.  S_bb upper is S_aa lower and the reverse (1e-5),
    and S_ab upper is the restatement's conj(Z_k Z_-k) within the cross bound."""
    n, length = 256, 1 << 17
    x = noise(length, 17)
    ftw = pkg.zoom_ftw(0.2345678901234567)[0]
    pair = (ftw, (-ftw) & M64)
    g = make(pkg, n, pair)
    g.process(x, x)
    got = g.csd()
    assert np.all(np.abs(got[2] - got[1]) <= 1e-5 * got[1]) and np.all(np.abs(got[3] - got[0]) <= 1e-5 * got[0])
    ref = stitch_zoom_cross(pkg, n, pkg.Window.HANN, restate_zoom_cross(ora, x, x, n, pair))
    assert got[6] == ref[6]
    assert_cross_rows(got, ref, 1e-5, "conjugate carriers")
    # written out for stage 0's first bins: conj(Z_a[k] Z_a[-k]) summed over the segments, from the f64 mixer alone
    i, q = mix_f64(x, ftw)
    w = np.asarray(pkg.WindowTable.hann(n).win, np.float64)
    hop = n // 2
    nseg = 1 + (length - n) // hop
    acc = np.zeros(n // 2 + 1, np.complex128)
    idx = (n - np.arange(n // 2 + 1)) % n
    for j in range(nseg):
        Z = np.fft.fft((i[j * hop:j * hop + n] + 1j * q[j * hop:j * hop + n]) * w)
        acc += np.conj(Z[:n // 2 + 1] * Z[idx])
    _, rows = g.stage_spectra(0)
    scale = np.sqrt(rows[0].astype(np.float64) * rows[2])
    assert np.all(np.abs((rows[4] + 1j * rows[6]) - acc) <= 1e-5 * scale)


def test_zoom_cross_lower_row_is_not_a_mirror(pkg, gpu_required):
    """A tone at f0 + delta on a and one at f0 - delta on b, delta the centre of bin 100 of stage 1 (N = 512): a's peak is in
    S_aa upper only, b's in S_bb lower only.  "Only": the other row of the same spectrum holds less than 1e-9 of the peak at that
    bin -- the tones sit on bin centres (no window leakage), the LO's error (2^-23) puts at most 2^-46 of a tone's power anywhere
    else and f32 rounding about eps^2 log2 N, so 1e-9 has four orders in hand, and a mirrored or conjugated-and-swapped row misses
    it by nine.  Neither tone is in the other channel, so S_ab is small on both sides."""
    n, k, bin_ = 512, 1, 100
    ftw, f0 = pkg.zoom_ftw(0.2)
    delta = bin_ / (n * 8.0 ** k)
    length = 1 << 17
    j = np.arange(length, dtype=np.float64)
    a = np.cos(2 * np.pi * (((f0 + delta) * j) % 1.0)).astype(np.float32)
    b = np.cos(2 * np.pi * (((f0 - delta) * j) % 1.0)).astype(np.float32)
    g = make(pkg, n, (ftw, ftw))
    g.process(a, b)
    assert g.num_stages() > k
    _, r = g.stage_spectra(k)
    r = r.astype(np.float64)
    assert int(np.argmax(r[0])) == bin_ and int(np.argmax(r[3])) == bin_
    print(f"stage {k} bin {bin_}: S_aa upper {r[0][bin_]:.3g} lower {r[1][bin_]:.3g}; S_bb upper {r[2][bin_]:.3g} lower {r[3][bin_]:.3g}; "
          f"|S_ab| upper {np.hypot(r[4][bin_], r[6][bin_]):.3g} lower {np.hypot(r[5][bin_], r[7][bin_]):.3g}")
    assert r[1][bin_] <= 1e-9 * r[0][bin_] and r[2][bin_] <= 1e-9 * r[3][bin_]
    peak = np.sqrt(r[0][bin_] * r[3][bin_])
    assert np.hypot(r[4][bin_], r[6][bin_]) <= 1e-4 * peak and np.hypot(r[5][bin_], r[7][bin_]) <= 1e-4 * peak
    # the stitched read-out shows the same, at the offset delta
    aup, alo, bup, blo, _, _, br = g.csd()
    f = pkg.Break.frequencies(br)
    assert abs(f[int(np.argmax(aup))] - delta) <= 0.5 / (n * 8.0 ** k) and abs(f[int(np.argmax(blo))] - delta) <= 0.5 / (n * 8.0 ** k)


def test_zoom_cross_cuts_and_memory(pkg, gpu_required):
    """One call against calls of 1000, 77 777 and 2^19 + 3 samples, host and device, within the chunking bound (2e-6); the same
    calls twice, host against device, and reset + replay: equal bits."""
    import torch
    n = 512
    cuts = np.cumsum([0, 1000, 77_777, (1 << 19) + 3])
    length = int(cuts[-1])
    a, b = pair_input(length, 31)
    ftw = (pkg.zoom_ftw(0.2718281828459045)[0], pkg.zoom_ftw(0.2718281828459045)[0])
    ph = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    one = make(pkg, n, ftw, phase0=ph)
    one.process(a, b)
    ref = one.csd()
    h = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        h.process(a[s:e], b[s:e])
    got_h = h.csd()
    same_csd(got_h, ref, 2e-6, "host chunks")
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    d = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(da.data_ptr() + 4 * int(s), db.data_ptr() + 4 * int(s), int(e - s))
    got_d = d.csd()
    same_csd(got_d, ref, 2e-6, "device chunks")
    same_csd(got_d, got_h, 0, "host against device, same calls")
    one_d = make(pkg, n, ftw, phase0=ph)
    one_d.process_device(da.data_ptr(), db.data_ptr(), length)
    same_csd(one_d.csd(), ref, 0, "host against device, one call")
    h2 = make(pkg, n, ftw, phase0=ph)
    for s, e in zip(cuts[:-1], cuts[1:]):
        h2.process(a[s:e], b[s:e])
    same_csd(h2.csd(), got_h, 0, "same calls twice")
    with pytest.raises(pkg.PsdError) as err:  # a carrier is set before the first sample only
        d.set_carrier(ftw=1, side=1)
    assert err.value.code == pkg.ERR_ARG and "before the first" in str(err.value)
    d.set_detrend(3)
    d.reset()  # (ZoomCsdCascade sets its carriers again; the detrend goes back to none)
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(da.data_ptr() + 4 * int(s), db.data_ptr() + 4 * int(s), int(e - s))
    same_csd(d.csd(), got_d, 0, "reset + replay")
    assert d.stats_read()["pairs_in"] == length
    bank = pkg.ZoomCsdCascadeBank(n, 1)
    bank.set_carrier(0, ftw=ftw[0])
    bank.process(0, a[:10], b[:10])
    bank.reset()
    bank.process(0, a[:50_000], b[:50_000])
    z0 = pkg.ZoomCsdCascade(n)
    z0.process(a[:50_000], b[:50_000])
    same_csd(bank.csd(0), z0.csd(), 0, "a bank's reset puts the carriers back to 0")


def test_zoom_cross_bank(pkg, gpu_required):
    """Three pairs with different carriers against three single objects: bit for bit when fed and read out in turn, within the
    chunking bound (2e-6) when the calls are interleaved."""
    n = 256
    lens = [200_000, 123_457, 1 << 17]
    step = [10_000, 33_333, 65_536]
    data = [pair_input(m, 500 + i) for i, m in enumerate(lens)]
    car = [tuple(pkg.zoom_ftw(f)[0] for f in fs) for fs in ((0.2, 0.2), (0.0123456789, 0.75), (0.4999, 0.4999))]
    ph = [(0, 0), (1 << 63, 12345), ((1 << 64) - 1, 7)]
    singles = []
    for i in range(3):
        s = make(pkg, n, car[i], phase0=ph[i])
        for p in range(0, lens[i], step[i]):
            s.process(data[i][0][p:p + step[i]], data[i][1][p:p + step[i]])
        singles.append(s.csd())

    def new_bank():
        bk = pkg.ZoomCsdCascadeBank(n, 3)
        for i in range(3):
            for side in (0, 1):
                bk.set_carrier(i, ftw=car[i][side], phase0=ph[i][side], side=side)
        return bk

    bank = new_bank()
    for i in range(3):
        for p in range(0, lens[i], step[i]):
            bank.process(i, data[i][0][p:p + step[i]], data[i][1][p:p + step[i]])
        same_csd(bank.csd(i), singles[i], 0, f"pair {i}, fed in turn")
    for i in range(3):
        same_csd(bank.csd(i), singles[i], 0, f"pair {i}, read again")
    mixed = new_bank()
    pos = [0] * 3
    while any(pos[i] < lens[i] for i in range(3)):
        for i in range(3):
            if pos[i] < lens[i]:
                mixed.process(i, data[i][0][pos[i]:pos[i] + step[i]], data[i][1][pos[i]:pos[i] + step[i]])
                pos[i] += step[i]
    for i in range(3):
        same_csd(mixed.csd(i), singles[i], 2e-6, f"pair {i}, interleaved")


def test_zoom_cross_argument_errors_on_an_object(pkg, gpu_required):
    """What needs an object: pair and side out of range, Detrend::Linear, NULL and unequal inputs."""
    L = pkg.lib()
    bank = pkg.ZoomCsdCascadeBank(256, 2)
    x = noise(1000, 1)
    with pytest.raises(pkg.PsdError) as e:
        bank.process(2, x, x)
    assert e.value.code == pkg.ERR_ARG and "pair 2 out of range (n_pairs 2)" in str(e.value)
    assert L.psdc_zcsd_set_carrier(bank._h, 2, 0, 1, 0) == pkg.ERR_ARG
    assert L.psdc_zcsd_set_carrier(bank._h, 0, 2, 1, 0) == pkg.ERR_ARG
    assert "side 2 out of range" in L.psdc_zcsd_last_error(bank._h).decode()
    with pytest.raises(pkg.PsdError) as e:
        bank.set_carrier(0, ftw=1, side=2)
    assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.PsdError) as e:
        bank.set_detrend(pkg.Detrend.LINEAR)
    assert e.value.code == pkg.ERR_UNIMPLEMENTED
    assert L.psdc_zcsd_process(bank._h, 0, pkg._fptr(x), None, 10) == pkg.ERR_ARG
    assert "null sample pointer" in L.psdc_zcsd_last_error(bank._h).decode()
    assert L.psdc_zcsd_process_device(bank._h, 0, None, None, 10, None) == pkg.ERR_ARG
    assert L.psdc_zcsd_process(bank._h, 0, None, None, 0) == 0  # (an empty call is accepted, as everywhere)
    with pytest.raises(pkg.PsdError):
        bank.process(0, x, x[:10])
    assert bank.num_stages(0) == 0 and bank.stats_read()["pairs_in"] == 0
    with pytest.raises(pkg.PsdError) as e:
        bank.stage_spectra(0, 0)
    assert e.value.code == pkg.ERR_ARG and "stage 0 out of range" in str(e.value)


@pytest.mark.parametrize("m,warm,depth", [(1 << 17, 8, 3), (1 << 22, 512, 8)])
def test_zoom_cross_launch_count(pkg, gpu_required, m, warm, depth):
    """A steady-state device call on one pair is PSDC_ZCSD_STEADY_LAUNCHES = 2 + 3 launches (two mixers; segments, decimators,
    fold + tails) with three and with eight live stages."""
    import torch
    n = 1024
    da, db = torch.randn(m, device="cuda"), torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.ZoomCsdCascade(n, f0=0.2)
    for _ in range(warm):
        g.process_device(da.data_ptr(), db.data_ptr(), m)
    g.stats_read(reset=True)
    for _ in range(8):
        g.process_device(da.data_ptr(), db.data_ptr(), m)
    assert g.stats_read()["launches"] == pkg.ZCSD_STEADY_LAUNCHES * 8 == 40
    g.sync()
    assert g.num_stages() >= depth


def test_zoom_cross_cli_raw(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --zoom-pair F0:raw:raw: the CSV (offset, then S_aa, S_bb, Re S_ab, Im S_ab a side) against a
    ZoomCsdCascadeBank fed the file's samples on both sides in one call (the tool feeds about 2^20 samples a call: the chunking
    bound, 2e-6, with the mean term the zoom tool's test uses for the bins the default detrend nulls)."""
    fs = 1000.0
    length = (1 << 20) + 777
    x = (noise(length, 43) + np.cos(2 * np.pi * 0.2001 * np.arange(length))).astype(np.float32)
    p = tmp_path / "raw.f32"
    x.astype("<f4").tofile(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--raw", str(p), "--fs", str(fs), "--zoom-pair",
                        "0.2:raw:0", "--csv", str(tmp_path / "csv")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "zoom pair raw:raw @ 0.2" in r.stdout
    d = np.loadtxt(tmp_path / "csv" / "zoompair_raw__raw_0_2.csv", delimiter=",")
    bank = pkg.ZoomCsdCascadeBank(512, 1)  # what the tool builds: the reference's default AcqOpts (detrend mean, avg_max 1000)
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    bank.set_carrier(0, f0=0.2)
    bank.process(0, x, x)
    aup, alo, bup, blo, xup, xlo, br = bank.csd(0)
    assert d.shape == (aup.size, 9)
    assert np.allclose(d[:, 0], pkg.Break.frequencies(br) * fs, rtol=1e-6, atol=0)
    for col, want in ((1, aup), (2, bup), (3, xup.real), (4, xup.imag), (5, alo), (6, blo), (7, xlo.real), (8, xlo.imag)):
        scale = aup if col < 5 else alo
        assert np.all(np.abs(d[:, col] - want) <= 2e-6 * scale + 1e-6 * np.mean(scale)), col
    assert abs(d[int(np.argmax(d[:, 1])), 0] - 0.0001 * fs) <= 0.5 * fs / (512 * 64)  # the tone, 1e-4 fs above the carrier
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "psd_cli.py"), "--raw", str(p), "--zoom-pair", "0.2:raw:nonesuch"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "unknown trace" in r.stderr
