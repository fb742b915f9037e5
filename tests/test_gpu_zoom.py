"""Zoom cascade on the GPU (psdc_zoom_*, csrc/zoom.hip) against the f64 restatement and its complex64 sibling of
tests/test_zoom_host.py, and against the auto-PSD object where a carrier makes the two comparable.  Semantics:
include/psdcascade.h, "zoom cascade"."""
import numpy as np
import pytest

from conftest import assert_psd_close
from test_gpu_cross import DETRENDS, assert_breaks
from test_zoom_host import (PARITY_CASES, U32_MAX, carrier_ftw, emul, mix_f32, noise, parity_input, restate_zoom,  # noqa: F401
                            stitch_zoom, windows_of)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", range(len(PARITY_CASES)))
def test_zoom_parity(pkg, ora, gpu_required, emul, case):  # noqa: F811
    n, wkind, detrend, avg, carrier, length = PARITY_CASES[case]
    pwin, owin = windows_of(pkg, n, wkind)
    avg = avg or (U32_MAX, U32_MAX)
    x = parity_input(n, length)
    ftw = carrier_ftw(pkg, n, carrier)
    g = pkg.ZoomCascade(n, ftw=ftw, window=pwin)
    g.set_detrend(DETRENDS[detrend])
    g.set_avg(pkg.AvgOpts(*avg))
    g.process(x)
    up, lo, br = g.psd()
    rup, rlo, rbr = stitch_zoom(pkg, n, pwin, restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg))
    assert br == rbr
    if detrend == "none":
        for name, got, want in (("upper", up, rup), ("lower", lo, rlo)):
            rel = assert_psd_close(got, want, f"zoom {name} case {case}", pure=True)
            print(f"case {case} {name}: worst relative error {rel:.3g}")
    else:  # a detrend nulls bin 0 of both rows: the widened bound, held to the complex64 sibling's own f32 arithmetic there
        sup, slo, _ = stitch_zoom(pkg, n, pwin, restate_zoom(ora, x, n, ftw, 0, owin, detrend, avg, "f32", iq=mix_f32(emul, x, ftw)))
        assert_psd_close(up, rup, f"zoom upper case {case} {detrend}", ref_f32=sup)
        assert_psd_close(lo, rlo, f"zoom lower case {case} {detrend}", ref_f32=slo)
    # stages and Breaks are those of the auto-PSD object fed x
    b = pkg.PsdCascadeBank(n, 1, pwin)
    b.set_detrend(DETRENDS[detrend])
    b.set_avg(pkg.AvgOpts(*avg))
    b.process(0, x)
    _, bbr = b.psd(0)
    assert bbr == br and g.num_stages() == b.num_stages(0)
    ref = ora.PsdCascade(n, "f64", window=owin)
    ref.set_detrend(detrend)
    ref.set_avg(*avg)
    ref.process(x)
    assert_breaks(br, ref.psd()[1])


def test_zoom_bin_aligned_and_zero_carrier_against_psdcascade(pkg, gpu_required):
    """A carrier on bin j permutes stage 0 of the auto-PSD object: upper[k] is its bin j + k, lower[k] its bin j - k.  ftw = 0 is
    the auto-PSD object itself on both rows, through every stage.  1e-5, as everywhere."""
    n, j = 1024, 137
    h = n // 2 + 1
    x = noise(1 << 20, 77)
    p = pkg.PsdCascade(n)
    p.process(x)
    s0 = p.stage_spectrum(0).astype(np.float64)
    z = pkg.ZoomCascade(n, ftw=(j << 64) // n)
    z.process(x)
    info, up, lo = z.stage_spectra(0)
    assert info["count"] == p.stage_count(0)
    ku, kl = np.arange(0, h - j), np.arange(0, j + 1)
    assert np.max(np.abs(up[ku] - s0[j + ku]) / s0[j + ku]) <= 1e-5
    assert np.max(np.abs(lo[kl] - s0[j - kl]) / s0[j - kl]) <= 1e-5
    z0 = pkg.ZoomCascade(n)
    z0.process(x)
    up, lo, br = z0.psd()
    pp, pbr = p.psd()
    assert br == pbr
    assert_psd_close(up, pp, "ftw = 0 upper vs PsdCascade", pure=True)
    assert_psd_close(lo, pp, "ftw = 0 lower vs PsdCascade", pure=True)


def test_zoom_reference_statistical_bound(pkg, gpu_required):
    """The reference's own test (src/psd.rs:623-643) on both rows: uniform noise of variance 1 reads 2 -- 0.5 p within 10 / sqrt(count)
    of 1 in every included bin."""
    n = 512
    x = pkg.noise_host(1 << 22, seed=0xC0FFEE)
    z = pkg.ZoomCascade(n, f0=0.2)
    z.process(x)
    up, lo, br = z.psd()
    assert len(br) >= 5
    for b in br:
        if not b.include or b.count == 0:  # (a stage below min_count contributes no bins)
            continue
        for name, row in (("upper", up), ("lower", lo)):
            p = row[b.start:b.start + b.bins.stop - b.bins.start].astype(np.float64)
            dev = np.max(np.abs(0.5 * p - 1.0))
            assert dev < 10.0 / np.sqrt(b.count), (name, b, dev)


def test_zoom_tone_image(pkg, ora, gpu_required, emul):  # noqa: F811
    """A tone at f0 + delta, delta the centre of bin 100 of stage 2: the peak is at offset delta in `upper`, and its image in
    `lower` is no larger, relative to the peak, than 4 x the worse of the f64 restatement's and the complex64 sibling's (the
    project's rule for f32 effects).  Printed beside them: the same image formed from a pair object fed (I, Q), Sii + Sqq + 2 Im
    Siq, whose terms f32 has rounded before they cancel."""
    n, k, b = 1024, 2, 100
    f0 = 0.2
    ftw, f0 = pkg.zoom_ftw(f0)
    delta = b / (n * 8.0 ** k)
    length = 1 << 20
    x = np.cos(2 * np.pi * ((f0 + delta) * np.arange(length, dtype=np.float64) % 1.0)).astype(np.float32)
    z = pkg.ZoomCascade(n, ftw=ftw)
    z.process(x)
    up, lo, br = z.psd()
    f = pkg.Break.frequencies(br)
    assert abs(f[int(np.argmax(up))] - delta) <= 0.5 / (n * 8.0 ** k)
    _, su, sl = z.stage_spectra(k)
    assert int(np.argmax(su)) == b
    gpu = float(sl[b]) / float(su[b])
    st64 = restate_zoom(ora, x, n, ftw)
    iq = mix_f32(emul, x, ftw)
    st32 = restate_zoom(ora, x, n, ftw, prec="f32", iq=iq)
    r64 = float(st64[k]["lower"][b] / st64[k]["upper"][b])
    r32 = float(st32[k]["lower"][b] / st32[k]["upper"][b])
    c = pkg.CsdCascade(n)
    c.process(iq[0], iq[1])
    _, sii, sqq, siq = c.stage_spectra(k)
    pair_up = float(sii[b]) + float(sqq[b]) - 2.0 * float(siq[b].imag)
    pair = abs(float(sii[b]) + float(sqq[b]) + 2.0 * float(siq[b].imag)) / pair_up
    print(f"image / peak at stage {k} bin {b}: GPU zoom {gpu:.3g}, f64 restatement {r64:.3g}, complex64 sibling {r32:.3g}, "
          f"pair object fed (I, Q) {pair:.3g}")
    assert gpu <= 4.0 * max(r64, r32), (gpu, r64, r32)


def same_psd(a, b, tol, what=""):
    """the bound of assert_same_csd (test_gpu_cross.py) on the two rows; tol 0: equal bits"""
    assert a[2] == b[2], what
    for u, v in zip(a[:2], b[:2]):
        if tol == 0:
            assert u.tobytes() == v.tobytes(), what
        else:
            assert np.all(np.abs(u - v) <= tol * v), what


def test_zoom_phase_continuity(pkg, gpu_required):
    """The phase comes from the 64-bit stream index: one call against calls of 1000, 77 777 and 2^20 + 3 samples, host and device,
    within the chunking bound of the pair object (2e-6); the same calls twice, host against device, and reset + replay: equal bits."""
    import torch
    n = 512
    cuts = np.cumsum([0, 1000, 77_777, (1 << 20) + 3])
    length = int(cuts[-1])
    x = noise(length, 31)
    ftw, ph0 = pkg.zoom_ftw(0.2718281828459045)[0], 0x0123456789ABCDEF
    one = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    one.process(x)
    ref = one.psd()
    a = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for s, e in zip(cuts[:-1], cuts[1:]):
        a.process(x[s:e])
    got_a = a.psd()
    same_psd(got_a, ref, 2e-6, "host chunks")
    dx = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    d = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    got_d = d.psd()
    same_psd(got_d, ref, 2e-6, "device chunks")
    same_psd(got_d, got_a, 0, "host against device, same calls")
    one_d = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    one_d.process_device(dx.data_ptr(), length)
    same_psd(one_d.psd(), ref, 0, "host against device, one call")
    a2 = pkg.ZoomCascade(n, ftw=ftw, phase0=ph0)
    for s, e in zip(cuts[:-1], cuts[1:]):
        a2.process(x[s:e])
    same_psd(a2.psd(), got_a, 0, "same calls twice")
    # a carrier is set before the first sample only
    with pytest.raises(pkg.PsdError) as err:
        d.set_carrier(ftw=1)
    assert err.value.code == pkg.ERR_ARG and "before the first" in str(err.value)
    # reset + replay == fresh (reset puts the bank's carrier back to the default; ZoomCascade sets its own again)
    d.set_detrend(3)
    d.reset()
    for s, e in zip(cuts[:-1], cuts[1:]):
        d.process_device(dx.data_ptr() + 4 * int(s), int(e - s))
    same_psd(d.psd(), got_d, 0, "reset + replay")
    assert d.stats_read()["samples_in"] == length
    bank = pkg.ZoomCascadeBank(n, 1)
    bank.set_carrier(0, ftw=ftw)
    bank.process(0, x[:10])
    bank.reset()
    bank.process(0, x[:50_000])
    z0 = pkg.ZoomCascade(n)
    z0.process(x[:50_000])
    same_psd(bank.psd(0), z0.psd(), 0, "a bank's reset puts the carrier back to 0")


def test_zoom_bank(pkg, gpu_required):
    """Four channels with four carriers against four single objects.  Bit for bit when every channel's rounds are those of its
    single object: a channel is fed its calls and read out before the next one starts (a round plans every channel with work, and
    where a round's segments are cut decides the order of the f32 partial sums).  Interleaved calls put a channel's decimated stages
    into other channels' rounds: the same spectra within the pair object's chunking bound (2e-6)."""
    n = 256
    lens = [300_000, 123_457, 1 << 18, 77_777]
    step = [10_000, 33_333, 65_536, 7_777]
    xs = [noise(m, 400 + i) for i, m in enumerate(lens)]
    car = [pkg.zoom_ftw(f)[0] for f in (0.2, 0.0123456789, 0.75, 0.4999)]
    ph = [0, 1 << 63, 12345, (1 << 64) - 1]
    singles = []
    for i in range(4):
        s = pkg.ZoomCascade(n, ftw=car[i], phase0=ph[i])
        for p in range(0, lens[i], step[i]):
            s.process(xs[i][p:p + step[i]])
        singles.append(s.psd())
    bank = pkg.ZoomCascadeBank(n, 4)
    for i in range(4):
        bank.set_carrier(i, ftw=car[i], phase0=ph[i])
    for i in range(4):
        for p in range(0, lens[i], step[i]):
            bank.process(i, xs[i][p:p + step[i]])
        same_psd(bank.psd(i), singles[i], 0, f"channel {i}, fed in turn")
    for i in range(4):
        same_psd(bank.psd(i), singles[i], 0, f"channel {i}, read again")
    mixed = pkg.ZoomCascadeBank(n, 4)
    for i in range(4):
        mixed.set_carrier(i, ftw=car[i], phase0=ph[i])
    pos = [0] * 4
    while any(pos[i] < lens[i] for i in range(4)):
        for i in range(4):
            if pos[i] < lens[i]:
                mixed.process(i, xs[i][pos[i]:pos[i] + step[i]])
                pos[i] += step[i]
    for i in range(4):
        same_psd(mixed.psd(i), singles[i], 2e-6, f"channel {i}, interleaved")
    with pytest.raises(pkg.PsdError) as e:
        bank.process(4, xs[0][:10])
    assert e.value.code == pkg.ERR_ARG and "out of range" in str(e.value)


def test_zoom_launch_count(pkg, gpu_required):
    """A steady-state device call is 1 + 3 launches (mixer; segments, decimators, fold + tails) at eight live stages."""
    import torch
    n = 1024
    m = 1 << 22
    dx = torch.randn(m, device="cuda")
    torch.cuda.synchronize()
    g = pkg.ZoomCascade(n, f0=0.2)
    for _ in range(512):  # 2^31 samples: eight stages
        g.process_device(dx.data_ptr(), m)
    g.stats_read(reset=True)
    for _ in range(8):
        g.process_device(dx.data_ptr(), m)
    assert g.stats_read()["launches"] == 4 * 8
    g.sync()
    assert g.num_stages() >= 8


def test_zoom_producer_event(pkg, gpu_required):
    """Samples made on a torch stream and handed over with an event (after=): the mixer waits for the producer on the device."""
    import torch
    n, m = 256, 1 << 20
    hx = noise(m, 300)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tx = torch.from_numpy(hx).pin_memory().cuda(non_blocking=True) * 1.0
        ev = torch.cuda.Event()
        ev.record(s)
    g = pkg.ZoomCascade(n, f0=0.3)
    g.process_device(tx.data_ptr(), m, after=ev.cuda_event)
    got = g.psd()
    h = pkg.ZoomCascade(n, f0=0.3)
    h.process(hx)
    same_psd(got, h.psd(), 0, "after=")
    s.synchronize()


def _cli(args, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _cli_bank(pkg, x, f0s):
    """what tools/psd_cli.py --zoom builds: ZoomCascade<512> with the reference's default AcqOpts (detrend mean, avg_max 1000)"""
    bank = pkg.ZoomCascadeBank(512, len(f0s))
    bank.set_detrend(pkg.Detrend.MEAN)
    bank.set_avg(pkg.AvgOpts(limit=999, count=0xFFFFFFFE))
    for i, f0 in enumerate(f0s):
        bank.set_carrier(i, f0=f0)
        bank.process(i, x[i])
    return bank


def test_zoom_cli_raw(pkg, gpu_required, tmp_path):
    """tools/psd_cli.py --raw FILE --zoom F0: the CSV (offset, upper, lower) and the printed lines against a ZoomCascadeBank fed the
    file's samples in one call (the tool feeds about 2^20 samples a call: the chunking bound, 2e-6)."""
    fs = 1000.0
    length = (1 << 21) + 777
    x = (noise(length, 41) + np.cos(2 * np.pi * 0.2001 * np.arange(length))).astype(np.float32)
    p = tmp_path / "raw.f32"
    x.astype("<f4").tofile(p)
    out = _cli(["--raw", str(p), "--fs", str(fs), "--zoom", "0.2", "--csv", str(tmp_path / "csv")], tmp_path)
    assert "zoom raw @ 0.2" in out
    d = np.loadtxt(tmp_path / "csv" / "zoom_raw_0_2.csv", delimiter=",")
    up, lo, br = _cli_bank(pkg, [x], [0.2]).psd(0)
    assert d.shape == (up.size, 3)
    assert np.allclose(d[:, 0], pkg.Break.frequencies(br) * fs, rtol=1e-6, atol=0)
    assert np.all(np.abs(d[:, 1] - up) <= 2e-6 * up + 1e-6 * np.mean(up)) and np.all(np.abs(d[:, 2] - lo) <= 2e-6 * lo + 1e-6 * np.mean(lo))
    assert abs(d[int(np.argmax(d[:, 1])), 0] - 0.0001 * fs) <= 0.5 * fs / (512 * 64)  # the tone, 1e-4 fs above the carrier
    # without --csv the lines go to stdout
    out = _cli(["--raw", str(p), "--zoom", "0.2"], tmp_path)
    rows = [ln for ln in out.splitlines() if ln.count(",") == 2]
    assert len(rows) == up.size and np.allclose([float(r.split(",")[1]) for r in rows], d[:, 1], rtol=1e-6)


def test_zoom_cli_frames(pkg, ora, gpu_required, tmp_path):
    """--file FRAMES --zoom F0:TRACE, by index and by label, through Source's host traces: against the oracle's decode of the frames"""
    import struct
    rng = np.random.default_rng(12)
    nb, fsz, nframes = 60, 1448, 700
    w = rng.integers(-(1 << 31), 1 << 31, size=(nframes, nb, 6), dtype=np.int64).astype(np.int32)
    frames = b"".join(bytes([0x7B, 0x05, 4, nb]) + struct.pack("<I", k * nb) + w[k].astype("<i4").tobytes() for k in range(nframes))
    p = tmp_path / "mpll.bin"
    p.write_bytes(frames)
    out = _cli(["--file", str(p), "--zoom", "0.125:1", "--zoom", "0.3:amplitude (V/G10)", "--csv", str(tmp_path / "csv")], tmp_path)
    traces = [[] for _ in range(3)]
    for k in range(nframes):
        st, _, _, _, tr = ora.frame_decode(frames[k * fsz:(k + 1) * fsz])
        assert st == 0
        for i, (_, v) in enumerate(tr):
            traces[i].append(v)
    xs = [np.concatenate(traces[1]).astype(np.float32), np.concatenate(traces[2]).astype(np.float32)]
    bank = _cli_bank(pkg, xs, [0.125, 0.3])
    for i, name in enumerate(("zoom_frequency__kHz__0_125.csv", "zoom_amplitude__V_G10__0_3.csv")):
        d = np.loadtxt(tmp_path / "csv" / name, delimiter=",")
        up, lo, br = bank.psd(i)
        assert d.shape == (up.size, 3) and np.allclose(d[:, 0], pkg.Break.frequencies(br), rtol=1e-6, atol=0)
        assert np.all(np.abs(d[:, 1] - up) <= 2e-6 * up + 1e-6 * np.mean(up)) and np.all(np.abs(d[:, 2] - lo) <= 2e-6 * lo + 1e-6 * np.mean(lo))
    assert "zoom frequency (kHz) @ 0.125" in out and "zoom amplitude (V/G10) @ 0.3" in out
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "psd_cli.py"), "--file", str(p), "--zoom", "0.1:nonesuch"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "unknown trace" in r.stderr
