"""Cross-spectral matrix cascade (psdc_csm_*): the parts that run without a GPU.  Semantics: include/psdcascade.h,
"cross-spectral matrix cascade"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CSM_SYMBOLS = ["psdc_csm_supported", "psdc_csm_create", "psdc_csm_create_window", "psdc_csm_destroy", "psdc_csm_reset",
               "psdc_csm_set_detrend", "psdc_csm_set_avg", "psdc_csm_process", "psdc_csm_process_device",
               "psdc_csm_process_frames", "psdc_csm_process_frames_device", "psdc_csm_loss_read", "psdc_csm_sync",
               "psdc_csm_num_stages", "psdc_csm_stage_spectra", "psdc_csm_csd", "psdc_csm_stitch", "psdc_csm_stats_read",
               "psdc_csm_last_error"]


def csm_stitch(pkg, n, m, wt, counts, avgs, pendings, rows, opts):
    """(rows (m*m, len) f32, breaks) of psdc_csm_stitch on caller stages `rows` (n_stages, m*m, n/2 + 1)."""
    L = pkg.lib()
    ns = len(counts)
    h = n // 2 + 1
    c64 = (C.c_uint64 * max(1, ns))(*[int(c) for c in counts])
    aa = (C.c_uint32 * max(1, ns))(*[int(a) for a in avgs])
    pp = (C.c_uint64 * max(1, ns))(*[int(p) for p in pendings])
    r = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1) if ns else np.zeros(m * m * h, np.float32)
    cap = max(1, ns * h)
    out = np.empty((m * m, cap), np.float32)
    br = (pkg._CBreak * max(1, ns))()
    ln, nb = C.c_size_t(), C.c_size_t()
    rc = L.psdc_csm_stitch(n, m, wt.power, wt.nenbw, wt.overlap, ns, c64, aa, pp, pkg._fptr(r), int(opts.keep_overlap),
                           opts.min_count, int(opts.keep_transition_band), pkg._fptr(out), cap, C.byref(ln), br, ns, C.byref(nb))
    assert rc == 0, L.psdc_csm_last_error(None)
    return out[:, :ln.value].copy(), [pkg.Break._from_c(br[i]) for i in range(nb.value)]


def test_csm_exports(pkg):
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    declared = set(re.findall(r"\b(psdc_csm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CSM_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (psdc_csm_[a-z0-9_]+)", out))
    assert exported == declared
    assert declared <= set(pkg.EXPORTS)
    # the row layout is written down
    assert "row a*m + a is S_aa" in hdr and "row a*m + b is" in hdr and "row b*m + a is Im S_ab" in hdr
    assert "xx, re, im, yy" in hdr


def test_csm_supported(pkg):
    L = pkg.lib()
    for m in (2, 3, 4):
        for n in (64, 128, 256, 512, 1024, 2048):
            assert L.psdc_csm_supported(n, m) == 1, (n, m)
    assert L.psdc_csm_supported(4096, 2) == 1
    for n, m in ((1024, 1), (1024, 5), (32, 2), (8192, 2), (1000, 3), (0, 2), (1024, 0)):
        assert L.psdc_csm_supported(n, m) == 0, (n, m)
    # what the header states for 4096 at m = 3, 4 is what the function says
    hdr = open(os.path.join(ROOT, "include", "psdcascade.h")).read()
    assert "4096 for m = 2 and m = 3" in hdr
    assert (L.psdc_csm_supported(4096, 3), L.psdc_csm_supported(4096, 4)) == (1, 0)
    assert pkg.csm_supported(1024, 4) and not pkg.csm_supported(4096, 4)


def test_csm_refused_size_names_itself(pkg):
    L = pkg.lib()
    for n, m in ((4096, 4), (1000, 3), (32, 2), (8192, 2), (1024, 5), (1024, 1)):
        assert not L.psdc_csm_create(n, 1, m, 1, 0)
        msg = L.psdc_csm_last_error(None).decode()
        assert msg.startswith("psdc_csm_create: ") and (f"n = {n}" in msg or f"m = {m}" in msg), msg
        with pytest.raises(pkg.PsdError) as e:
            pkg.CsmCascadeBank(n, m)
        assert e.value.code == pkg.ERR_ARG
    w = np.ones(256, np.float32)
    assert not L.psdc_csm_create_window(256, pkg._fptr(w), 1.0, 1.0, 4, 3, 1, 0)
    assert "overlap" in L.psdc_csm_last_error(None).decode()
    assert not L.psdc_csm_create_window(256, None, 1.0, 1.0, 0, 3, 1, 0)
    assert "null window" in L.psdc_csm_last_error(None).decode()


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("seed", range(4))
def test_csm_stitch_exact(pkg, m, seed):
    """psdc_csm_stitch == psdc_stitch_window on each of the m*m rows, bit for bit, Breaks field by field."""
    rng = np.random.default_rng(100 * m + seed)
    n = int(rng.choice([64, 256, 1024, 2048]))
    h = n // 2 + 1
    wt = pkg.WindowTable.hann(n) if seed % 2 == 0 else pkg.WindowTable.rectangular(n)
    ns = int(rng.integers(1, 9))
    counts = [int(c) for c in rng.integers(0, 5000, ns)]
    if seed == 3:
        counts[0] = (1 << 33) + 7  # 64-bit counts
    avgs = [int(a) for a in rng.integers(1, 1 << 20, ns)]
    pend = [int(p) for p in rng.integers(0, n, ns)]
    rows = rng.standard_normal((ns, m * m, h)).astype(np.float32)
    for a in range(m):
        rows[:, a * m + a] = np.abs(rows[:, a * m + a])
    opts = pkg.MergeOpts(keep_overlap=bool(rng.integers(2)), min_count=int(rng.integers(0, 3000)),
                         keep_transition_band=bool(rng.integers(2)))
    got, br = csm_stitch(pkg, n, m, wt, counts, avgs, pend, rows, opts)
    for r in range(m * m):
        want, wbr = pkg.stitch(n, counts, avgs, pend, rows[:, r], opts, window=wt)
        assert got[r].tobytes() == want.tobytes(), r
        assert br == wbr


def test_csm_null_handles(pkg):
    L = pkg.lib()
    ok = C.c_size_t(77)
    st = C.c_uint64()
    loss = pkg._CLoss()
    nul = C.POINTER(C.c_uint32)()
    calls = {
        "psdc_csm_reset": lambda: L.psdc_csm_reset(None),
        "psdc_csm_set_detrend": lambda: L.psdc_csm_set_detrend(None, 0),
        "psdc_csm_set_avg": lambda: L.psdc_csm_set_avg(None, 1, 1),
        "psdc_csm_process": lambda: L.psdc_csm_process(None, 0, None, 4),
        "psdc_csm_process_device": lambda: L.psdc_csm_process_device(None, 0, None, 4, None),
        "psdc_csm_process_frames": lambda: L.psdc_csm_process_frames(None, nul, None, 16, 1, C.byref(ok)),
        "psdc_csm_process_frames_device": lambda: L.psdc_csm_process_frames_device(None, nul, None, 16, 1, C.byref(ok), None),
        "psdc_csm_loss_read": lambda: L.psdc_csm_loss_read(None, C.byref(loss), 0),
        "psdc_csm_sync": lambda: L.psdc_csm_sync(None),
        "psdc_csm_num_stages": lambda: L.psdc_csm_num_stages(None, 0),
        "psdc_csm_stage_spectra": lambda: L.psdc_csm_stage_spectra(None, 0, 0, None, None),
        "psdc_csm_csd": lambda: L.psdc_csm_csd(None, 0, 0, 1, 0, None, 0, None, None, 0, None),
        "psdc_csm_stats_read": lambda: L.psdc_csm_stats_read(None, C.byref(st), None, 0),
    }
    for name, call in calls.items():
        ok.value = 77
        assert call() == pkg.ERR_ARG, name
        assert L.psdc_csm_last_error(None).decode() == f"{name}: null handle"
        if "frames" in name:
            assert ok.value == 0, name
    L.psdc_csm_destroy(None)
    assert L.psdc_csm_stitch(64, 3, 1.0, 1.0, 0, 2, None, None, None, None, 0, 1, 0, None, 0, None, None, 0, None) == pkg.ERR_ARG
    assert "null input" in L.psdc_csm_last_error(None).decode()
    assert L.psdc_csm_stitch(64, 5, 1.0, 1.0, 0, 0, None, None, None, None, 0, 1, 0, None, 0, None, None, 0, None) == pkg.ERR_ARG


def test_group_map(pkg):
    none = pkg.TRACE_NONE
    m = pkg.group_map([("ADC0", "ADC1", "DAC0", "DAC1")], 4, 1)
    assert m.dtype == np.uint32 and m.tolist() == [0, 1, 2, 3]
    m = pkg.group_map([None, ("phase (rad)", 2, "frequency (kHz)")], 3, 3)
    assert m.tolist() == [none] * 3 + [0, 2, 1] + [none] * 3
    assert pkg.group_map([], 2, 2).tolist() == [none] * 4
    with pytest.raises(pkg.PsdError) as e:
        pkg.group_map([(0, 1), (1, 2)], 2, 1)
    assert e.value.code == pkg.ERR_ARG and "2 groups for a bank of 1" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        pkg.group_map([(0, 1)], 3, 1)
    assert e.value.code == pkg.ERR_ARG and "m = 3" in str(e.value)
    with pytest.raises(pkg.PsdError) as e:
        pkg.group_map([("ADC0", "nope")], 2, 1)
    assert e.value.code == pkg.ERR_ARG and "unknown trace label" in str(e.value)


def test_csm_matrix_layout(pkg):
    """csm_matrix reads the header's row layout: Hermitian, real diagonal, both sides filled."""
    rng = np.random.default_rng(2)
    for m in (2, 3, 4):
        rows = rng.standard_normal((m * m, 9)).astype(np.float32)
        S = pkg.csm_matrix(rows, m)
        assert S.shape == (m, m, 9) and S.dtype == np.complex64
        for a in range(m):
            assert np.array_equal(S[a, a].real, rows[a * m + a]) and np.all(S[a, a].imag == 0)
            for b in range(a + 1, m):
                assert np.array_equal(S[a, b].real, rows[a * m + b]) and np.array_equal(S[a, b].imag, rows[b * m + a])
                assert np.array_equal(S[b, a], np.conj(S[a, b]))


def test_mimo_transfer_and_multiple_coherence(pkg):
    """Synthetic matrices in f64: random Hermitian positive-definite S_xx (2 inputs), random H (2 outputs), uncorrelated output
    noise of known power P: S_xy = S_xx H^T, S_yy = conj(H) S_xx H^T + P."""
    rng = np.random.default_rng(11)
    bins, ni, no = 40, 2, 2
    S = np.zeros((ni + no, ni + no, bins), np.complex128)
    Ht = rng.standard_normal((no, ni, bins)) + 1j * rng.standard_normal((no, ni, bins))
    P = rng.uniform(0.1, 2.0, (no, bins))
    for k in range(bins):
        a = rng.standard_normal((ni, ni)) + 1j * rng.standard_normal((ni, ni))
        sxx = a.conj().T @ a + 0.5 * np.eye(ni)
        sxy = sxx @ Ht[:, :, k].T
        syy = Ht[:, :, k].conj() @ sxx @ Ht[:, :, k].T + np.diag(P[:, k])
        S[:ni, :ni, k], S[:ni, ni:, k], S[ni:, :ni, k], S[ni:, ni:, k] = sxx, sxy, sxy.conj().T, syy
    H = pkg.mimo_transfer(S, [0, 1], [2, 3])
    assert H.shape == (no, ni, bins) and H.dtype == np.complex128
    assert np.max(np.abs(H - Ht) / np.abs(Ht)) <= 1e-9
    for o in range(no):
        mc = pkg.multiple_coherence(S, [0, 1], ni + o)
        want = 1 - P[o] / S[ni + o, ni + o].real
        assert np.max(np.abs(mc - want)) <= 1e-9
        assert np.all(mc >= -1e-12) and np.all(mc <= 1 + 1e-12)
    # one input: transfer() and coherence()
    for i in range(ni):
        for o in range(no):
            h1 = pkg.mimo_transfer(S, [i], [ni + o])[0, 0]
            assert np.max(np.abs(h1 - pkg.transfer(S[i, i].real, S[i, ni + o])) / np.abs(h1)) <= 1e-12
            c1 = pkg.multiple_coherence(S, [i], ni + o)
            assert np.max(np.abs(c1 - pkg.coherence(S[i, i].real, S[ni + o, ni + o].real, S[i, ni + o]))) <= 1e-12
    # the single-input estimate of a correlated pair of inputs is biased, the multi-input one is not
    assert np.max(np.abs(pkg.transfer(S[0, 0].real, S[0, 2]) - Ht[0, 0])) > 1e-3


def test_csm_lane_emulation(tmp_path):
    """The matrix kernel's per-bin arithmetic (csrc/csm_fft.h) against an f64 DFT for M = 2, 3, 4."""
    exe = str(tmp_path / "csm_emul")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "csm_emul.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]


def test_csm_no_gpu_fails_loudly(pkg):
    from conftest import has_gpu
    if has_gpu():
        pytest.skip("a HIP device is visible")
    with pytest.raises(pkg.PsdError) as e:
        pkg.CsmCascade(1024, 3)
    assert e.value.code == pkg.ERR_DEVICE and "no CPU fallback" in str(e.value)
