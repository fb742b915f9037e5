"""Measure the read-out of a whole PsdCascadeBank: psd(c) channel by channel against one bank read-out call.

    python tools/readout_probe.py [--seconds 0.5] [--reps 3] [--out profiles/bank_readout_probe.json]

A device-resident bank of C channels is fed until six stages are live in every channel, then ONLY read-outs are timed, with no
feed in the window (every read-out finds the pipeline idle):
  A  a loop of psd(c) over the C channels: 2 C stream synchronisations and C copy-out launches a read-out, stitched on the host;
  B  bankread.bank_psd: one launch, one copy, one synchronisation, host arrays;
  C  bankread.bank_psd_device into a torch tensor, the form that returns when the kernel has completed: one launch, one
     synchronisation, no copy.
C = 4 and 64 at N = 512, 1024 and 4096, in turns of A / B / A / C / A, --reps turns, each leg a window of at least --seconds on
the host clock.  All three go through the Python binding, as their callers do.  Reported: microseconds a read-out of all channels,
the rate ratios B / A and C / A of every turn (A: the mean of the turn's first two A legs for B, of its last two for C), and the
largest |A' - A| / A between two A legs of a turn.  B and C hand their Breaks back unbuilt (the Python objects are made when
`breaks` is first indexed; psd() builds them in every call): `breaks_us` is what building them once costs.  Findings, no gate.

    python tools/readout_probe.py --cross [--seconds 0.3] [--out profiles/cross_readout_probe.json]

The same for a CsdCascadeBank of P = 64 and 4 pairs at N = 1024, six live stages, read-outs only:
  A  a loop over the P pairs of csd(p) plus numpy coherence() and transfer(): per pair two stream synchronisations, one blocking
     copy a stage, four host stitches;
  B  crossread.bank_csd(coherence=True, transfer=True): one launch, one copy, one synchronisation, host arrays;
  C  crossread.bank_csd_device with the same five outputs into torch tensors, the form that returns when the kernel has completed.
Five turns of A / B / C / A.  Reported: the median microseconds a read-out of all pairs of each leg, the rate ratios against the
turn's two A legs, the largest |A' - A| / A of a turn, and `breaks_us`.  Findings, no gate.

    python tools/readout_probe.py --var [--seconds 0.3] [--out profiles/bank_var_probe.json]

The Var read-out (bankvar) of a PsdCascadeBank of C = 64 and 4 channels at N = 1024, six live stages, read-outs only, for T = 64 and
1024 taus (log-spaced from 1 to 10^6 samples) and for AVAR alone and AVAR + MVAR + FVAR:
  A  bankread.bank_psd(frequencies=True) plus the Python loop of var_eval over rows x descriptors x taus: the sequential f32 fold on
     the host, the only way there was;
  B  bankvar.bank_var: one launch, one copy of the curves, host arrays;
  C  bankvar.bank_var_device into a torch tensor, the form that returns when the kernel has completed.
A does f32 work and B / C do f64 work (one f64 sine a term where A takes one sinf): the comparison is of unequal arithmetic.  Five
turns of A / B / C / A; a leg is a window of at least --seconds, and at least one call (an A leg of the largest condition is one
call of several seconds).  Reported: the median microseconds a read-out of all channels of each leg, the rate ratios against the
turn's two A legs, the largest |A' - A| / A of a turn, and the largest |B - A| over the curves, relative to each curve's largest value (the f32 fold against f64).
Findings, no gate.

    python tools/readout_probe.py --carrier [--sk|--ampm] [--seconds 0.3] [--out profiles/carrier_readout_probe.json]
    python tools/readout_probe.py --pair-carrier [--ampm] [--seconds 0.3] [--out profiles/pair_readout_probe.json]

The carrier banks' read-outs (carrierread) of a zoom bank of C = 64 and 4 channels at N = 1024 with a carrier at the tuning word,
six live stages, read-outs only; the mode picks the bank: ZoomCascadeBank, with --sk ZoomSkCascadeBank, with --ampm
ZoomAmPmCascadeBank:
  A  the per-channel route over the C channels, unchanged in this build: psd(c); with --sk psd(c) and sk(c); with --ampm am_pm(c),
     which reads carrier() with a snapshot of stage 0 and then sidebands() with another.  Per call a drain, both streams
     synchronised, one blocking copy a stage, a host stitch;
  B  carrierread.bank_sides / bank_sk / bank_am_pm: one launch, one copy, one synchronisation, host arrays;
  C  the device form into torch tensors, the form that returns when the kernel has completed: upper and lower; with --sk also
     sk_upper and sk_lower; with --ampm s_am, s_pm, s_ampm and the carrier records.
Five turns of A / B / C / A.  Reported: the median microseconds a read-out of all channels of each leg, the rate ratios against the
turn's two A legs, the largest |A' - A| / A of a turn, and `breaks_us`: B and C hand their Breaks back unbuilt (the Python objects
are made when `breaks` is first indexed), A's calls build them every time.  The file keeps the three modes side by side; a run
replaces the rows of its own mode.  Findings, no gate.

--pair-carrier is the same for the pair carrier banks' read-outs (pairread) of P = 64 and 4 pairs: ZoomCsdCascadeBank, where A is
csd(p) plus numpy coherence() and transfer() of both sides, B pairread.bank_csd(coherence=True, transfer=True) and C the device form
with the same ten outputs; with --ampm ZoomAmPmCsdCascadeBank, where A is am_pm_cross(p) (carriers() with a snapshot of stage 0,
then sidebands() of twelve f64 rows, then numpy), B pairread.bank_am_pm_cross and C the device form with the four AM/PM rows and
the carrier records.  Not measured: the kernels' own time, the band kernels.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

STAGES = 6
CALL = 1 << 24  # samples a feed call


def window(fn, seconds):
    """microseconds a call of fn over a window of at least `seconds`"""
    fn()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e6 * dt / calls


def config(pkg, bankread, torch, n, channels, seconds, reps):
    bank = pkg.PsdCascadeBank(n, channels)
    x = torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5
    torch.cuda.synchronize()
    need = int(1.1 * n * 8 ** (STAGES - 1))
    for _ in range((need + CALL - 1) // CALL):
        for c in range(channels):
            bank.process_device(c, x.data_ptr(), CALL)
    bank.sync()
    lay = bankread.layout(bank)
    live = [sum(b.count > 0 for b in br) for br in lay["breaks"]]
    assert min(live) >= STAGES, live
    out = torch.empty((channels, lay["max_len"]), device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    legs = {"A": lambda: [bank.psd(c) for c in range(channels)],
            "B": lambda: bankread.bank_psd(bank),
            "C": lambda: bankread.bank_psd_device(bank, out.data_ptr(), lay["max_len"])}
    # the three give the same bytes before anything is timed
    a, b = legs["A"](), legs["B"]()
    legs["C"]()
    dev = out.cpu().numpy()
    for c in range(channels):
        assert a[c][0].tobytes() == b["psd"][c, :b["lens"][c]].tobytes() == dev[c, :b["lens"][c]].tobytes(), c
    turns = []
    for _ in range(reps):
        t = [window(legs[k], seconds) for k in "ABACA"]
        turns.append({"A_us": [t[0], t[2], t[4]], "B_us": t[1], "C_us": t[3], "B_over_A": 0.5 * (t[0] + t[2]) / t[1],
                      "C_over_A": 0.5 * (t[2] + t[4]) / t[3], "A_spread": max(abs(t[2] - t[0]) / t[0], abs(t[4] - t[2]) / t[2])})
    r = legs["B"]()
    t0 = time.perf_counter()
    list(r["breaks"])
    breaks_us = 1e6 * (time.perf_counter() - t0)
    bank.close()
    return {"n": n, "breaks_us": breaks_us, "channels": channels, "live_stages": min(live), "row_len": lay["max_len"], "launches_B": b["launches"], "turns": turns,
            "A_us": min(min(t["A_us"]) for t in turns), "B_us": min(t["B_us"] for t in turns), "C_us": min(t["C_us"] for t in turns),
            "B_over_A_min": min(t["B_over_A"] for t in turns), "C_over_A_min": min(t["C_over_A"] for t in turns),
            "A_spread_max": max(t["A_spread"] for t in turns)}


CROSS_TURNS = 5


def cross_config(pkg, crossread, torch, n, pairs, seconds):
    import statistics
    bank = pkg.CsdCascadeBank(n, pairs)
    x = torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5
    y = 0.6 * x + 0.8 * (torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5)
    torch.cuda.synchronize()
    need = int(1.1 * n * 8 ** (STAGES - 1))
    for _ in range((need + CALL - 1) // CALL):
        for p in range(pairs):
            bank.process_device(p, x.data_ptr(), y.data_ptr(), CALL)
    bank.sync()
    lay = crossread.layout(bank)
    live = [sum(b.count > 0 for b in br) for br in lay["breaks"]]
    assert min(live) >= STAGES, live
    width = lay["max_len"]
    f32 = {k: torch.empty((pairs, w * width), device="cuda", dtype=torch.float32) for k, w in (("sxx", 1), ("syy", 1), ("sxy", 2))}
    f64 = {k: torch.empty((pairs, w * width), device="cuda", dtype=torch.float64) for k, w in (("coherence", 1), ("transfer", 2))}
    ptrs = {k: t.data_ptr() for k, t in {**f32, **f64}.items()}
    torch.cuda.synchronize()

    def leg_a():
        out = []
        for p in range(pairs):
            sxx, syy, sxy, br = bank.csd(p)
            out.append((sxx, syy, sxy, br, pkg.coherence(sxx, syy, sxy), pkg.transfer(sxx, sxy)))
        return out

    legs = {"A": leg_a, "B": lambda: crossread.bank_csd(bank, coherence=True, transfer=True),
            "C": lambda: crossread.bank_csd_device(bank, width, **ptrs)}
    # the three give the same rows before anything is timed
    a, b = legs["A"](), legs["B"]()
    legs["C"]()
    dev = {k: t.cpu().numpy() for k, t in {**f32, **f64}.items()}
    for p in range(pairs):
        ln = b["lens"][p]
        assert a[p][0].tobytes() == b["sxx"][p, :ln].tobytes() == dev["sxx"][p, :ln].tobytes(), p
        assert a[p][2].tobytes() == b["sxy"][p, :ln].tobytes() == dev["sxy"][p, :2 * ln].tobytes(), p
        assert b["coherence"][p, :ln].tobytes() == dev["coherence"][p, :ln].tobytes(), p
    turns = []
    for _ in range(CROSS_TURNS):
        t = [window(legs[k], seconds) for k in "ABCA"]
        turns.append({"A_us": [t[0], t[3]], "B_us": t[1], "C_us": t[2], "B_over_A": 0.5 * (t[0] + t[3]) / t[1],
                      "C_over_A": 0.5 * (t[0] + t[3]) / t[2], "A_spread": abs(t[3] - t[0]) / t[0]})
    r = legs["B"]()
    t0 = time.perf_counter()
    list(r["breaks"])
    breaks_us = 1e6 * (time.perf_counter() - t0)
    bank.close()
    med = statistics.median
    return {"n": n, "pairs": pairs, "breaks_us": breaks_us, "live_stages": min(live), "row_len": width, "launches_B": b["launches"], "turns": turns,
            "A_us": med(v for t in turns for v in t["A_us"]), "B_us": med(t["B_us"] for t in turns), "C_us": med(t["C_us"] for t in turns),
            "B_over_A": med(t["B_over_A"] for t in turns), "C_over_A": med(t["C_over_A"] for t in turns),
            "A_spread_max": max(t["A_spread"] for t in turns)}


def window_warm(fn, seconds):
    """microseconds a call of fn over a window of at least `seconds` and at least one call; fn has been called before"""
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e6 * dt / calls


def var_bank(pkg, bankread, torch, n, channels):
    bank = pkg.PsdCascadeBank(n, channels)
    x = torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5
    torch.cuda.synchronize()
    need = int(1.1 * n * 8 ** (STAGES - 1))
    for _ in range((need + CALL - 1) // CALL):
        for c in range(channels):
            bank.process_device(c, x.data_ptr(), CALL)
    bank.sync()
    live = [sum(b.count > 0 for b in br) for br in bankread.layout(bank)["breaks"]]
    assert min(live) >= STAGES, live
    return bank, min(live)


def var_config(pkg, bankread, bankvar, torch, np, bank, live, n_taus, vs, seconds):
    import statistics
    channels = bank.n_channels
    taus = np.logspace(0, 6, n_taus).astype(np.float32)
    out = torch.empty((channels, len(vs), n_taus), device="cuda", dtype=torch.float64)
    torch.cuda.synchronize()

    def leg_a():
        r = bankread.bank_psd(bank, frequencies=True)
        curves = np.empty((channels, len(vs), n_taus))
        for c in range(channels):
            ln = r["lens"][c]
            p, f = r["psd"][c, :ln], r["frequencies"][c, :ln]
            for k, v in enumerate(vs):
                for j, tau in enumerate(taus):
                    curves[c, k, j] = pkg.var_eval(p, f, float(tau), v.x_exp, v.sinx_exp, v.clip, v.dc_cut)
        return curves

    legs = {"A": leg_a, "B": lambda: bankvar.bank_var(bank, taus, vs), "C": lambda: bankvar.bank_var_device(bank, out.data_ptr(), taus, vs)}
    a, b = legs["A"](), legs["B"]()
    legs["C"]()
    assert out.cpu().numpy().tobytes() == b["var"].tobytes()
    gap = float(np.max(np.abs(b["var"] - a) / np.maximum(np.max(np.abs(b["var"]), axis=-1, keepdims=True), 1e-300)))  # of a curve's largest value
    turns = []
    for _ in range(CROSS_TURNS):
        t = [window_warm(legs[k], seconds) for k in "ABCA"]
        turns.append({"A_us": [t[0], t[3]], "B_us": t[1], "C_us": t[2], "B_over_A": 0.5 * (t[0] + t[3]) / t[1],
                      "C_over_A": 0.5 * (t[0] + t[3]) / t[2], "A_spread": abs(t[3] - t[0]) / t[0]})
    med = statistics.median
    return {"n": bank.n, "channels": channels, "taus": n_taus, "vars": len(vs), "live_stages": live, "row_len": max(b["lens"]), "launches_B": b["launches"],
            "f32_fold_against_f64_max_rel": gap, "turns": turns,
            "A_us": med(v for t in turns for v in t["A_us"]), "B_us": med(t["B_us"] for t in turns), "C_us": med(t["C_us"] for t in turns),
            "B_over_A": med(t["B_over_A"] for t in turns), "C_over_A": med(t["C_over_A"] for t in turns),
            "A_spread_max": max(t["A_spread"] for t in turns)}


CARRIER_F0 = 0.25
CARRIER_CLASSES = {"sides": "ZoomCascadeBank", "sk": "ZoomSkCascadeBank", "ampm": "ZoomAmPmCascadeBank"}


def carrier_config(pkg, carrierread, torch, np, mode, n, channels, seconds):
    import statistics
    bank = getattr(pkg, CARRIER_CLASSES[mode])(n, channels)
    for c in range(channels):
        bank.set_carrier(c, f0=CARRIER_F0)
    j = np.arange(CALL, dtype=np.float64)  # (CALL * CARRIER_F0 is whole: every call continues the carrier's phase)
    x = torch.from_numpy((np.cos(2 * np.pi * CARRIER_F0 * j + 0.3)).astype(np.float32)).cuda()
    x += 0.01 * (torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5)
    torch.cuda.synchronize()
    need = int(1.1 * n * 8 ** (STAGES - 1))
    for _ in range((need + CALL - 1) // CALL):
        for c in range(channels):
            bank.process_device(c, x.data_ptr(), CALL)
    bank.sync()
    lay = carrierread.layout(bank)
    live = [sum(b.count > 0 for b in br) for br in lay["breaks"]]
    assert min(live) >= STAGES, live
    width = lay["max_len"]
    f32 = {k: torch.empty((channels, width), device="cuda", dtype=torch.float32) for k in ("upper", "lower")}
    f64 = {k: torch.empty((channels, w * width), device="cuda", dtype=torch.float64)
           for k, w in {"sides": (), "sk": (("sk_upper", 1), ("sk_lower", 1)), "ampm": (("s_am", 1), ("s_pm", 1), ("s_ampm", 2))}[mode]}
    if mode == "ampm":
        f64["carrier"] = torch.empty((channels, 4), device="cuda", dtype=torch.float64)
    tensors = {**f64} if mode == "ampm" else {**f32, **f64}  # (am_pm(c) returns no upper / lower: C writes none)
    ptrs = {k: t.data_ptr() for k, t in tensors.items()}
    torch.cuda.synchronize()
    # A: the parent's route for every channel, unchanged in this build
    leg_a = {"sides": lambda: [bank.psd(c) for c in range(channels)],
             "sk": lambda: [(bank.psd(c), bank.sk(c)) for c in range(channels)],
             "ampm": lambda: [bank.am_pm(c) for c in range(channels)]}[mode]
    host = {"sides": carrierread.bank_sides, "sk": carrierread.bank_sk, "ampm": carrierread.bank_am_pm}[mode]
    dev = {"sides": carrierread.bank_sides_device, "sk": carrierread.bank_sk_device, "ampm": carrierread.bank_am_pm_device}[mode]
    legs = {"A": leg_a, "B": lambda: host(bank), "C": lambda: dev(bank, width, **ptrs)}
    # the three agree before anything is timed: bytes for the f32 rows and SK, am_pm(c) to 1e-12 of a row's largest value
    a, b = legs["A"](), legs["B"]()
    legs["C"]()
    got = {k: t.cpu().numpy() for k, t in tensors.items()}
    for c in range(channels):
        ln = b["lens"][c]
        if mode == "sides":
            assert a[c][0].tobytes() == b["upper"][c, :ln].tobytes() == got["upper"][c, :ln].tobytes(), c
        elif mode == "sk":
            assert a[c][0][1].tobytes() == b["lower"][c, :ln].tobytes() == got["lower"][c, :ln].tobytes(), c
            assert a[c][1][0].tobytes() == b["sk_upper"][c, :ln].tobytes() == got["sk_upper"][c, :ln].tobytes(), c
        else:
            assert b["s_pm"][c, :ln].tobytes() == got["s_pm"][c, :ln].tobytes() and b["carrier"][c].tobytes() == got["carrier"][c].tobytes(), c
            # (at the carrier's own bins s_pm is the small difference of two large terms: the scale is s_am's there)
            assert np.max(np.abs(a[c][1] - b["s_pm"][c, :ln])) <= 1e-12 * max(np.max(np.abs(a[c][0])), np.max(np.abs(a[c][1]))), c
    turns = []
    for _ in range(CROSS_TURNS):
        t = [window(legs[k], seconds) for k in "ABCA"]
        turns.append({"A_us": [t[0], t[3]], "B_us": t[1], "C_us": t[2], "B_over_A": 0.5 * (t[0] + t[3]) / t[1],
                      "C_over_A": 0.5 * (t[0] + t[3]) / t[2], "A_spread": abs(t[3] - t[0]) / t[0]})
    r = legs["B"]()
    t0 = time.perf_counter()
    list(r["breaks"])
    breaks_us = 1e6 * (time.perf_counter() - t0)
    bank.close()
    med = statistics.median
    return {"mode": mode, "n": n, "channels": channels, "breaks_us": breaks_us, "live_stages": min(live), "row_len": width, "launches_B": b["launches"],
            "outputs_C": sorted(ptrs), "turns": turns,
            "A_us": med(v for t in turns for v in t["A_us"]), "B_us": med(t["B_us"] for t in turns), "C_us": med(t["C_us"] for t in turns),
            "B_over_A": med(t["B_over_A"] for t in turns), "C_over_A": med(t["C_over_A"] for t in turns),
            "A_spread_max": max(t["A_spread"] for t in turns)}


def carrier_main(a, torch, pkg):
    import numpy as np
    from stabilizer_stream_amd import carrierread
    mode = "sk" if a.sk else "ampm" if a.ampm else "sides"
    rows = [carrier_config(pkg, carrierread, torch, np, mode, 1024, c, a.seconds) for c in (64, 4)]
    path = a.out or os.path.join(ROOT, "profiles", "carrier_readout_probe.json")
    rec = {}
    if os.path.exists(path):  # (one file for the three modes: a run replaces its own mode's rows)
        with open(path) as f:
            rec = json.loads(f.read())
    rec.update({"metric": "carrier_readout_us",
                "unit": "microseconds a read-out of all channels, median of the turns (host clock, through the Python binding)",
                "note": "findings, no gate: A = the per-channel route over the channels (sides: psd(c); sk: psd(c) + sk(c); ampm: am_pm(c), which "
                        "reads carrier() and sidebands()), B = carrierread.bank_sides / bank_sk / bank_am_pm (host arrays), C = the device form "
                        "with the outputs named in outputs_C (synchronising form); a zoom bank with a carrier at the tuning word, read-outs "
                        "only, six live stages, no feed in the window; five turns of A / B / C / A; ratios are rates (above 1: faster than A); "
                        "B and C do not build the Python Break objects (breaks_us: building them once), A's calls do",
                "device": torch.cuda.get_device_name(0), "turns": CROSS_TURNS})
    rec.setdefault("modes", {})[mode] = {"seconds": a.seconds, "configs": rows}
    line = json.dumps(rec)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)
    for r in rows:
        print(f"{mode:5s} N={r['n']:5d} C={r['channels']:3d}  A {r['A_us']:9.1f} us  B {r['B_us']:8.1f} us  C {r['C_us']:8.1f} us  "
              f"B/A {r['B_over_A']:.2f}  C/A {r['C_over_A']:.2f}  A/A spread <= {r['A_spread_max']:.3f}  breaks {r['breaks_us']:.0f} us", file=sys.stderr)


def pair_config(pkg, pairread, torch, np, ampm, n, pairs, seconds):
    import statistics
    bank = (pkg.ZoomAmPmCsdCascadeBank if ampm else pkg.ZoomCsdCascadeBank)(n, pairs)
    for p in range(pairs):
        bank.set_carrier(p, f0=CARRIER_F0)
    j = np.arange(CALL, dtype=np.float64)  # (CALL * CARRIER_F0 is whole: every call continues the carriers' phases)
    x = torch.from_numpy((np.cos(2 * np.pi * CARRIER_F0 * j + 0.3)).astype(np.float32)).cuda()
    y = torch.from_numpy((np.cos(2 * np.pi * CARRIER_F0 * j + 0.8)).astype(np.float32)).cuda()
    x += 0.01 * (torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5)
    y += 0.01 * (torch.rand(CALL, device="cuda", dtype=torch.float32) - 0.5)
    torch.cuda.synchronize()
    need = int(1.1 * n * 8 ** (STAGES - 1))
    for _ in range((need + CALL - 1) // CALL):
        for p in range(pairs):
            bank.process_device(p, x.data_ptr(), y.data_ptr(), CALL)
    bank.sync()
    lay = pairread.layout(bank)
    live = [sum(b.count > 0 for b in br) for br in lay["breaks"]]
    assert min(live) >= STAGES, live
    width = lay["max_len"]
    if ampm:
        tensors = {k: torch.empty((pairs, 2 * width), device="cuda", dtype=torch.float64) for k in ("s_am", "s_pm", "s_am_pm", "s_pm_am")}
        tensors["carrier"] = torch.empty((pairs, 7), device="cuda", dtype=torch.float64)
    else:
        tensors = {k: torch.empty((pairs, w * width), device="cuda", dtype=torch.float32)
                   for k, w in (("saa_up", 1), ("saa_lo", 1), ("sbb_up", 1), ("sbb_lo", 1), ("sab_up", 2), ("sab_lo", 2))}
        tensors.update({k: torch.empty((pairs, w * width), device="cuda", dtype=torch.float64)
                        for k, w in (("coh_up", 1), ("coh_lo", 1), ("h1_up", 2), ("h1_lo", 2))})
    ptrs = {k: t.data_ptr() for k, t in tensors.items()}
    torch.cuda.synchronize()

    def leg_a_csd():  # the parent's route for every pair, unchanged in this build
        out = []
        for p in range(pairs):
            r = bank.csd(p)
            out.append((r, pkg.coherence(r[0], r[2], r[4]), pkg.coherence(r[1], r[3], r[5]), pkg.transfer(r[0], r[4]), pkg.transfer(r[1], r[5])))
        return out

    if ampm:
        legs = {"A": lambda: [bank.am_pm_cross(p) for p in range(pairs)], "B": lambda: pairread.bank_am_pm_cross(bank),
                "C": lambda: pairread.bank_am_pm_cross_device(bank, width, **ptrs)}
    else:
        legs = {"A": leg_a_csd, "B": lambda: pairread.bank_csd(bank, coherence=True, transfer=True),
                "C": lambda: pairread.bank_csd_device(bank, width, **ptrs)}
    # the three agree before anything is timed: bytes for the f32 rows, am_pm_cross(p) to 1e-12 of a row's largest value
    a, b = legs["A"](), legs["B"]()
    legs["C"]()
    got = {k: t.cpu().numpy() for k, t in tensors.items()}
    for p in range(pairs):
        ln = b["lens"][p]
        if ampm:
            assert b["s_pm"][p, :ln].tobytes() == got["s_pm"][p, :2 * ln].tobytes(), p
            assert np.max(np.abs(a[p][1] - b["s_pm"][p, :ln])) <= 1e-12 * max(np.max(np.abs(a[p][0])), np.max(np.abs(a[p][1]))), p
        else:
            assert a[p][0][0].tobytes() == b["saa_up"][p, :ln].tobytes() == got["saa_up"][p, :ln].tobytes(), p
            assert a[p][0][5].tobytes() == b["sab_lo"][p, :ln].tobytes() == got["sab_lo"][p, :2 * ln].tobytes(), p
            assert b["coherence_lo"][p, :ln].tobytes() == got["coh_lo"][p, :ln].tobytes(), p
    turns = []
    for _ in range(CROSS_TURNS):
        t = [window(legs[k], seconds) for k in "ABCA"]
        turns.append({"A_us": [t[0], t[3]], "B_us": t[1], "C_us": t[2], "B_over_A": 0.5 * (t[0] + t[3]) / t[1],
                      "C_over_A": 0.5 * (t[0] + t[3]) / t[2], "A_spread": abs(t[3] - t[0]) / t[0]})
    r = legs["B"]()
    t0 = time.perf_counter()
    list(r["breaks"])
    breaks_us = 1e6 * (time.perf_counter() - t0)
    bank.close()
    med = statistics.median
    return {"mode": "ampm" if ampm else "csd", "n": n, "pairs": pairs, "breaks_us": breaks_us, "live_stages": min(live), "row_len": width,
            "launches_B": b["launches"], "outputs_C": sorted(ptrs), "turns": turns,
            "A_us": med(v for t in turns for v in t["A_us"]), "B_us": med(t["B_us"] for t in turns), "C_us": med(t["C_us"] for t in turns),
            "B_over_A": med(t["B_over_A"] for t in turns), "C_over_A": med(t["C_over_A"] for t in turns),
            "A_spread_max": max(t["A_spread"] for t in turns)}


def pair_main(a, torch, pkg):
    import numpy as np
    from stabilizer_stream_amd import pairread
    mode = "ampm" if a.ampm else "csd"
    rows = [pair_config(pkg, pairread, torch, np, a.ampm, 1024, p, a.seconds) for p in (64, 4)]
    path = a.out or os.path.join(ROOT, "profiles", "pair_readout_probe.json")
    rec = {}
    if os.path.exists(path):  # (one file for the two modes: a run replaces its own mode's rows)
        with open(path) as f:
            rec = json.loads(f.read())
    rec.update({"metric": "pair_readout_us",
                "unit": "microseconds a read-out of all pairs, median of the turns (host clock, through the Python binding)",
                "note": "findings, no gate: A = the per-pair route over the pairs (csd: csd(p) + numpy coherence() and transfer() of both sides; "
                        "ampm: am_pm_cross(p), which reads carriers() and sidebands()), B = pairread.bank_csd(coherence, transfer) / "
                        "bank_am_pm_cross (host arrays), C = the device form with the outputs named in outputs_C (synchronising form); a zoom "
                        "bank with both carriers at the tuning word, read-outs only, six live stages, no feed in the window; five turns of "
                        "A / B / C / A; ratios are rates (above 1: faster than A); unequal Break work: B and C build the Python Break objects when "
                        "first indexed (breaks_us: building them once), A's calls always do; not measured: the kernels' own time, the band kernels",
                "device": torch.cuda.get_device_name(0), "turns": CROSS_TURNS})
    rec.setdefault("modes", {})[mode] = {"seconds": a.seconds, "configs": rows}
    line = json.dumps(rec)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)
    for r in rows:
        print(f"{mode:5s} N={r['n']:5d} P={r['pairs']:3d}  A {r['A_us']:9.1f} us  B {r['B_us']:8.1f} us  C {r['C_us']:8.1f} us  "
              f"B/A {r['B_over_A']:.2f}  C/A {r['C_over_A']:.2f}  A/A spread <= {r['A_spread_max']:.3f}  breaks {r['breaks_us']:.0f} us", file=sys.stderr)


def var_main(a, torch, pkg):
    import numpy as np
    from stabilizer_stream_amd import bankread, bankvar
    rows = []
    for channels in (64, 4):
        bank, live = var_bank(pkg, bankread, torch, 1024, channels)
        for n_taus in (64, 1024):
            for vs in ([bankvar.Var.avar()], [bankvar.Var.avar(), bankvar.Var.mvar(), bankvar.Var.fvar()]):
                rows.append(var_config(pkg, bankread, bankvar, torch, np, bank, live, n_taus, vs, a.seconds))
                r = rows[-1]
                print(f"N={r['n']:5d} C={r['channels']:3d} T={r['taus']:5d} V={r['vars']}  A {r['A_us']:11.1f} us  B {r['B_us']:9.1f} us  C {r['C_us']:9.1f} us  "
                      f"B/A {r['B_over_A']:.1f}  C/A {r['C_over_A']:.1f}  A/A spread <= {r['A_spread_max']:.3f}", file=sys.stderr, flush=True)
        bank.close()
    rec = {"metric": "bank_var_us", "unit": "microseconds a read-out of all channels, median of the turns (host clock, through the Python binding)",
           "note": "findings, no gate: A = bankread.bank_psd(frequencies) + the Python loop of var_eval over rows x descriptors x taus (the sequential "
                   "f32 fold on the host), B = bankvar.bank_var, C = bankvar.bank_var_device (synchronising form); A does f32 work and B / C do f64 "
                   "work: unequal arithmetic; read-outs only, six live stages, no feed in the window; taus log-spaced from 1 to 1e6 samples; "
                   "vars = 1: AVAR, 3: AVAR + MVAR + FVAR; five turns of A / B / C / A; ratios are rates (above 1: faster than A)",
           "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "turns": CROSS_TURNS, "configs": rows}
    line = json.dumps(rec)
    with open(a.out or os.path.join(ROOT, "profiles", "bank_var_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def cross_main(a, torch, pkg):
    from stabilizer_stream_amd import crossread
    rows = [cross_config(pkg, crossread, torch, 1024, p, a.seconds) for p in (64, 4)]
    rec = {"metric": "cross_readout_us", "unit": "microseconds a read-out of all pairs, median of the turns (host clock, through the Python binding)",
           "note": "findings, no gate: A = csd(p) + numpy coherence() and transfer() over the pairs, B = crossread.bank_csd(coherence, transfer), "
                   "C = crossread.bank_csd_device with the same five outputs (synchronising form); read-outs only, six live stages, no feed in the "
                   "window; five turns of A / B / C / A; ratios are rates (above 1: faster than A); B and C do not build the Python Break objects "
                   "(breaks_us: building them once), A's csd() does",
           "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "turns": CROSS_TURNS, "configs": rows}
    line = json.dumps(rec)
    with open(a.out or os.path.join(ROOT, "profiles", "cross_readout_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    for r in rows:
        print(f"N={r['n']:5d} P={r['pairs']:3d}  A {r['A_us']:9.1f} us  B {r['B_us']:8.1f} us  C {r['C_us']:8.1f} us  "
              f"B/A {r['B_over_A']:.2f}  C/A {r['C_over_A']:.2f}  A/A spread <= {r['A_spread_max']:.3f}  breaks {r['breaks_us']:.0f} us", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=None, help="a leg's window (default 0.5, with --cross and --var 0.3)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cross", action="store_true", help="measure the pair object's read-outs (crossread) instead")
    ap.add_argument("--var", action="store_true", help="measure the Var read-out (bankvar) against the host loop of var_eval instead")
    ap.add_argument("--carrier", action="store_true", help="measure the carrier banks' read-outs (carrierread) instead: the zoom bank's "
                                                           "sidebands, with --sk the zoom SK bank's SK, with --ampm the zoom AM/PM bank's split")
    ap.add_argument("--pair-carrier", action="store_true", help="measure the pair carrier banks' read-outs (pairread) instead: the zoom "
                                                                "cross bank's CSD, coherence and H1, with --ampm the zoom AM/PM cross bank's split")
    ap.add_argument("--sk", action="store_true")
    ap.add_argument("--ampm", action="store_true")
    ap.add_argument("--out", default=None, help="default profiles/bank_readout_probe.json, with --cross profiles/cross_readout_probe.json, "
                                                "with --var profiles/bank_var_probe.json, with --carrier profiles/carrier_readout_probe.json, "
                                                "with --pair-carrier profiles/pair_readout_probe.json")
    a = ap.parse_args()
    if (a.sk and not a.carrier) or (a.ampm and not (a.carrier or a.pair_carrier)) or (a.sk and a.ampm) or (a.carrier and a.pair_carrier):
        ap.error("--sk and --ampm select the mode of --carrier (--ampm also of --pair-carrier), one at a time")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readout_probe: no GPU is visible (there is nothing to measure without one)")
    pkg = entry.load_package()
    if a.seconds is None:
        a.seconds = 0.3 if a.cross or a.var or a.carrier or a.pair_carrier else 0.5
    if a.pair_carrier:
        return pair_main(a, torch, pkg)
    if a.carrier:
        return carrier_main(a, torch, pkg)
    if a.var:
        return var_main(a, torch, pkg)
    if a.cross:
        return cross_main(a, torch, pkg)
    a.out = a.out or os.path.join(ROOT, "profiles", "bank_readout_probe.json")
    from stabilizer_stream_amd import bankread
    rows = [config(pkg, bankread, torch, n, c, a.seconds, a.reps) for n in (512, 1024, 4096) for c in (4, 64)]
    rec = {"metric": "bank_readout_us", "unit": "microseconds a read-out of all channels (host clock, through the Python binding)",
           "note": "findings, no gate: A = psd(c) over the channels, B = bankread.bank_psd, C = bankread.bank_psd_device (synchronising "
                   "form); read-outs only, six live stages, no feed in the window; ratios are rates (above 1: faster than A); B and C do not build "
                   "the Python Break objects (breaks_us: building them once), A's psd() does",
           "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "reps": a.reps, "configs": rows}
    line = json.dumps(rec)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    for r in rows:
        print(f"N={r['n']:5d} C={r['channels']:3d}  A {r['A_us']:9.1f} us  B {r['B_us']:8.1f} us  C {r['C_us']:8.1f} us  "
              f"B/A >= {r['B_over_A_min']:.2f}  C/A >= {r['C_over_A_min']:.2f}  A/A spread <= {r['A_spread_max']:.3f}", file=sys.stderr)


if __name__ == "__main__":
    main()
