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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_readout_probe.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readout_probe: no GPU is visible (there is nothing to measure without one)")
    pkg = entry.load_package()
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
