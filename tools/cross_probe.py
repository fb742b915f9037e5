"""Measure the cross-spectral cascade (psdc_cross_*): one JSON line.

    python tools/cross_probe.py [--seconds 0.5]

Legs: device-resident pairs at N = 512, 1024, 4096 with 1 and 4 pairs in 2^24-pair calls (warm-up, then a window of at
least --seconds timed on the host clock ending in psdc_cross_sync); kernel launches of one steady-state call; one
host-fed leg.  Roofline: 8 algorithmic bytes a pair (x and y read once) against 8 TB/s of HBM.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM = 8e12


def rate(pkg, torch, n, pairs, call, seconds):
    xs = [torch.randn(call, device="cuda") for _ in range(pairs)]
    ys = [(0.5 * x + torch.randn(call, device="cuda")) for x in xs]
    torch.cuda.synchronize()
    b = pkg.CsdCascadeBank(n, pairs)
    for _ in range(3):
        for p in range(pairs):
            b.process_device(p, xs[p].data_ptr(), ys[p].data_ptr(), call)
    # launches of steady-state calls: consecutive calls without a sync, so that every round has work in several stages
    b.stats_read(reset=True)
    for _ in range(8):
        for p in range(pairs):
            b.process_device(p, xs[p].data_ptr(), ys[p].data_ptr(), call)
    launches = b.stats_read()["launches"] / (8 * pairs)
    b.sync()
    # calibrate the number of calls, then ONE timed window of back-to-back calls that ends in psdc_cross_sync (its drain
    # rounds included once, as a caller's read-out would)
    t0 = time.perf_counter()
    for p in range(pairs):
        for _ in range(4):
            b.process_device(p, xs[p].data_ptr(), ys[p].data_ptr(), call)
    b.sync()
    per_call = (time.perf_counter() - t0) / (4 * pairs)
    rounds = max(4, int(seconds / (per_call * pairs)) + 1)
    while True:
        t0 = time.perf_counter()
        for _ in range(rounds):
            for p in range(pairs):
                b.process_device(p, xs[p].data_ptr(), ys[p].data_ptr(), call)
        b.sync()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
        rounds = int(rounds * 1.1 * seconds / dt) + 1  # (the calibration includes a drain: the window came out short)
    calls = rounds * pairs
    gps = calls * call / dt / 1e9
    return {"n": n, "pairs": pairs, "call": call, "calls": calls, "seconds": round(dt, 4), "gpairs_s": round(gps, 2),
            "launches_per_call": round(launches, 3), "stages": b.num_stages(0),
            "hbm_frac": round(gps * 1e9 * 8 / HBM, 4)}


def host_leg(pkg, n, call, seconds):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(call).astype(np.float32)
    y = rng.standard_normal(call).astype(np.float32)
    c = pkg.CsdCascade(n)
    c.process(x, y)
    c.sync()
    calls = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        c.process(x, y)
        calls += 1
    c.sync()
    dt = time.perf_counter() - t0
    return {"n": n, "call": call, "calls": calls, "seconds": round(dt, 4), "gpairs_s": round(calls * call / dt / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--call-log2", type=int, default=24)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    call = 1 << a.call_log2
    legs = [rate(pkg, torch, n, p, call, a.seconds) for n in (512, 1024, 4096) for p in (1, 4)]
    host = host_leg(pkg, 1024, 1 << 22, a.seconds)
    best = max(l["hbm_frac"] for l in legs)
    print(json.dumps({"metric": "cross_gpairs_s", "legs": legs, "host_fed": host,
                      "roofline": {"bytes_per_pair": 8, "hbm_bytes_s": HBM, "best_frac": best},
                      "n1024_1pair_gpairs_s": next(l["gpairs_s"] for l in legs if l["n"] == 1024 and l["pairs"] == 1)}))


if __name__ == "__main__":
    main()
