"""Wave census of a team-kernel launch (GPU box; tools/stamps/build_census.sh builds the library): runs the bench's round -- 16
spans of 2^26 samples at N = 1024 unless told otherwise -- a few times and reduces the records the wavefronts of the LAST launch
left (csrc/fused.hip, PSDK_CENSUS): how long the launch took, what share of it its compute wavefronts were resident, how they
started, when they left -- by wave slot, wave index, workgroup placement, SE, XCD and job -- and where the empty slot-time went.

    python tools/stamps/census.py [--lib tools/stamps/libpsdcascade_census.so] [--n 1024] [--log2 26] [--spans 16] [--min-run 200] [--json OUT]

`reduce_census` is a pure function of the record array (tests/test_census_reduce.py feeds it a synthetic launch)."""
import argparse
import json
import os
import sys

import numpy as np

TICK_US = 0.01  # s_memrealtime: 100 MHz
WORDS = 8
MAX_WAVES = 8192
# share of the vector issue rate of four resident wavefronts that a SIMD reaches with fewer (three waves/SIMD
# measured -21 %, two at most 0.76 of the rate -- 0.6 taken --, one 0.35 taken)
ISSUE_RATE = {4: 1.0, 3: 0.79, 2: 0.6, 1: 0.35}


def decode(rec):
    """(W, 8) uint64 records -> dict of int64 columns, empty records dropped"""
    rec = np.asarray(rec, dtype=np.uint64).reshape(-1, WORDS)
    lo = lambda w: (w & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hi = lambda w: (w >> np.uint64(32)).astype(np.int64)
    s32 = lambda v: np.where(v >= 1 << 31, v - (1 << 32), v)
    kind = hi(rec[:, 5])
    keep = kind != 0
    rec, kind = rec[keep], kind[keep]
    lvl_first, lvl_last = (kind >> 8) & 15, (kind >> 12) & 15  # PSDK_FAIR_FB: level + 1 of the first / last decision (0: none, 4: rotation)
    kind = kind & 0xFF
    hw = lo(rec[:, 3])
    return {
        "entry": rec[:, 0].astype(np.int64), "first": rec[:, 1].astype(np.int64), "exit": rec[:, 2].astype(np.int64),
        "slot": hw & 15, "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7,
        "xcd": hi(rec[:, 3]) & 15, "wg": lo(rec[:, 4]), "wave": hi(rec[:, 4]), "job": s32(lo(rec[:, 5])), "kind": kind,
        "run": s32(lo(rec[:, 6])), "nrun": np.maximum(s32(hi(rec[:, 6])), 0), "npairs": s32(lo(rec[:, 7])), "grid": hi(rec[:, 7]),
        "lvl_first": lvl_first, "lvl_last": lvl_last,
    }


def _dist(x):
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return None
    q = np.percentile(x, [10, 50, 90])
    return {"n": int(x.size), "mean": float(x.mean()), "p10": float(q[0]), "p50": float(q[1]), "p90": float(q[2]),
            "min": float(x.min()), "max": float(x.max())}


def _groups(keys, frac):
    return {str(k): _dist(frac[keys == k]) for k in np.unique(keys)}


def reduce_census(rec):
    """The census of one launch.  Times in microseconds, exits and losses as fractions of the launch span (first entry of
    any wavefront to the last exit of a compute wavefront).  The empty slot-time of the compute wavefronts, 1 - residency, is
    split four ways, and the four add up to it:
      quantisation  a wavefront whose run is shorter than the launch's longest leaves early by (1 - nrun / longest) of the mean
                    lifetime of the full-run wavefronts (never more than its own tail)
      within_simd   the rest of its tail up to the last exit of ITS SIMD: the SIMD still had wavefronts, fewer than it holds
      empty_simd    from its SIMD's last exit to the end of the launch: differences between SIMDs, CUs, SEs, XCDs
      ramp          from the first entry of the launch to its own"""
    d = decode(rec)
    if d["grid"].size:  # one launch: the records of the commonest grid (the export clears them, a later launch of a round overwrites)
        g, n_ = np.unique(d["grid"], return_counts=True)
        d = {k: v[d["grid"] == g[np.argmax(n_)]] for k, v in d.items()}
    comp = d["kind"] == 1
    if not comp.any():
        raise ValueError("no compute wavefront in the records")
    c = {k: v[comp] for k, v in d.items()}
    t0 = int(d["entry"].min())
    t_end = int(c["exit"].max())
    span = float(t_end - t0)
    w = c["exit"].size
    life = (c["exit"] - c["entry"]).astype(np.float64)
    frac = (c["exit"] - t0) / span
    out = {"grid": int(c["grid"].max()), "compute_waves": int(w), "aux_waves": int((~comp).sum()),
           "span_us": span * TICK_US, "residency": float(life.sum() / (w * span)),
           "slots_seen": sorted(int(s) for s in np.unique(c["slot"]))}
    ent = (c["entry"] - t0) * TICK_US
    out["start_ramp_us"] = _dist(ent)
    out["warmup_us"] = _dist((c["first"] - c["entry"]) * TICK_US)
    # a job's stage: the jobs of a round hold an eighth of the pairs of the stage before, so rank them by length
    order = {j: r for r, j in enumerate(sorted(set(c["job"].tolist()), key=lambda j: -int(c["npairs"][c["job"] == j][0])))}
    rank = np.array([order[j] for j in c["job"].tolist()])
    stage = np.zeros(w, dtype=np.int64)
    np_of = {r: int(c["npairs"][rank == r][0]) for r in set(rank.tolist())}
    longest = max(np_of.values())
    for r, n_ in np_of.items():
        s, m = 0, longest
        while m >= 4 * max(n_, 1) and s < 30:  # (an eighth a stage: 4 splits two neighbours, spans of different lengths aside)
            m //= 8
            s += 1
        stage[rank == r] = s
    # placement: which of the workgroups that ran on a CU came first (by its earliest entry)
    cu_id = ((c["xcd"] * 8 + c["se"]) * 2 + c["sh"]) * 16 + c["cu"]
    simd_id = cu_id * 4 + c["simd"]
    placed = np.zeros(w, dtype=np.int64)
    for u in np.unique(cu_id):
        m = cu_id == u
        wgs = sorted(set(c["wg"][m].tolist()), key=lambda g: int(c["entry"][m & (c["wg"] == g)].min()))
        for i, g in enumerate(wgs):
            placed[m & (c["wg"] == g)] = i
    out["exit_frac"] = {
        "all": _dist(frac), "by_slot": _groups(c["slot"], frac), "by_wave_half": _groups((c["wave"] >= 4).astype(int), frac),
        "by_placement": _groups(placed, frac), "by_se": _groups(c["se"], frac),
        "by_xcd": _groups(c["xcd"], frac), "by_stage": _groups(stage, frac), "by_nrun": _groups(c["nrun"], frac),
    }
    # the spread inside a SIMD: full-run wavefronts only, so that a shorter run is not counted as an early exit
    nmax = int(c["nrun"].max())
    full = c["nrun"] == nmax
    simd_last = np.zeros(w, dtype=np.int64)
    spreads, rank_exit, ideal, late = [], {}, [], []
    for u in np.unique(simd_id):
        m = simd_id == u
        simd_last[m] = c["exit"][m].max()
        mf = m & full
        if mf.sum() >= 2:
            e = np.sort(c["exit"][mf])
            spreads.append((e[-1] - e[0]) / span)
            for i, x in enumerate(e):
                rank_exit.setdefault(i, []).append((x - t0) / span)
        if mf.sum() == 4:  # the bound of equal progress: the same work at the issue rate of four, all four leaving together
            s0 = float(c["entry"][mf].min())
            edges = np.concatenate(([s0], e.astype(np.float64)))
            work = float(sum(ISSUE_RATE[4 - k] * (edges[k + 1] - edges[k]) for k in range(4)))
            ideal.append((s0 + work / ISSUE_RATE[4] - t0) / span)
            late.append((e[-1] - s0 - work / ISSUE_RATE[4]) / span)
    out["simd_exit_spread"] = _dist(spreads)
    out["simd_exit_by_order"] = {str(i): _dist(v) for i, v in sorted(rank_exit.items())}
    # (SIMDs with exactly four full-run wavefronts; the last exit of such a SIMD against the exit all four would share)
    out["equal_progress_bound"] = {"issue_rate": {str(k): v for k, v in ISSUE_RATE.items()}, "ideal_common_exit": _dist(ideal),
                                   "last_exit_minus_ideal": _dist(late)}
    if c["lvl_last"].any():  # PSDK_FAIR_FB: the levels of the first and the last decision of a run, by wave slot
        name = {1: "0", 2: "1", 3: "2", 4: "rotation"}
        tab = lambda col: {str(s): {name[int(k)]: int(n_) for k, n_ in zip(*np.unique(col[(c["slot"] == s) & (col != 0)], return_counts=True))}
                           for s in np.unique(c["slot"])}
        out["feedback_levels"] = {"first": tab(c["lvl_first"]), "last": tab(c["lvl_last"])}
    out["waves_per_simd"] = _dist(np.unique(simd_id, return_counts=True)[1])
    mean_full = float(life[full].mean())
    tail = (t_end - c["exit"]).astype(np.float64)
    quant = np.minimum(tail, (1.0 - c["nrun"] / max(nmax, 1)) * mean_full)
    inside = np.maximum(0.0, np.minimum(tail - quant, (simd_last - c["exit"]).astype(np.float64)))
    empty = tail - quant - inside
    ramp = (c["entry"] - t0).astype(np.float64)
    den = w * span
    out["loss"] = {"total": 1.0 - out["residency"], "quantisation": float(quant.sum() / den), "within_simd": float(inside.sum() / den),
                   "empty_simd": float(empty.sum() / den), "ramp": float(ramp.sum() / den)}
    out["quantisation_by_construction"] = float(1.0 - c["nrun"].sum() / (w * max(nmax, 1)))
    out["runs"] = {str(k): int(v) for k, v in zip(*np.unique(c["nrun"], return_counts=True))}
    return out


def report(r, file=sys.stdout):
    p = lambda *a: print(*a, file=file)
    p(f"grid {r['grid']} workgroups: {r['compute_waves']} compute + {r['aux_waves']} aux wavefronts; span {r['span_us']:.1f} us; "
      f"RESIDENCY {r['residency']:.4f}; wave slots seen {r['slots_seen']}; runs (pairs: waves) {r['runs']}")
    s = r["start_ramp_us"]
    p(f"start ramp us: p50 {s['p50']:.2f} p90 {s['p90']:.2f} max {s['max']:.2f}; warm-up us p50 {r['warmup_us']['p50']:.2f}")
    for name, g in r["exit_frac"].items():
        if name == "all":
            p(f"exit (fraction of span) all: mean {g['mean']:.4f} p10 {g['p10']:.4f} p50 {g['p50']:.4f} p90 {g['p90']:.4f} min {g['min']:.4f}")
            continue
        p(f"  {name}: " + "  ".join(f"{k}: {v['mean']:.4f} [{v['p10']:.3f} {v['p90']:.3f}] n={v['n']}" for k, v in g.items()))
    sp = r["simd_exit_spread"]
    if sp:
        p(f"exit spread inside a SIMD (full runs, last - first, fraction of span): mean {sp['mean']:.4f} p50 {sp['p50']:.4f} p90 {sp['p90']:.4f} max {sp['max']:.4f}")
        p("  exit by order within the SIMD: " + "  ".join(f"{k}: {v['mean']:.4f}" for k, v in r["simd_exit_by_order"].items()))
    b = r.get("equal_progress_bound")
    if b and b["ideal_common_exit"]:
        p(f"equal progress (SIMDs of four full runs, n={b['ideal_common_exit']['n']}): ideal common exit p50 {b['ideal_common_exit']['p50']:.4f}, "
          f"last exit - ideal mean {b['last_exit_minus_ideal']['mean']:.4f} p50 {b['last_exit_minus_ideal']['p50']:.4f} of the span")
    for when, t in r.get("feedback_levels", {}).items():
        p(f"  feedback level at the {when} decision, by slot: {t}")
    lo = r["loss"]
    p(f"empty slot-time {lo['total']:.4f} = quantisation {lo['quantisation']:.4f} (by construction {r['quantisation_by_construction']:.4f}) "
      f"+ within SIMD {lo['within_simd']:.4f} + empty SIMD {lo['empty_simd']:.4f} + ramp {lo['ramp']:.4f}")


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(root, "tools", "stamps", "libpsdcascade_census.so"))
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--log2", type=int, default=26)
    ap.add_argument("--spans", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--min-run", type=int, default=200, help="record launches with a job in runs of this many pairs or more")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C
    sys.path.insert(0, root)
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.LIB_PATH = os.path.abspath(a.lib)
    L = pkg.lib()
    total = 1 << a.log2
    x = torch.empty(total, dtype=torch.float32, device="cuda:0")
    pkg.fill_noise_device(x.data_ptr(), total, seed=0x7654321)
    torch.cuda.synchronize()
    bank = pkg.PsdCascadeBank(a.n, n_channels=1)
    out = np.zeros((MAX_WAVES, WORDS), dtype=np.uint64)
    ptr = out.ctypes.data_as(C.POINTER(C.c_ulonglong))
    assert L.psdc_debug_census_min_run(a.min_run) == 0
    for r in range(a.rounds):
        if r == a.rounds - 1:
            bank.sync()
            assert L.psdc_debug_census(ptr, MAX_WAVES) == 0  # (clears the records of the rounds before)
        for _ in range(a.spans):
            bank.process_device(0, x.data_ptr(), total)
    bank.sync()
    rc = L.psdc_debug_census(ptr, MAX_WAVES)
    assert rc == 0, rc
    res = reduce_census(out)
    res["config"] = {"lib": os.path.basename(a.lib), "n": a.n, "log2": a.log2, "spans": a.spans, "min_run": a.min_run}
    report(res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    bank.close()


if __name__ == "__main__":
    main()
