"""Measure the cross-spectral cascade (psdc_cross_*): one JSON line.

    python tools/cross_probe.py [--seconds 0.5]
    python tools/cross_probe.py --frames [--out profiles/cross_frames_probe.json]

Legs: device-resident pairs at N = 512, 1024, 4096 with 1 and 4 pairs in 2^24-pair calls (warm-up, then a window of at
least --seconds timed on the host clock ending in psdc_cross_sync); kernel launches of one steady-state call; one
host-fed leg.  Roofline: 8 algorithmic bytes a pair (x and y read once) against 8 TB/s of HBM.
--frames: device-resident AdcDac frames (128 batches a frame) into the pairs (ADC0, DAC0), (ADC1, DAC1) at N = 512, 1024, 4096
in calls of 2^22 samples a trace (psdc_csd_process_frames_device), next to the same two pairs fed f32 (psdc_cross_process_device,
2^22 samples a call and pair); both timed the same way, G pairs/s = pairs fed / second.
--matrix: one m = 4 group (psdc_csm_*) against the six pairs it replaces.  Four device-resident f32 streams of 2^22 samples a call
at N = 512, 1024, 2048; leg A is CsdCascadeBank(n, 6) fed the six pairs of the four streams (six calls a step), leg B is
CsmCascadeBank(n, 4) (one call a step); unit: sample times a second (one sample of each of the four streams).  A, B and A again
are timed in turn --reps times in one session: the ratio B / A per turn, and |A' - A| / A as the session's spread.  Also one
m = 2 group against one pair.  --matrix --only-a times leg A alone (for a run on another build of the library through PSDC_LIB).
--matrix --frames: the four traces of device-resident AdcDac frames as one m = 4 group against the two-pair frames leg above.
--zoom --frames: stream frames into a zoom object.  AdcDac (128 batches a frame) and Mpll (255 batches) frames of 2^22 samples a
trace a call at N = 512, 1024, 4096.  Leg A is the route tools/psd_cli.py --zoom takes: every frame decoded on the host
(source.decode_frame), the trace through psdc_zoom_process from host memory.  Leg B is psdc_zoomcascade_process_frames_device on the same
frames resident in device memory.  Leg C (a ceiling, not a gate) is psdc_zoom_process_device on the pre-decoded f32 trace resident
in device memory.  A, B, A, C in turn --reps times in one session; B beats A when every B / A exceeds 1 + the largest |A' - A| / A.
Also four carriers on trace 0: one B call feeding four channels against four C calls.  Clocks and power from rocm-smi (read only)
before and after.  Writes profiles/zoom_frames_probe.json unless --out names another file.
--zoom --pair: two streams around a carrier.  Two device-resident f32 streams (b = 0.6 a delayed by 3 samples + noise) of 2^24
samples a call at N = 512, 1024, 2048; leg A is CsmCascadeBank(n, 4) fed the pre-mixed (I_a, Q_a, I_b, Q_b) -- four transforms and
sixteen rows a segment pair --, leg B is ZoomCsdCascadeBank(n, 1) fed (a, b) -- two mixers, two transforms and eight rows a segment;
A / B / A in turn --reps times in one session, idle clocks and power before and after.  Also the tone-image figure of the cross
row: a tone at f0 + delta on both channels, |S_ab lower| / |S_ab upper| at the tone's bin from B and rebuilt from A's sixteen rows.
Writes profiles/zoom_cross_probe.json unless --out names another file.
--zoom --pair --frames: stream frames into a zoom cross object.  AdcDac (128 batches a frame, the pair (ADC0, DAC0)) and Mpll (255
batches, the pair (phase, frequency)) frames of 2^22 samples a trace a call, one piece each, at N = 512, 1024, 4096.  Leg A is the
route tools/psd_cli.py --zoom-pair takes: every frame decoded on the host (source.decode_frame), both traces through
psdc_zcsd_process from host memory.  Leg B is psdc_zoomcsdcascade_process_frames_device on the same frames resident in device
memory with ONE carrier on both sides (the shared oscillator); leg B' is the same call with two different carriers (two
oscillators a sample).  Leg C (a ceiling, not a gate) is psdc_zcsd_process_device on the pre-decoded f32 traces resident in device
memory.  A, B, A, C, B' in turn --reps times in one session; B beats A when every B / A exceeds 1 + the largest |A' - A| / A.
B / C and B / B' are recorded, not gated.  Clocks and power from rocm-smi (read only) before and after.  Writes
profiles/zoom_cross_frames_probe.json unless --out names another file.
--iq: a complex stream that is complex already.  One device-resident complex64 stream of 2^24 samples a call at N = 512, 1024, 4096.
Leg A (a ceiling: the same round, 4 bytes a sample read instead of 8) is ZoomCascadeBank(n, 1) fed a real stream; leg B is
IqCascadeBank(n, 1) fed the interleaved complex64; leg C is what a user did before: CsdCascadeBank(n, 1) fed the planar (I, Q).
A, B, A, C in turn --reps times in one session; B / A, B / C and the largest |A' - A| / A are recorded as findings, none is a gate.
Clocks and power from rocm-smi (read only) before and after.  Writes profiles/iq_probe.json unless --out names another file.
--iq --pair: two complex streams.  One device-resident pair of 2^24 sample pairs a call at N = 512, 1024, 2048, 4096.  Leg A (a
ceiling: the same round, half the bytes read) is ZoomCsdCascadeBank(n, 1) fed two real streams; leg B is IqCsdCascadeBank(n, 1) fed
two interleaved complex64 streams; leg C is what a user did before: CsmCascadeBank(n, 4, 1) fed the four planar streams (N <= 2048
only, and it cannot retune).  A, B, A, C in turn --reps times in one session; B / A, B / C, the largest |A' - A| / A and B's launches
a call are recorded as findings, none is a gate.  Writes profiles/iq_cross_probe.json unless --out names another file.
--iq --int [--pair]: the integer feed against the f32 feed of the same stream (sc16, scale 2^-15) at N = 512, 1024, 4096.  Host
memory, 2^22 units a call: leg A is IqCascadeBank(n, 1) (--pair: IqCsdCascadeBank(n, 1)) fed interleaved complex64, leg B the same
object kind fed the sc16 stream whose conversion A's is -- half the bytes over the host link.  Device memory, 2^24 units a call:
legs C (complex64) and D (sc16).  A, B, A and C, D, C in turn --reps times in one session; the rates, B / A, D / C, the largest
|A' - A| / A and |C' - C| / C and the launches a call of B and D are recorded as findings, none is a gate.  Writes
profiles/iq_int_probe.json (--pair: its "pair" entry; the file holds one entry a flavour) unless --out names another file.
--real-int: the integer feed of the objects with no mixer (s16, scale 2^-15) against the f32 feed of the converted stream on the
same kind of object, at N = 512, 1024, 4096: PsdCascadeBank(n, 1) and CsdCascadeBank(n, 1), host-fed in 2^22-unit calls and
device-resident in 2^24-unit calls.  A (f32), B (s16), A in turn --reps times for each of the four; the rates, B / A, the largest
|A' - A| / A and the pair object's launches a steady call are recorded as findings, none is a gate.  Writes
profiles/real_int_probe.json unless --out names another file.
--sk: per-bin Gaussianity beside the PSD.  One device-resident f32 stream of 2^24 samples a call at N = 512, 1024, 4096.  Leg A:
CsdCascadeBank(n, 1) fed (x, x), the nearest the other objects come (two transforms and decimations, S1 three times, no S2).  Leg B:
SkCascadeBank(n, 1) fed x.  A, B, A in turn --reps times; the rates, B / A, the largest |A' - A| / A and B's launches a steady call
are recorded as findings, none is a gate.  Writes profiles/sk_probe.json unless --out names another file.
--zoom --sk / --iq --sk: SK around a carrier against the first-moment object it extends.  One device-resident stream (real f32 /
complex64, carrier 0.2) of 2^24 samples a call at N = 512, 1024, 4096.  Leg A: ZoomCascadeBank(n, 1) / IqCascadeBank(n, 1).  Leg B:
ZoomSkCascadeBank(n, 1) / IqSkCascadeBank(n, 1) fed the same stream: the same transform with the second accumulator set.  A, B, A in
turn --reps times with the windows and the sync of --sk; B / A of every turn, the largest |A' - A| / A, B's launches a steady call
and the live stages are recorded as findings, none is a gate.  Each writes its family's entry ("zoom" / "iq") of
profiles/zoom_sk_probe.json unless --out names another file.
--zoom --ampm / --iq --ampm: the AM/PM objects.  One device-resident stream (real f32 / complex64, carrier 0.2) of 2^24 samples a
call at N = 512, 1024, 4096, the windows and the sync of --sk.  --zoom, first leg: A is ZoomCsdCascadeBank(n, 1) fed (x, x) with the
carriers +ftw and -ftw -- the only way to the complementary spectrum without the object: two mixers, two transforms, eight rows --
and B is ZoomAmPmCascadeBank(n, 1) fed x.  Second leg (the only one of --iq): A is the two-row object, ZoomCascadeBank /
IqCascadeBank, and B the AM/PM bank: the cost of the two extra rows and the natural-order pass.  A, B, A in turn --reps times; B / A
of every turn, the largest |A' - A| / A, B's launches a steady call and the live stages are recorded as findings, none is a gate.
Each writes its family's entry ("zoom" / "iq") of profiles/zoom_ampm_probe.json unless --out names another file.
--zoom --pair --ampm / --iq --pair --ampm: the AM/PM cross objects.  Two device-resident streams (real f32 / complex64, carrier 0.2
on both sides) of 2^24 samples a call at N = 512, 1024, 4096, the windows and the sync of --sk.  A is the only way to the twelve
rows without the object: a ZoomCsdCascadeBank(n, 2) whose pairs are (a:+ftw, b:+ftw) and (a:+ftw, b:-ftw) -- four mixers, four
transforms, eight decimator jobs -- or, for --iq, an IqCsdCascadeBank(n, 2) fed (a, b) and (a, conj b).  B is
ZoomAmPmCsdCascadeBank(n, 1) / IqAmPmCsdCascadeBank(n, 1) fed (a, b): two transforms.  A, B, A in turn --reps times; B / A of every
turn, the largest |A' - A| / A, B's launches a steady call and the live stages are recorded as findings, none is a gate.  Each writes
its family's entry ("zoom" / "iq") of profiles/zoom_ampm_cross_probe.json unless --out names another file.
--waterfall / --zoom --waterfall: what cutting a round into blocks costs.  One device-resident real f32 stream (carrier 0.2 for
--zoom) of 2^24 samples a call at N = 512, 1024, 4096, the windows and the sync of --sk.  Leg A: SkCascadeBank(n, 1) /
ZoomSkCascadeBank(n, 1).  Leg B: WaterfallCascadeBank(n, 1) / ZoomWaterfallCascadeBank(n, 1) with depth 64, at block 64 and at block
4096.  A, B, A in turn --reps times; B / A of every turn, the largest |A' - A| / A, the launches a steady call of both, and the time
of one image_device call of every stage are recorded as findings, none is a gate.  Each writes its entry ("real" / "zoom") of
profiles/waterfall_probe.json unless --out names another file.
--waterfall --robust [--zoom]: what the robust read-out costs beside the image.  One device-resident real f32 stream (carrier 0.2
for --zoom) into a WaterfallCascadeBank(n, 1, block=64, depth=64) / ZoomWaterfallCascadeBank until the ring of stage 0 is full, at
N = 512, 1024, 4096.  Leg A: one image_device call of stage 0 (both images, 64 rows).  Leg B: one robust.stage_robust_device call of
stage 0 with all five outputs (64 rows).  Both return when their kernel has completed, so a leg is a window of >= --seconds of
back-to-back calls on the host clock, and its figure the time a call.  A, B, A in turn --reps times; B / A of every turn and the
largest |A' - A| / A are recorded as findings, none is a gate.  Each writes its entry ("real" / "zoom") of
profiles/waterfall_robust_probe.json unless --out names another file.
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


def timed(step, sync, seconds):
    """pairs fed per second by back-to-back step() calls (each returns the pairs it fed): a window of >= seconds ending in sync()"""
    for _ in range(3):
        step()
    sync()
    calls = 4
    while True:
        t0 = time.perf_counter()
        fed = sum(step() for _ in range(calls))
        sync()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return fed / dt, calls, dt
        calls = int(calls * 1.2 * seconds / dt) + 1


def frames_legs(pkg, torch, seconds):
    call = 1 << 22
    batches = 128
    rng = np.random.default_rng(7)
    w = rng.integers(-20000, 20000, size=(4, call), dtype=np.int64).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(w, batches)
    nf = len(data) // fs
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    lsb = np.float32(4.096) * np.float32(2.5) / np.float32(32768.0)
    tr = [torch.from_numpy(w[c].astype(np.float32) * lsb).cuda() for c in range(4)]
    torch.cuda.synchronize()
    pairs = [("ADC0", "DAC0"), ("ADC1", "DAC1")]
    legs = []
    for n in (512, 1024, 4096):
        fb = pkg.CsdCascadeBank(n, 2)

        def fstep():
            fb.process_frames_device(d.data_ptr(), fs, nf, pairs)
            return 2 * call

        fr, fcalls, fdt = timed(fstep, fb.sync, seconds)
        fb.stats_read(reset=True)
        fstep()
        flaunch = fb.stats_read()["launches"]
        xb = pkg.CsdCascadeBank(n, 2)

        def xstep():
            xb.process_device(0, tr[0].data_ptr(), tr[2].data_ptr(), call)
            xb.process_device(1, tr[1].data_ptr(), tr[3].data_ptr(), call)
            return 2 * call

        xr, xcalls, xdt = timed(xstep, xb.sync, seconds)
        legs.append({"n": n, "pairs": 2, "call_samples_per_trace": call, "frame_size": fs,
                     "frames_gpairs_s": round(fr / 1e9, 2), "frames_calls": fcalls, "frames_seconds": round(fdt, 4),
                     "frames_launches_per_call": flaunch,
                     "f32_gpairs_s": round(xr / 1e9, 2), "f32_calls": xcalls, "f32_seconds": round(xdt, 4),
                     "ratio": round(fr / xr, 3)})
        fb.close()
        xb.close()
    return legs


def matrix_legs(pkg, torch, seconds, reps, only_a):
    call = 1 << 22
    xs = [torch.randn(call, device="cuda")]
    xs += [(0.5 * xs[0] + torch.randn(call, device="cuda")) for _ in range(3)]
    torch.cuda.synchronize()
    ptr = [x.data_ptr() for x in xs]
    six = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    legs = []
    for n in (512, 1024, 2048):
        pa = pkg.CsdCascadeBank(n, 6)

        def a_step():
            for p, (a, b) in enumerate(six):
                pa.process_device(p, ptr[a], ptr[b], call)
            return call

        if only_a:
            series = [round(timed(a_step, pa.sync, seconds)[0] / 1e9, 3) for _ in range(reps)]
            legs.append({"n": n, "a_gst_s": series})
            pa.close()
            continue
        gb = pkg.CsmCascadeBank(n, 4)
        p1 = pkg.CsdCascadeBank(n, 1)
        g2 = pkg.CsmCascadeBank(n, 2)

        def b_step():
            gb.process_device(0, ptr, call)
            return call

        def p1_step():
            p1.process_device(0, ptr[0], ptr[1], call)
            return call

        def g2_step():
            g2.process_device(0, ptr[:2], call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, gb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
        gb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = gb.stats_read()["launches"] / 8
        gb.sync()
        pair = timed(p1_step, p1.sync, seconds)[0] / 1e9
        grp2 = timed(g2_step, g2.sync, seconds)[0] / 1e9
        ratios = [y / x for x, y in zip(a1, b)]
        spread = max(abs(y - x) / x for x, y in zip(a1, a2))
        legs.append({"n": n, "call": call, "a_six_pairs_gst_s": [round(v, 3) for v in a1], "b_group4_gst_s": [round(v, 3) for v in b],
                     "a_again_gst_s": [round(v, 3) for v in a2], "ratio_b_over_a": [round(r, 3) for r in ratios],
                     "ratio_min": round(min(ratios), 3), "aa_spread_max": round(spread, 4),
                     "b_beats_a": bool(min(ratios) > 1 + spread), "b_launches_per_call": launches, "stages": gb.num_stages(0),
                     "one_pair_gst_s": round(pair, 3), "group2_gst_s": round(grp2, 3), "group2_over_pair": round(grp2 / pair, 3)})
        for o in (pa, gb, p1, g2):
            o.close()
    return legs


def zoom_legs(pkg, torch, seconds, reps, call):
    """One device-resident f32 stream.  A: CsdCascadeBank(n, 1) fed the pre-mixed (I, Q) streams (the same transforms and
    decimations, four rows and a separation).  B: ZoomCascadeBank(n, 1) fed x (two rows, plus the mixer).  A / B / A in turn."""
    x = torch.randn(call, device="cuda")
    ph = 2 * np.pi * 0.2 * torch.arange(call, device="cuda", dtype=torch.float64)
    xi = (x * torch.cos(ph).float()).contiguous()
    xq = (-x * torch.sin(ph).float()).contiguous()
    del ph
    torch.cuda.synchronize()
    legs = []
    for n in (512, 1024, 4096):
        pa = pkg.CsdCascadeBank(n, 1)
        zb = pkg.ZoomCascadeBank(n, 1)
        zb.set_carrier(0, f0=0.2)

        def a_step():
            pa.process_device(0, xi.data_ptr(), xq.data_ptr(), call)
            return call

        def b_step():
            zb.process_device(0, x.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
        zb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = zb.stats_read()["launches"] / 8
        zb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        legs.append({"n": n, "call": call, "a_pair_fed_iq_gs_s": [round(v, 3) for v in a1], "b_zoom_gs_s": [round(v, 3) for v in b],
                     "a_again_gs_s": [round(v, 3) for v in a2], "ratio_b_over_a": [round(r, 3) for r in ratios],
                     "ratio_min": round(min(ratios), 3), "aa_spread_max": round(spread, 4),
                     "b_beats_a": bool(min(ratios) > 1 + spread), "b_launches_per_call": launches, "stages": zb.num_stages(0)})
        pa.close()
        zb.close()
    return legs


def sk_legs(pkg, torch, seconds, reps, call):
    """One device-resident f32 stream x.  A: CsdCascadeBank(n, 1) fed (x, x) -- the only way the other objects come near the
    question, two transforms and two decimations a segment pair, four rows, S1 three times over and no S2.  B: SkCascadeBank(n, 1)
    fed x (one transform and one decimation, two rows).  A / B / A in turn."""
    x = torch.randn(call, device="cuda")
    torch.cuda.synchronize()
    legs = []
    for n in (512, 1024, 4096):
        pa = pkg.CsdCascadeBank(n, 1)
        sb = pkg.SkCascadeBank(n, 1)

        def a_step():
            pa.process_device(0, x.data_ptr(), x.data_ptr(), call)
            return call

        def b_step():
            sb.process_device(0, x.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, sb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, pa.sync, seconds)[0] / 1e9)
        sb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = sb.stats_read()["launches"] / 8
        sb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        legs.append({"n": n, "call": call, "a_pair_fed_xx_gs_s": [round(v, 3) for v in a1], "b_sk_gs_s": [round(v, 3) for v in b],
                     "a_again_gs_s": [round(v, 3) for v in a2], "ratio_b_over_a": [round(r, 3) for r in ratios],
                     "ratio_min": round(min(ratios), 3), "aa_spread_max": round(spread, 4),
                     "b_beats_a": bool(min(ratios) > 1 + spread), "b_launches_per_call": launches, "stages": sb.num_stages(0)})
        pa.close()
        sb.close()
    return legs


def zoom_sk_legs(pkg, torch, seconds, reps, call, iq):
    """One device-resident stream, carrier 0.2: real f32 (iq False) or complex64 interleaved (iq True).  A: ZoomCascadeBank /
    IqCascadeBank; B: ZoomSkCascadeBank / IqSkCascadeBank, the same mixer and transform with S2 kept beside S1.  A / B / A in turn."""
    x = torch.randn(call, dtype=torch.complex64 if iq else torch.float32, device="cuda")
    torch.cuda.synchronize()
    legs = []
    for n in (512, 1024, 4096):
        za = (pkg.IqCascadeBank if iq else pkg.ZoomCascadeBank)(n, 1)
        zb = (pkg.IqSkCascadeBank if iq else pkg.ZoomSkCascadeBank)(n, 1)
        za.set_carrier(0, f0=0.2)
        zb.set_carrier(0, f0=0.2)

        def a_step():
            za.process_device(0, x.data_ptr(), call)
            return call

        def b_step():
            zb.process_device(0, x.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, za.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, za.sync, seconds)[0] / 1e9)
        zb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = zb.stats_read()["launches"] / 8
        zb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "call": call, "a_first_moment_gs_s": r3(a1), "b_sk_gs_s": r3(b), "a_again_gs_s": r3(a2),
                     "ratio_b_over_a": r3(ratios), "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
                     "aa_spread_max": round(spread, 4), "b_below_a_beyond_spread": bool(max(ratios) < 1 - spread),
                     "b_launches_per_call": launches, "stages": zb.num_stages(0), "a_stages": za.num_stages(0)})
        za.close()
        zb.close()
    return legs


def waterfall_legs(pkg, torch, seconds, reps, call, zoom):
    """One device-resident real f32 stream (zoom: carrier 0.2).  A: SkCascadeBank / ZoomSkCascadeBank; B: WaterfallCascadeBank /
    ZoomWaterfallCascadeBank with depth 64 at block 64 (a call crosses many blocks: a job a block) and block 4096 (about as many
    segments as a call of 2^24 samples has at N = 4096: a piece or two a stage).  A / B / A in turn; then B's launches a steady call and
    one image_device of every stage into a tensor."""
    x = torch.randn(call, device="cuda")
    torch.cuda.synchronize()
    legs = []
    r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
    for n in (512, 1024, 4096):
        for block in (64, 4096):
            sa = (pkg.ZoomSkCascadeBank if zoom else pkg.SkCascadeBank)(n, 1)
            wb = (pkg.ZoomWaterfallCascadeBank if zoom else pkg.WaterfallCascadeBank)(n, 1, block=block, depth=64)
            if zoom:
                sa.set_carrier(0, f0=0.2)
                wb.set_carrier(0, f0=0.2)

            def a_step():
                sa.process_device(0, x.data_ptr(), call)
                return call

            def b_step():
                wb.process_device(0, x.data_ptr(), call)
                return call

            a1, b, a2 = [], [], []
            for _ in range(reps):
                a1.append(timed(a_step, sa.sync, seconds)[0] / 1e9)
                b.append(timed(b_step, wb.sync, seconds)[0] / 1e9)
                a2.append(timed(a_step, sa.sync, seconds)[0] / 1e9)
            launches = []
            for obj, step in ((sa, a_step), (wb, b_step)):
                obj.stats_read(reset=True)
                for _ in range(8):
                    step()
                launches.append(obj.stats_read()["launches"] / 8)
                obj.sync()
            sides = 2 if zoom else 1
            img = torch.empty((64, sides, n // 2 + 1), device="cuda")
            sk = torch.empty_like(img)
            torch.cuda.synchronize()
            image_us = []
            for k in range(wb.num_stages(0)):
                wb.image_device(0, k, img.data_ptr(), sk.data_ptr())  # (the first call of a stage pays nothing extra; timed below)
                t0 = time.perf_counter()
                idx, _ = wb.image_device(0, k, img.data_ptr(), sk.data_ptr())
                image_us.append({"stage": k, "rows": int(idx.size), "us": round((time.perf_counter() - t0) * 1e6, 1)})
            ratios = [y / u for u, y in zip(a1, b)]
            spread = max(abs(y - u) / u for u, y in zip(a1, a2))
            legs.append({"n": n, "call": call, "block": block, "depth": 64, "a_sk_gs_s": r3(a1), "b_waterfall_gs_s": r3(b),
                         "a_again_gs_s": r3(a2), "ratio_b_over_a": r3(ratios), "ratio_min": round(min(ratios), 3),
                         "ratio_max": round(max(ratios), 3), "aa_spread_max": round(spread, 4),
                         "b_below_a_beyond_spread": bool(max(ratios) < 1 - spread), "a_launches_per_call": launches[0],
                         "b_launches_per_call": launches[1], "stages": wb.num_stages(0), "image_device": image_us})
            sa.close()
            wb.close()
    return legs


def per_call_us(step, seconds):
    """microseconds a call of back-to-back step() calls that each return when their kernel has completed: a window of >= seconds"""
    for _ in range(5):
        step()
    calls = 16
    while True:
        t0 = time.perf_counter()
        for _ in range(calls):
            step()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / calls * 1e6
        calls = int(calls * 1.2 * seconds / dt) + 1


def waterfall_robust_legs(pkg, torch, seconds, reps, call, zoom):
    """One device-resident real f32 stream (zoom: carrier 0.2) into a waterfall bank with block 64 and depth 64 until stage 0's ring
    is full.  A: image_device of stage 0 (psd and sk, 64 rows); B: robust.stage_robust_device of stage 0 (all five outputs, 64
    rows).  A / B / A in turn, the time a call."""
    from stabilizer_stream_amd import robust
    x = torch.randn(call, device="cuda")
    torch.cuda.synchronize()
    legs = []
    r2 = lambda vs: [round(v, 2) for v in vs]  # noqa: E731
    for n in (512, 1024, 4096):
        wb = (pkg.ZoomWaterfallCascadeBank if zoom else pkg.WaterfallCascadeBank)(n, 1, block=64, depth=64)
        if zoom:
            wb.set_carrier(0, f0=0.2)
        while not wb.num_stages(0) or wb.stage_blocks(0, 0)["started"] <= 64:
            wb.process_device(0, x.data_ptr(), call)
        sides = 2 if zoom else 1
        img = torch.empty((64, sides, n // 2 + 1), device="cuda")
        sk = torch.empty_like(img)
        outs = {k: torch.empty((sides, n // 2 + 1), device="cuda", dtype=torch.int32 if k == "kept" else torch.float32)
                for k in ("median", "min", "max", "excised", "kept")}
        ptrs = {k: v.data_ptr() for k, v in outs.items()}
        lim = robust.sk_limits(64)
        torch.cuda.synchronize()
        rows_a = int(wb.image_device(0, 0, img.data_ptr(), sk.data_ptr())[0].size)
        info = robust.stage_robust_device(wb, 0, ptrs, sk_limits=lim)

        def a_step():
            wb.image_device(0, 0, img.data_ptr(), sk.data_ptr())

        def b_step():
            robust.stage_robust_device(wb, 0, ptrs, sk_limits=lim)

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(per_call_us(a_step, seconds))
            b.append(per_call_us(b_step, seconds))
            a2.append(per_call_us(a_step, seconds))
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        legs.append({"n": n, "block": 64, "depth": 64, "stage": 0, "image_rows": rows_a, "robust_rows": info["rows"],
                     "a_image_device_us": r2(a1), "b_stage_robust_device_us": r2(b), "a_again_us": r2(a2),
                     "ratio_b_over_a": [round(v, 3) for v in ratios], "ratio_min": round(min(ratios), 3),
                     "ratio_max": round(max(ratios), 3), "aa_spread_max": round(spread, 4),
                     "ring_bytes_a_pass": 64 * 2 * sides * (n // 2 + 1) * 8})
        wb.close()
    return legs


def ampm_legs(pkg, torch, seconds, reps, call, iq, recipe):
    """One device-resident stream, carrier 0.2: real f32 (iq False) or complex64 interleaved (iq True).  B: ZoomAmPmCascadeBank /
    IqAmPmCascadeBank.  A: with `recipe` ZoomCsdCascadeBank fed (x, x) with carriers +ftw and -ftw (S_ab upper is conj(comp)), else
    the two-row object ZoomCascadeBank / IqCascadeBank.  A / B / A in turn."""
    x = torch.randn(call, dtype=torch.complex64 if iq else torch.float32, device="cuda")
    torch.cuda.synchronize()
    ftw = pkg.zoom_ftw(0.2)[0]
    legs = []
    for n in (512, 1024, 4096):
        zb = (pkg.IqAmPmCascadeBank if iq else pkg.ZoomAmPmCascadeBank)(n, 1)
        zb.set_carrier(0, ftw=ftw)
        if recipe:
            za = pkg.ZoomCsdCascadeBank(n, 1)
            za.set_carrier(0, ftw=ftw, side=0)
            za.set_carrier(0, ftw=(-ftw) % (1 << 64), side=1)
        else:
            za = (pkg.IqCascadeBank if iq else pkg.ZoomCascadeBank)(n, 1)
            za.set_carrier(0, ftw=ftw)

        def a_step():
            if recipe:
                za.process_device(0, x.data_ptr(), x.data_ptr(), call)
            else:
                za.process_device(0, x.data_ptr(), call)
            return call

        def b_step():
            zb.process_device(0, x.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, za.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, za.sync, seconds)[0] / 1e9)
        zb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = zb.stats_read()["launches"] / 8
        zb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "call": call, "a_gs_s": r3(a1), "b_ampm_gs_s": r3(b), "a_again_gs_s": r3(a2),
                     "ratio_b_over_a": r3(ratios), "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
                     "aa_spread_max": round(spread, 4), "b_beats_a_beyond_spread": bool(min(ratios) > 1 + spread),
                     "b_below_a_beyond_spread": bool(max(ratios) < 1 - spread),
                     "b_launches_per_call": launches, "stages": zb.num_stages(0), "a_stages": za.num_stages(0)})
        za.close()
        zb.close()
    return legs


def ampm_pair_legs(pkg, torch, seconds, reps, call, iq):
    """Two device-resident streams, carrier 0.2 on both sides: real f32 (iq False) or complex64 interleaved (iq True).
    B: ZoomAmPmCsdCascadeBank / IqAmPmCsdCascadeBank, one pair.  A: the two-pair recipe on ZoomCsdCascadeBank (pair 1 with -ftw on
    side b) / IqCsdCascadeBank (pair 1 fed conj b).  A / B / A in turn; a sample pair is one sample of each side."""
    dt = torch.complex64 if iq else torch.float32
    xa, xb = torch.randn(call, dtype=dt, device="cuda"), torch.randn(call, dtype=dt, device="cuda")
    xc = torch.conj(xb).resolve_conj().contiguous() if iq else xb
    torch.cuda.synchronize()
    ftw = pkg.zoom_ftw(0.2)[0]
    legs = []
    for n in (512, 1024, 4096):
        zb = (pkg.IqAmPmCsdCascadeBank if iq else pkg.ZoomAmPmCsdCascadeBank)(n, 1)
        zb.set_carrier(0, ftw=ftw)
        za = (pkg.IqCsdCascadeBank if iq else pkg.ZoomCsdCascadeBank)(n, 2)
        za.set_carrier(0, ftw=ftw)
        za.set_carrier(1, ftw=ftw, side=0)
        za.set_carrier(1, ftw=ftw if iq else (-ftw) % (1 << 64), side=1)

        def a_step():
            za.process_device(0, xa.data_ptr(), xb.data_ptr(), call)
            za.process_device(1, xa.data_ptr(), xc.data_ptr(), call)
            return call

        def b_step():
            zb.process_device(0, xa.data_ptr(), xb.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, za.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, za.sync, seconds)[0] / 1e9)
        zb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = zb.stats_read()["launches"] / 8
        zb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "call": call, "a_gpairs_s": r3(a1), "b_gpairs_s": r3(b), "a_again_gpairs_s": r3(a2),
                     "ratio_b_over_a": r3(ratios), "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
                     "aa_spread_max": round(spread, 4), "b_beats_a_beyond_spread": bool(min(ratios) > 1 + spread),
                     "b_below_a_beyond_spread": bool(max(ratios) < 1 - spread),
                     "b_launches_per_call": launches, "stages": zb.num_stages(0), "a_stages": za.num_stages(0)})
        za.close()
        zb.close()
    return legs


def iq_legs(pkg, torch, seconds, reps, call):
    """One device-resident complex64 stream z, its planar copies (I, Q) and a real stream x.  A: ZoomCascadeBank fed x (carrier
    0.2); B: IqCascadeBank fed z interleaved (carrier 0.2); C: CsdCascadeBank fed (I, Q).  A / B / A / C in turn."""
    x = torch.randn(call, device="cuda")
    z = torch.randn(call, dtype=torch.complex64, device="cuda")
    zi, zq = z.real.contiguous(), z.imag.contiguous()
    torch.cuda.synchronize()
    legs = []
    for n in (512, 1024, 4096):
        za = pkg.ZoomCascadeBank(n, 1)
        za.set_carrier(0, f0=0.2)
        qb = pkg.IqCascadeBank(n, 1)
        qb.set_carrier(0, f0=0.2)
        pc = pkg.CsdCascadeBank(n, 1)

        def a_step():
            za.process_device(0, x.data_ptr(), call)
            return call

        def b_step():
            qb.process_device(0, z.data_ptr(), call)
            return call

        def c_step():
            pc.process_device(0, zi.data_ptr(), zq.data_ptr(), call)
            return call

        a1, b, a2, c = [], [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, za.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, qb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, za.sync, seconds)[0] / 1e9)
            c.append(timed(c_step, pc.sync, seconds)[0] / 1e9)
        qb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = qb.stats_read()["launches"] / 8
        qb.sync()
        ba = [v / u for u, v in zip(a1, b)]
        bc = [v / u for u, v in zip(c, b)]
        spread = max(abs(v - u) / u for u, v in zip(a1, a2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "call": call, "a_zoom_real_gs_s": r3(a1), "b_iq_interleaved_gs_s": r3(b), "a_again_gs_s": r3(a2),
                     "c_pair_fed_iq_gs_s": r3(c), "ratio_b_over_a": r3(ba), "ratio_b_over_c": r3(bc),
                     "b_over_a_min": round(min(ba), 3), "b_over_c_min": round(min(bc), 3), "aa_spread_max": round(spread, 4),
                     "b_launches_per_call": launches, "stages": qb.num_stages(0)})
        za.close()
        qb.close()
        pc.close()
    return legs


def iq_pair_legs(pkg, torch, seconds, reps, call):
    """One device-resident pair: two real streams (xa, xb), two complex64 streams (za, zb) and their four planar copies.  A:
    ZoomCsdCascadeBank fed (xa, xb) -- half the bytes of B, a ceiling; B: IqCsdCascadeBank fed (za, zb) interleaved; C:
    CsmCascadeBank(n, 4) fed the four planar streams, what a user does today (N <= 2048 only).  Carrier 0.2 on both sides of A
    and B (C cannot retune).  A / B / A / C in turn; unit: sample pairs a second (one sample of each side)."""
    xa, xb = torch.randn(call, device="cuda"), torch.randn(call, device="cuda")
    za = torch.randn(call, dtype=torch.complex64, device="cuda")
    zb = (0.6 * za + 0.8 * torch.randn(call, dtype=torch.complex64, device="cuda")).contiguous()
    four = [za.real.contiguous(), za.imag.contiguous(), zb.real.contiguous(), zb.imag.contiguous()]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in four]
    legs = []
    for n in (512, 1024, 2048, 4096):
        zc = pkg.ZoomCsdCascadeBank(n, 1)
        zc.set_carrier(0, f0=0.2)
        qb = pkg.IqCsdCascadeBank(n, 1)
        qb.set_carrier(0, f0=0.2)
        mc = pkg.CsmCascadeBank(n, 4, 1) if pkg.csm_supported(n, 4) else None

        def a_step():
            zc.process_device(0, xa.data_ptr(), xb.data_ptr(), call)
            return call

        def b_step():
            qb.process_device(0, za.data_ptr(), zb.data_ptr(), call)
            return call

        def c_step():
            mc.process_device(0, ptrs, call)
            return call

        a1, b, a2, c = [], [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, zc.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, qb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, zc.sync, seconds)[0] / 1e9)
            if mc is not None:
                c.append(timed(c_step, mc.sync, seconds)[0] / 1e9)
        qb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = qb.stats_read()["launches"] / 8
        qb.sync()
        ba = [v / u for u, v in zip(a1, b)]
        bc = [v / u for u, v in zip(c, b)]
        spread = max(abs(v - u) / u for u, v in zip(a1, a2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "call": call, "a_zoom_cross_real_gpairs_s": r3(a1), "b_iq_cross_interleaved_gpairs_s": r3(b),
                     "a_again_gpairs_s": r3(a2), "c_matrix_fed_planar_gpairs_s": r3(c) if c else None, "ratio_b_over_a": r3(ba),
                     "ratio_b_over_c": r3(bc) if c else None, "b_over_a_min": round(min(ba), 3),
                     "b_over_c_min": round(min(bc), 3) if c else None, "aa_spread_max": round(spread, 4),
                     "b_beats_c": bool(min(bc) > 1 + spread) if c else None, "b_launches_per_call": launches,
                     "stages": qb.num_stages(0)})
        zc.close()
        qb.close()
        if mc is not None:
            mc.close()
    return legs


def iq_int_legs(pkg, torch, seconds, reps, pair):
    """The sc16 feed against the complex64 feed of the same stream, from host memory (2^22 units a call) and from device memory
    (2^24 units a call): A / B / A and C / D / C in turn.  pair: IqCsdCascadeBank and two streams, else IqCascadeBank and one."""
    host_call, dev_call = 1 << 22, 1 << 24
    rng = np.random.default_rng(7)
    sides = 2 if pair else 1
    kind, scale = pkg.sample_kind(np.int16)
    ints = [np.clip(np.rint(rng.standard_normal((dev_call, 2)) * 6000.0), -32768, 32767).astype(np.int16) for _ in range(sides)]
    f32 = [np.ascontiguousarray(v.astype(np.float32) * np.float32(scale)).view(np.complex64).reshape(-1) for v in ints]
    d_int = [torch.from_numpy(v).cuda() for v in ints]
    d_f32 = [torch.from_numpy(z).cuda() for z in f32]
    torch.cuda.synchronize()
    h_int, h_f32 = [v[:host_call] for v in ints], [z[:host_call] for z in f32]
    cls = pkg.IqCsdCascadeBank if pair else pkg.IqCascadeBank
    legs = []
    for n in (512, 1024, 4096):
        objs = {k: cls(n, 1) for k in "abcd"}
        for o in objs.values():
            o.set_carrier(0, f0=0.2)

        def a_step():
            objs["a"].process(0, *h_f32)
            return host_call

        def b_step():
            objs["b"].process_int(0, *h_int)
            return host_call

        def c_step():
            objs["c"].process_device(0, *[t.data_ptr() for t in d_f32], dev_call)
            return dev_call

        def d_step():
            objs["d"].process_int_device(0, *[t.data_ptr() for t in d_int], dev_call, kind)
            return dev_call

        a1, b, a2, c1, d, c2 = [], [], [], [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, objs["a"].sync, seconds)[0] / 1e9)
            b.append(timed(b_step, objs["b"].sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, objs["a"].sync, seconds)[0] / 1e9)
        for _ in range(reps):
            c1.append(timed(c_step, objs["c"].sync, seconds)[0] / 1e9)
            d.append(timed(d_step, objs["d"].sync, seconds)[0] / 1e9)
            c2.append(timed(c_step, objs["c"].sync, seconds)[0] / 1e9)
        launches = {}
        for k, step in (("a", a_step), ("b", b_step), ("c", c_step), ("d", d_step)):
            objs[k].stats_read(reset=True)
            for _ in range(8):
                step()
            launches[k] = objs[k].stats_read()["launches"] / 8
            objs[k].sync()
        ba = [v / u for u, v in zip(a1, b)]
        dc = [v / u for u, v in zip(c1, d)]
        aa = max(abs(v - u) / u for u, v in zip(a1, a2))
        cc = max(abs(v - u) / u for u, v in zip(c1, c2))
        r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
        legs.append({"n": n, "host_call": host_call, "device_call": dev_call, "a_host_complex64_gs_s": r3(a1), "b_host_sc16_gs_s": r3(b),
                     "a_again_gs_s": r3(a2), "c_device_complex64_gs_s": r3(c1), "d_device_sc16_gs_s": r3(d), "c_again_gs_s": r3(c2),
                     "ratio_b_over_a": r3(ba), "ratio_d_over_c": r3(dc), "b_over_a_min": round(min(ba), 3),
                     "d_over_c_min": round(min(dc), 3), "d_over_c_max": round(max(dc), 3), "aa_spread_max": round(aa, 4),
                     "cc_spread_max": round(cc, 4), "b_beats_a": bool(min(ba) > 1 + aa), "d_beats_c": bool(min(dc) > 1 + cc),
                     "launches_per_call": launches, "stages": objs["d"].num_stages(0)})
        for o in objs.values():
            o.close()
    return legs


def real_int_legs(pkg, torch, seconds, reps):
    """The s16 feed (scale 2^-15) of the PSD and the pair object against the f32 feed of the converted stream on the same kind of
    object: host-fed in 2^22-unit calls (legs psd_host, pair_host) and device-resident in 2^24-unit calls (psd_device, pair_device),
    A / B / A in turn for each, and the launches of a steady call of the pair object."""
    host_call, dev_call = 1 << 22, 1 << 24
    rng = np.random.default_rng(7)
    kind, scale = pkg.sample_kind(np.int16)
    ints = [np.clip(np.rint(rng.standard_normal(dev_call) * 6000.0), -32768, 32767).astype(np.int16) for _ in range(2)]
    f32 = [v.astype(np.float32) * np.float32(scale) for v in ints]
    d_int = [torch.from_numpy(v).cuda() for v in ints]
    d_f32 = [torch.from_numpy(x).cuda() for x in f32]
    torch.cuda.synchronize()
    h_int, h_f32 = [v[:host_call] for v in ints], [x[:host_call] for x in f32]
    r3 = lambda vs: [round(v, 3) for v in vs]  # noqa: E731
    legs = []
    for n in (512, 1024, 4096):
        psd = {k: pkg.PsdCascadeBank(n, 1) for k in "ab"}
        csd = {k: pkg.CsdCascadeBank(n, 1) for k in "ab"}
        steps = {  # name -> (objects, f32 step, s16 step)
            "psd_host": (psd, lambda: psd["a"].process(0, h_f32[0]) or host_call, lambda: psd["b"].process_int(0, h_int[0]) or host_call),
            "pair_host": (csd, lambda: csd["a"].process(0, *h_f32) or host_call, lambda: csd["b"].process_int(0, *h_int) or host_call),
            "psd_device": (psd, lambda: psd["a"].process_device(0, d_f32[0].data_ptr(), dev_call) or dev_call,
                           lambda: psd["b"].process_int_device(0, d_int[0].data_ptr(), dev_call, kind) or dev_call),
            "pair_device": (csd, lambda: csd["a"].process_device(0, *[t.data_ptr() for t in d_f32], dev_call) or dev_call,
                            lambda: csd["b"].process_int_device(0, *[t.data_ptr() for t in d_int], dev_call, kind) or dev_call),
        }
        out = {"n": n, "host_call": host_call, "device_call": dev_call}
        for name, (objs, a_step, b_step) in steps.items():
            a1, b, a2 = [], [], []
            for _ in range(reps):
                a1.append(timed(a_step, objs["a"].sync, seconds)[0] / 1e9)
                b.append(timed(b_step, objs["b"].sync, seconds)[0] / 1e9)
                a2.append(timed(a_step, objs["a"].sync, seconds)[0] / 1e9)
            ba = [v / u for u, v in zip(a1, b)]
            aa = max(abs(v - u) / u for u, v in zip(a1, a2))
            out[name] = {"a_f32_gs_s": r3(a1), "b_s16_gs_s": r3(b), "a_again_gs_s": r3(a2), "ratio_b_over_a": r3(ba),
                         "b_over_a_min": round(min(ba), 3), "b_over_a_max": round(max(ba), 3), "aa_spread_max": round(aa, 4),
                         "b_beats_a": bool(min(ba) > 1 + aa), "b_loses_to_a": bool(max(ba) < 1 - aa)}
        launches = {}
        for name in ("pair_host", "pair_device"):
            objs, a_step, b_step = steps[name]
            for k, step in (("a", a_step), ("b", b_step)):
                objs[k].stats_read(reset=True)
                for _ in range(8):
                    step()
                launches[f"{name}_{'f32' if k == 'a' else 's16'}"] = objs[k].stats_read()["launches"] / 8
                objs[k].sync()
        out["launches_per_call"] = launches
        legs.append(out)
        for o in list(psd.values()) + list(csd.values()):
            o.close()
    return legs


def zoom_pair_image(pkg, torch, n=1024, k=2, b=100, f0=0.2, length=1 << 20):
    """A tone at f0 + delta (delta the centre of bin b of stage k) on both channels, b's at 0.7 of a's and 1 rad behind:
    |S_ab lower[b]| / |S_ab upper[b]| at stage k from the zoom cross object, and the same rebuilt from a matrix object fed the
    pre-mixed (I_a, Q_a, I_b, Q_b): with S[c, d] = conj(X_c) X_d of the four real streams, bin k of
    S_ab upper = S[0,2] + i S[0,3] - i S[1,2] + S[1,3] and S_ab lower = the same sum of the conjugated entries."""
    ftw, f0 = pkg.zoom_ftw(f0)
    delta = b / (n * 8.0 ** k)
    j = np.arange(length, dtype=np.float64)
    xa = np.cos(2 * np.pi * (((f0 + delta) * j) % 1.0)).astype(np.float32)
    xb = (0.7 * np.cos(2 * np.pi * (((f0 + delta) * j) % 1.0) - 1.0)).astype(np.float32)
    z = pkg.ZoomCsdCascade(n, ftw=ftw)
    z.process(xa, xb)
    _, r = z.stage_spectra(k)
    r = r.astype(np.float64)
    native = float(np.hypot(r[5][b], r[7][b]) / np.hypot(r[4][b], r[6][b]))
    z.close()
    ph = 2 * np.pi * ((f0 * j) % 1.0)
    c, sn = np.cos(ph), np.sin(ph)
    four = [(xa * c).astype(np.float32), (-xa * sn).astype(np.float32), (xb * c).astype(np.float32), (-xb * sn).astype(np.float32)]
    m = pkg.CsmCascade(n, 4)
    m.process(four)
    S = m.stage_spectra(k)[1].astype(np.complex128)[:, :, b]  # (m, m, bins) Hermitian, from the f32 rows
    m.close()
    up = S[0, 2] + 1j * S[0, 3] - 1j * S[1, 2] + S[1, 3]
    lo = np.conj(S[0, 2]) + 1j * np.conj(S[0, 3]) - 1j * np.conj(S[1, 2]) + np.conj(S[1, 3])
    return {"n": n, "stage": k, "bin": b, "image_over_peak_zoom_cross": native, "image_over_peak_rebuilt_from_matrix_rows": float(abs(lo) / abs(up))}


def zoom_pair_legs(pkg, torch, seconds, reps, call):
    """Two device-resident f32 streams.  A: CsmCascadeBank(n, 4) fed the pre-mixed (I_a, Q_a, I_b, Q_b).  B: ZoomCsdCascadeBank(n, 1)
    fed (a, b).  A / B / A in turn; unit: sample pairs a second (one sample of a and one of b)."""
    xa = torch.randn(call + 3, device="cuda")
    xb = (0.6 * xa[:-3] + 0.8 * torch.randn(call, device="cuda")).contiguous()
    xa = xa[3:].contiguous()
    ph = 2 * np.pi * 0.2 * torch.arange(call, device="cuda", dtype=torch.float64)
    c, sn = torch.cos(ph).float(), torch.sin(ph).float()
    del ph
    four = [(xa * c).contiguous(), (-xa * sn).contiguous(), (xb * c).contiguous(), (-xb * sn).contiguous()]
    del c, sn
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in four]
    legs = []
    for n in (512, 1024, 2048):
        ma = pkg.CsmCascadeBank(n, 4, 1)
        zb = pkg.ZoomCsdCascadeBank(n, 1)
        zb.set_carrier(0, f0=0.2)

        def a_step():
            ma.process_device(0, ptrs, call)
            return call

        def b_step():
            zb.process_device(0, xa.data_ptr(), xb.data_ptr(), call)
            return call

        a1, b, a2 = [], [], []
        for _ in range(reps):
            a1.append(timed(a_step, ma.sync, seconds)[0] / 1e9)
            b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
            a2.append(timed(a_step, ma.sync, seconds)[0] / 1e9)
        zb.stats_read(reset=True)
        for _ in range(8):
            b_step()
        launches = zb.stats_read()["launches"] / 8
        zb.sync()
        ratios = [y / u for u, y in zip(a1, b)]
        spread = max(abs(y - u) / u for u, y in zip(a1, a2))
        legs.append({"n": n, "call": call, "a_matrix_fed_iq_gpairs_s": [round(v, 3) for v in a1],
                     "b_zoom_cross_gpairs_s": [round(v, 3) for v in b], "a_again_gpairs_s": [round(v, 3) for v in a2],
                     "ratio_b_over_a": [round(r, 3) for r in ratios], "ratio_min": round(min(ratios), 3),
                     "aa_spread_max": round(spread, 4), "b_beats_a": bool(min(ratios) > 1 + spread),
                     "b_launches_per_call": launches, "stages": zb.num_stages(0)})
        ma.close()
        zb.close()
    return legs


def gpu_state():
    """sclk / mclk / power as rocm-smi prints them (read only); None where the tool is missing"""
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=30)
        card = next(iter(json.loads(out.stdout).values()))
        return {k: v for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "power"))}
    except Exception:  # noqa: BLE001
        return None


def timed_calls(step, sync, calls):
    """samples a second of `calls` back-to-back step() calls behind one warm-up call (the host-bound leg: a call takes 0.1 ... 1 s)"""
    step()
    sync()
    t0 = time.perf_counter()
    fed = sum(step() for _ in range(calls))
    sync()
    return fed / (time.perf_counter() - t0)


def zoom_frames_legs(pkg, torch, seconds, reps):
    from test_gpu_payload_formats import make_frames, random_payloads  # the frame builders of the test suite
    from stabilizer_stream_amd import source as src  # decode_frame: the host decode of Source (load_package has registered the package)
    call = 1 << 22
    rng = np.random.default_rng(7)
    inputs = []
    w = rng.integers(-20000, 20000, size=(4, call), dtype=np.int64).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(w, 128)
    inputs.append(("AdcDac", data, fs, 0))
    nf = call // 255  # whole frames of at most 2^22 samples: a call is one piece
    data, fs = make_frames(4, 255, random_payloads(rng, 4, 255, nf, wild=False))
    inputs.append(("Mpll", data, fs, 0))
    legs = []
    for name, data, fs, trace in inputs:
        nf = len(data) // fs
        frames = [data[k * fs:(k + 1) * fs] for k in range(nf)]
        x = np.concatenate([src.decode_frame(f)[3][trace][1] for f in frames]).astype(np.float32)
        per_call = x.size
        d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        dx = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        for n in (512, 1024, 4096):
            za, zb, zc = (pkg.ZoomCascadeBank(n, 1) for _ in range(3))
            for z in (za, zb, zc):
                z.set_carrier(0, f0=0.2)

            def a_step():
                za.process(0, np.concatenate([src.decode_frame(f)[3][trace][1] for f in frames]))
                return per_call

            def b_step():
                zb.process_frames_device(d.data_ptr(), fs, nf, [trace])
                return per_call

            def c_step():
                zc.process_device(0, dx.data_ptr(), per_call)
                return per_call

            a1, b, a2, c = [], [], [], []
            for _ in range(reps):
                a1.append(timed_calls(a_step, za.sync, 2) / 1e9)
                b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
                a2.append(timed_calls(a_step, za.sync, 2) / 1e9)
                c.append(timed(c_step, zc.sync, seconds)[0] / 1e9)
            zb.stats_read(reset=True)
            for _ in range(8):
                b_step()
            launches = zb.stats_read()["launches"] / 8
            zb.sync()
            # four carriers on the one trace: one fused call against four calls of the pre-decoded trace
            z4b, z4c = pkg.ZoomCascadeBank(n, 4), pkg.ZoomCascadeBank(n, 4)
            for ch in range(4):
                z4b.set_carrier(ch, f0=0.05 * (ch + 1))
                z4c.set_carrier(ch, f0=0.05 * (ch + 1))

            def b4_step():
                z4b.process_frames_device(d.data_ptr(), fs, nf, [trace] * 4)
                return 4 * per_call

            def c4_step():
                for ch in range(4):
                    z4c.process_device(ch, dx.data_ptr(), per_call)
                return 4 * per_call

            b4, c4 = [], []
            for _ in range(reps):
                b4.append(timed(b4_step, z4b.sync, seconds)[0] / 1e9)
                c4.append(timed(c4_step, z4c.sync, seconds)[0] / 1e9)
            ba = [y / u for u, y in zip(a1, b)]
            bc = [y / u for u, y in zip(c, b)]
            spread = max(abs(y - u) / u for u, y in zip(a1, a2))
            r3 = lambda v: [round(t, 4) for t in v]  # noqa: E731
            legs.append({"format": name, "n": n, "call_samples": per_call, "frame_size": fs, "frames": nf,
                         "a_host_decode_gs_s": r3(a1), "b_frames_device_gs_s": r3(b), "a_again_gs_s": r3(a2),
                         "c_f32_device_gs_s": r3(c), "ratio_b_over_a": [round(r, 2) for r in ba], "ratio_b_over_a_min": round(min(ba), 2),
                         "aa_spread_max": round(spread, 4), "b_beats_a": bool(min(ba) > 1 + spread),
                         "ratio_b_over_c": [round(r, 3) for r in bc], "b_launches_per_call": launches,
                         "four_carriers_b_gs_s": r3(b4), "four_carriers_4c_gs_s": r3(c4),
                         "four_carriers_ratio_b_over_4c": [round(y / u, 3) for u, y in zip(c4, b4)]})
            for o in (za, zb, zc, z4b, z4c):
                o.close()
    return legs


def zoom_pair_frames_legs(pkg, torch, seconds, reps):
    from test_gpu_payload_formats import make_frames, random_payloads  # the frame builders of the test suite
    from stabilizer_stream_amd import source as src  # decode_frame: the host decode of Source
    call = 1 << 22
    rng = np.random.default_rng(7)
    inputs = []
    w = rng.integers(-20000, 20000, size=(4, call), dtype=np.int64).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(w, 128)
    inputs.append(("AdcDac", data, fs, (0, 2)))
    nf = call // 255  # whole frames of at most 2^22 samples: a call is one piece
    data, fs = make_frames(4, 255, random_payloads(rng, 4, 255, nf, wild=False))
    inputs.append(("Mpll", data, fs, (0, 1)))
    legs = []
    for name, data, fs, pair in inputs:
        nf = len(data) // fs
        frames = [data[k * fs:(k + 1) * fs] for k in range(nf)]

        def host_decode():
            tr = [src.decode_frame(f)[3] for f in frames]
            return [np.concatenate([t[side][1] for t in tr]).astype(np.float32) for side in pair]

        xa, xb = host_decode()
        per_call = xa.size
        d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        dxa, dxb = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
        torch.cuda.synchronize()
        for n in (512, 1024, 4096):
            za, zb, zc, z2 = (pkg.ZoomCsdCascadeBank(n, 1) for _ in range(4))
            for z in (za, zb, zc):
                z.set_carrier(0, f0=0.2)
            z2.set_carrier(0, f0=0.2, side=0)
            z2.set_carrier(0, f0=0.21, side=1)

            def a_step():
                za.process(0, *host_decode())
                return per_call

            def b_step():
                zb.process_frames_device(d.data_ptr(), fs, nf, [pair])
                return per_call

            def b2_step():
                z2.process_frames_device(d.data_ptr(), fs, nf, [pair])
                return per_call

            def c_step():
                zc.process_device(0, dxa.data_ptr(), dxb.data_ptr(), per_call)
                return per_call

            a1, b, a2, c, b2 = [], [], [], [], []
            for _ in range(reps):
                a1.append(timed_calls(a_step, za.sync, 2) / 1e9)
                b.append(timed(b_step, zb.sync, seconds)[0] / 1e9)
                a2.append(timed_calls(a_step, za.sync, 2) / 1e9)
                c.append(timed(c_step, zc.sync, seconds)[0] / 1e9)
                b2.append(timed(b2_step, z2.sync, seconds)[0] / 1e9)
            zb.stats_read(reset=True)
            for _ in range(8):
                b_step()
            launches = zb.stats_read()["launches"] / 8
            zb.sync()
            ba = [y / u for u, y in zip(a1, b)]
            spread = max(abs(y - u) / u for u, y in zip(a1, a2))
            r3 = lambda v: [round(t, 4) for t in v]  # noqa: E731
            legs.append({"format": name, "n": n, "pair": list(pair), "call_pairs": per_call, "frame_size": fs, "frames": nf,
                         "a_host_decode_gpairs_s": r3(a1), "b_frames_device_one_carrier_gpairs_s": r3(b), "a_again_gpairs_s": r3(a2),
                         "c_f32_device_gpairs_s": r3(c), "b2_frames_device_two_carriers_gpairs_s": r3(b2),
                         "ratio_b_over_a": [round(r, 2) for r in ba], "ratio_b_over_a_min": round(min(ba), 2),
                         "aa_spread_max": round(spread, 4), "b_beats_a": bool(min(ba) > 1 + spread),
                         "ratio_b_over_c": [round(y / u, 3) for u, y in zip(c, b)],
                         "ratio_b_over_b2": [round(y / u, 3) for u, y in zip(b2, b)], "b_launches_per_call": launches,
                         "stages": zb.num_stages(0)})
            for o in (za, zb, zc, z2):
                o.close()
    return legs


def matrix_frames_legs(pkg, torch, seconds, reps):
    call = 1 << 22
    batches = 128
    rng = np.random.default_rng(7)
    w = rng.integers(-20000, 20000, size=(4, call), dtype=np.int64).astype(np.int16)
    data, fs = pkg.make_adcdac_frames(w, batches)
    nf = len(data) // fs
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    legs = []
    for n in (512, 1024, 2048):
        fb = pkg.CsdCascadeBank(n, 2)
        gb = pkg.CsmCascadeBank(n, 4)

        def pstep():
            fb.process_frames_device(d.data_ptr(), fs, nf, [("ADC0", "DAC0"), ("ADC1", "DAC1")])
            return call

        def gstep():
            gb.process_frames_device(d.data_ptr(), fs, nf, [("ADC0", "ADC1", "DAC0", "DAC1")])
            return call

        pr, gr = [], []
        for _ in range(reps):
            pr.append(timed(pstep, fb.sync, seconds)[0] / 1e9)
            gr.append(timed(gstep, gb.sync, seconds)[0] / 1e9)
        legs.append({"n": n, "call_samples_per_trace": call, "frame_size": fs, "two_pairs_gst_s": [round(v, 3) for v in pr],
                     "group4_gst_s": [round(v, 3) for v in gr], "ratio_group_over_two_pairs": round(min(gr) / max(pr), 3)})
        fb.close()
        gb.close()
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--call-log2", type=int, default=24)
    ap.add_argument("--frames", action="store_true", help="the frames leg only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--matrix", action="store_true", help="one m = 4 group against the six pairs it replaces")
    ap.add_argument("--only-a", action="store_true", help="with --matrix: leg A (six pairs) alone")
    ap.add_argument("--reps", type=int, default=5, help="with --matrix: turns of A, B, A")
    ap.add_argument("--zoom", action="store_true", help="ZoomCascadeBank fed x against CsdCascadeBank fed the pre-mixed (I, Q)")
    ap.add_argument("--pair", action="store_true", help="with --zoom: ZoomCsdCascadeBank fed (a, b) against CsmCascadeBank(n, 4) fed the "
                                                        "pre-mixed (I_a, Q_a, I_b, Q_b); with --zoom --frames: stream frames into a "
                                                        "ZoomCsdCascadeBank against the host decode")
    ap.add_argument("--iq", action="store_true", help="IqCascadeBank fed complex64 against ZoomCascadeBank fed a real stream (a ceiling) "
                                                      "and CsdCascadeBank fed the planar (I, Q); with --pair: IqCsdCascadeBank fed two "
                                                      "complex64 streams against ZoomCsdCascadeBank fed two real streams (a ceiling) "
                                                      "and CsmCascadeBank(n, 4) fed the four planar streams")
    ap.add_argument("--int", dest="int_feed", action="store_true", help="with --iq [--pair]: the sc16 feed against the complex64 feed of "
                                                                        "the same stream, host-fed and device-resident")
    ap.add_argument("--sk", action="store_true", help="SkCascadeBank fed x against CsdCascadeBank fed (x, x); writes profiles/sk_probe.json; "
                                                      "with --zoom / --iq: ZoomSkCascadeBank / IqSkCascadeBank against ZoomCascadeBank / "
                                                      "IqCascadeBank; writes profiles/zoom_sk_probe.json")
    ap.add_argument("--real-int", action="store_true", help="the s16 feed of PsdCascadeBank and CsdCascadeBank against the f32 feed of "
                                                            "the converted stream, host-fed and device-resident")
    ap.add_argument("--ampm", action="store_true", help="with --zoom: ZoomAmPmCascadeBank against ZoomCsdCascadeBank fed (x, x) with "
                                                        "carriers +-ftw, and against ZoomCascadeBank; with --iq: IqAmPmCascadeBank "
                                                        "against IqCascadeBank; writes profiles/zoom_ampm_probe.json; with --pair: "
                                                        "ZoomAmPmCsdCascadeBank / IqAmPmCsdCascadeBank against the two-pair recipe on "
                                                        "the eight-row object; writes profiles/zoom_ampm_cross_probe.json")
    ap.add_argument("--waterfall", action="store_true", help="WaterfallCascadeBank against SkCascadeBank (with --zoom: the zoom objects) "
                                                             "at block 64 and 4096, depth 64; writes profiles/waterfall_probe.json")
    ap.add_argument("--robust", action="store_true", help="with --waterfall: one robust.stage_robust_device call against one image_device "
                                                          "call on the same ring; writes profiles/waterfall_robust_probe.json")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    if a.waterfall and a.robust:
        fam = "zoom" if a.zoom else "real"
        path = a.out or os.path.join(ROOT, "profiles", "waterfall_robust_probe.json")
        record = {}
        if os.path.exists(path):
            with open(path) as f:
                record = json.loads(f.read() or "{}")
        record.update({"metric": "waterfall_robust_call_us", "unit": "microseconds a call (host clock; the call returns when its kernel has completed)",
                       "note": "findings, no gate: A is image_device of stage 0 (psd and sk images of 64 rows), B stage_robust_device of the "
                               "same ring (median, min, max, excised, kept over 64 rows), both one launch and one stream synchronise a "
                               "call; not measured here: kernel time alone, host outputs, other depths and blocks, banks"})
        before = gpu_state()
        legs = waterfall_robust_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, a.zoom)
        record[fam] = {"object": "ZoomWaterfallCascadeBank" if a.zoom else "WaterfallCascadeBank", "gpu_before": before,
                       "gpu_after": gpu_state(), "legs": legs}
        line = json.dumps(record)
        print(line)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.waterfall:
        fam = "zoom" if a.zoom else "real"
        path = a.out or os.path.join(ROOT, "profiles", "waterfall_probe.json")
        record = {}
        if os.path.exists(path):
            with open(path) as f:
                record = json.loads(f.read() or "{}")
        record.update({"metric": "waterfall_gsamples_s", "unit": "1e9 samples a second of one real stream",
                       "note": "findings, no gate: A is the spectral kurtosis object on the same device-resident stream, B the same segment "
                               "kernel with a round cut into one job a block and folded into ring slots; image_device: one call a stage, "
                               "host time to its return; not measured here: host memory, banks, other depths, block sizes between"})
        before = gpu_state()
        legs = waterfall_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, a.zoom)
        record[fam] = {"a": "ZoomSkCascadeBank" if a.zoom else "SkCascadeBank",
                       "b": "ZoomWaterfallCascadeBank" if a.zoom else "WaterfallCascadeBank",
                       "gpu_before": before, "gpu_after": gpu_state(), "legs": legs}
        line = json.dumps(record)
        print(line)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.ampm and a.pair:
        if not (a.zoom or a.iq):
            raise SystemExit("--pair --ampm goes with --zoom or --iq")
        path = a.out or os.path.join(ROOT, "profiles", "zoom_ampm_cross_probe.json")
        record = {}
        if os.path.exists(path):
            with open(path) as f:
                record = json.loads(f.read() or "{}")
        record.update({"metric": "zoom_ampm_cross_gpairs_s", "unit": "1e9 sample pairs a second (one sample of each side; complex for iq)",
                       "note": "findings, no gate: B is the AM/PM cross bank on one device-resident pair (two transforms a segment); A "
                               "is the two-pair recipe on the eight-row object (four); not measured here: host memory, banks, the EWMA "
                               "regime, N = 2048, two different carriers"})
        for fam, on in (("zoom", a.zoom), ("iq", a.iq)):
            if on:
                before = gpu_state()
                record[fam] = {"a": ("IqCsdCascadeBank(n, 2) fed (a, b) and (a, conj b)" if fam == "iq" else
                                     "ZoomCsdCascadeBank(n, 2): pairs (a:+ftw, b:+ftw) and (a:+ftw, b:-ftw)"),
                               "b": "IqAmPmCsdCascadeBank" if fam == "iq" else "ZoomAmPmCsdCascadeBank", "gpu_before": before,
                               "legs": ampm_pair_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, fam == "iq"),
                               "gpu_after": gpu_state()}
        line = json.dumps(record)
        print(line)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.ampm:
        if not (a.zoom or a.iq):
            raise SystemExit("--ampm goes with --zoom or --iq")
        path = a.out or os.path.join(ROOT, "profiles", "zoom_ampm_probe.json")
        record = {}
        if os.path.exists(path):
            with open(path) as f:
                record = json.loads(f.read() or "{}")
        record.update({"metric": "zoom_ampm_gsamples_s", "unit": "1e9 samples a second of one stream (complex samples for iq)",
                       "note": "findings, no gate: B is the AM/PM bank on one device-resident stream; A is the (x, x) recipe on the "
                               "zoom cross object (vs_recipe) or the two-row object (vs_two_rows); not measured here: host memory, "
                               "banks, the EWMA regime, N = 2048"})
        for fam, on in (("zoom", a.zoom), ("iq", a.iq)):
            if on:
                before = gpu_state()
                rec = {"b": "IqAmPmCascadeBank" if fam == "iq" else "ZoomAmPmCascadeBank", "gpu_before": before}
                if fam == "zoom":
                    rec["vs_recipe"] = {"a": "ZoomCsdCascadeBank fed (x, x), carriers +ftw / -ftw",
                                        "legs": ampm_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, False, True)}
                rec["vs_two_rows"] = {"a": "IqCascadeBank" if fam == "iq" else "ZoomCascadeBank",
                                      "legs": ampm_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, fam == "iq", False)}
                rec["gpu_after"] = gpu_state()
                record[fam] = rec
        line = json.dumps(record)
        print(line)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.sk and (a.zoom or a.iq):
        path = a.out or os.path.join(ROOT, "profiles", "zoom_sk_probe.json")
        record = {}
        if os.path.exists(path):
            with open(path) as f:
                record = json.loads(f.read() or "{}")
        record.update({"metric": "zoom_sk_gsamples_s", "unit": "1e9 samples a second of one stream (complex samples for iq)",
                       "note": "findings, no gate: A is the first-moment object on the same device-resident stream, B the same "
                               "transform with the second accumulator set; not measured here: host memory, banks, the EWMA regime"})
        for fam, on in (("zoom", a.zoom), ("iq", a.iq)):
            if on:
                before = gpu_state()
                legs = zoom_sk_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2, fam == "iq")
                record[fam] = {"a": "IqCascadeBank" if fam == "iq" else "ZoomCascadeBank",
                               "b": "IqSkCascadeBank" if fam == "iq" else "ZoomSkCascadeBank",
                               "gpu_before": before, "gpu_after": gpu_state(), "legs": legs}
        line = json.dumps(record)
        print(line)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.sk:
        before = gpu_state()
        legs = sk_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2)
        line = json.dumps({"metric": "sk_gsamples_s", "unit": "1e9 samples a second of one real stream",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "findings, no gate: A runs two transforms and two decimations where B runs one of each; not measured "
                                   "here: host memory, banks, the EWMA regime (default averaging: every weight is 1)",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "sk_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.real_int:
        before = gpu_state()
        legs = real_int_legs(pkg, torch, a.seconds, a.reps)
        line = json.dumps({"metric": "real_int_gsamples_s", "unit": "1e9 samples a second (of each side for the pair object)",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "findings, no gate: host-fed, B moves 2 bytes a sample over the host link where A moves 4; "
                                   "device-resident, the PSD object's s16 route converts into the stream buffer (one extra pass) where "
                                   "its f32 route is read in place, and the pair object's converter stands where its copies stand; "
                                   "not measured here: s8, the matrix object, banks, a wider converter",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "real_int_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.iq and a.int_feed:
        before = gpu_state()
        legs = iq_int_legs(pkg, torch, a.seconds, a.reps, a.pair)
        entry_ = {"metric": "iq_int_gsamples_s", "object": "IqCsdCascadeBank" if a.pair else "IqCascadeBank",
                  "unit": "1e9 complex samples a second" + (" of each side" if a.pair else ""),
                  "gpu_before": before, "gpu_after": gpu_state(),
                  "note": "findings, no gate: B moves 4 bytes a complex sample over the host link where A moves 8, so B / A can be at most "
                          "about 2; the mixer runs beside the previous round, so D / C is expected near 1; not measured here: s8, the "
                          "real objects, banks, two different carriers with --pair (the shared-oscillator branch runs)",
                  "legs": legs}
        path = a.out or os.path.join(ROOT, "profiles", "iq_int_probe.json")
        try:
            with open(path) as f:
                record = json.load(f)
        except (OSError, ValueError):
            record = {}
        record["pair" if a.pair else "single"] = entry_
        line = json.dumps(record)
        print(json.dumps(entry_))
        with open(path, "w") as f:
            f.write(line + "\n")
        return
    if a.iq and a.pair:
        before = gpu_state()
        legs = iq_pair_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2)
        line = json.dumps({"metric": "iq_cross_gpairs_s", "unit": "1e9 sample pairs a second (one sample of each side; complex for B and C, "
                                                                  "real for A)",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "findings, no gate: A reads 8 bytes a sample pair where B and C read 16; no kernel trace was taken, so "
                                   "nothing is said about the split between the mixer and the round; not measured here: the planar route, "
                                   "host memory, frames, banks, two different carriers (B runs the shared-oscillator branch)",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "iq_cross_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.iq:
        before = gpu_state()
        legs = iq_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2)
        line = json.dumps({"metric": "iq_gsamples_s", "unit": "1e9 samples a second of one stream (complex for B and C, real for A)",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "findings, no gate: A reads 4 bytes a sample where B reads 8; not measured here: the planar route, host "
                                   "memory, frames, banks",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "iq_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.zoom and a.pair and a.frames:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        before = gpu_state()
        legs = zoom_pair_frames_legs(pkg, torch, a.seconds, a.reps)
        line = json.dumps({"metric": "zoom_cross_frames_gpairs_s",
                           "unit": "1e9 sample pairs a second (one sample of each of the two traces of a pair)",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "not measured here: frames in HOST memory (they go up through the object's 32 MB pinned staging slots "
                                   "into a 32 MB device buffer), the dword-store path (every call here starts 16-byte aligned), banks "
                                   "(more than one pair a launch)",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "zoom_cross_frames_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.zoom and a.frames:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        before = gpu_state()
        legs = zoom_frames_legs(pkg, torch, a.seconds, a.reps)
        line = json.dumps({"metric": "zoom_frames_gsamples_s", "unit": "1e9 samples a second and channel-sample for the four-carrier legs",
                           "gpu_before": before, "gpu_after": gpu_state(),
                           "note": "leg A's samples go up through the zoom object's 16 MB pinned staging slots (psdc_zoom_process); host FRAMES "
                                   "(not measured here) would go up in 16 MB slots too, half the pair object's 32 MB",
                           "legs": legs})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "zoom_frames_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.zoom and a.pair:
        before = gpu_state()
        legs = zoom_pair_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2)
        after = gpu_state()
        line = json.dumps({"metric": "zoom_cross_gpairs_s", "unit": "1e9 sample pairs a second (one sample of each of the two real streams)",
                           "gpu_before": before, "gpu_after": after, "legs": legs, "tone_image": zoom_pair_image(pkg, torch)})
        print(line)
        with open(a.out or os.path.join(ROOT, "profiles", "zoom_cross_probe.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.zoom:
        line = json.dumps({"metric": "zoom_gsamples_s", "unit": "1e9 samples a second of one real stream",
                           "legs": zoom_legs(pkg, torch, a.seconds, a.reps, 1 << a.call_log2)})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.matrix:
        if a.frames:
            out = {"metric": "csm_frames_gsampletimes_s", "legs": matrix_frames_legs(pkg, torch, a.seconds, a.reps)}
        else:
            out = {"metric": "csm_gsampletimes_s", "unit": "1e9 sample times a second (one sample of each of four streams)",
                   "only_a": a.only_a, "legs": matrix_legs(pkg, torch, a.seconds, a.reps, a.only_a)}
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.frames:
        line = json.dumps({"metric": "cross_frames_gpairs_s", "legs": frames_legs(pkg, torch, a.seconds)})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    call = 1 << a.call_log2
    legs = [rate(pkg, torch, n, p, call, a.seconds) for n in (512, 1024, 4096) for p in (1, 4)]
    host = host_leg(pkg, 1024, 1 << 22, a.seconds)
    best = max(l["hbm_frac"] for l in legs)
    print(json.dumps({"metric": "cross_gpairs_s", "legs": legs, "host_fed": host,
                      "roofline": {"bytes_per_pair": 8, "hbm_bytes_s": HBM, "best_frac": best},
                      "n1024_1pair_gpairs_s": next(l["gpairs_s"] for l in legs if l["n"] == 1024 and l["pairs"] == 1)}))


if __name__ == "__main__":
    main()
