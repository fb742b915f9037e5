"""Every one of the 288 separately compiled fused single-pass PSD kernels (tests/fused_instances.py) against the f64 oracle, on the
GPU, in the job shapes at which its run, team and workgroup logic can go wrong.

One test an instance, reached the way a caller reaches it (fused_instances.route: the window, finite AvgOpts, AdcDac frames or
f32 spans in device memory, $PSDC_FFT3=0 and $PSDC_NO_DOUBLE for the two documented switches; never PSDC_DBG_VARIANT), with
PSDC_DBG_FIXED_RUN=2, min_pairs = 1 and coalesce = 2 so that a short stream makes jobs of several workgroups, deep-stage jobs and
rounds of two spans.  The walk is fused_instances.shape_walk.  After every check point of the walk and at the end the handle is held
to the oracle by tests/test_gpu_parity.py::check_against_oracle over the samples taken so far: counters, Breaks, pendings and
frequencies exactly, spectra at the bounds of tests/conftest.py with the two f32 restatements as the yardstick of the widened bins; a
state without a segment has nothing but the exact parts.  No bound is new here.  The PSDC_DBG_PLAN lines of the case then prove that
its launches went to this instance and showed the shapes (fused_instances.check_plan)."""
import time

import numpy as np
import pytest

from conftest import test_signal as make_signal
from fused_instances import INSTANCES, batches_of, check_plan, instance_id, parse_plan, route, seed_of, shape_walk, walk_samples
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

WORST = {}  # family -> (worst relative error of a stage spectrum against the f64 oracle, as check_against_oracle returns it, case)
SLOWEST = [0.0, ""]
LSB = np.float32(4.096) * np.float32(2.5) / np.float32(32768)  # src/de/data.rs:28-35, in f32 as the reference computes it


@pytest.fixture(scope="module", autouse=True)
def report():
    """one summary of the module on stdout (shown with -s or -rA): the figures DESIGN.md quotes"""
    t0 = time.time()
    yield
    if WORST:
        print("\nfused instances: worst relative error against the f64 oracle: " +
              ", ".join(f"{fam} {w:.3g} ({what})" for fam, (w, what) in sorted(WORST.items())))
        print(f"fused instances: module {time.time() - t0:.0f} s, slowest case {SLOWEST[1]} {SLOWEST[0]:.2f} s")


def signal(pkg, n, total, seed):
    """white noise, a tone a fifth of a bin above zero and an offset: something for every detrend to remove"""
    return make_signal(pkg, total, seed=seed, tone=1.0, dc=3.0, f0=0.2 / n)


def frame_words(pkg, ora, n, total, seed, batches):
    """(the int16 words of the four traces on the wire, the f32 traces the reference decodes from them)"""
    words = np.stack([np.clip(np.round(signal(pkg, n, total, seed + 1000 * c).astype(np.float64) * 3000.0), -32768, 32767).astype(np.int16)
                      for c in range(4)])
    wire = words.copy()
    wire[2:] = (wire[2:].view(np.uint16) ^ np.uint16(0x8000)).view(np.int16)  # DAC words are offset binary (src/de/data.rs:64)
    traces = [words[c].astype(np.float32) * LSB for c in range(4)]
    data, _ = pkg.make_adcdac_frames(wire[:, :8 * batches], batches)  # the oracle's own decode of the first frame against the above
    st, _, nb, tr = ora.adcdac_decode(data)
    assert st == 0 and nb == batches and all(np.array_equal(tr[c], traces[c][:8 * batches]) for c in range(4))
    return wire, traces


@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_fused_instance(pkg, ora, gpu_required, monkeypatch, capfd, inst):
    import torch
    t0 = time.time()
    fam, n, detrend, ewma, form = inst
    r = route(inst)
    what = instance_id(inst)
    batches = batches_of(inst) if form == "frames" else None
    ops = shape_walk(n, form, batches)
    total = walk_samples(ops, batches)
    nch = 4 if batches else 1
    if batches:
        wire, streams = frame_words(pkg, ora, n, total, seed_of(inst), batches)
    else:
        streams = [signal(pkg, n, total, seed_of(inst))]
    capfd.readouterr()
    for k, v in r["env"].items():  # read when the handle is made
        monkeypatch.setenv(k, v)
    g = pkg.PsdCascadeBank(n, nch, window=pkg.Window.RECTANGULAR) if r["window"] == "rect" else pkg.PsdCascadeBank(n, nch)
    for k in r["env"]:
        monkeypatch.delenv(k)
    keep = []
    try:
        g.configure(min_pairs=1, coalesce=2)
        g.set_detrend(pkg.Detrend[detrend.upper()])
        avg = pkg.AvgOpts(*r["avg"]) if r["avg"] else None
        if avg:
            g.set_avg(avg)
        taken, seq, checks, worst = 0, 0, 0, 0.0
        frames_end = None

        def check(channels, when):
            w = 0.0
            for c in channels:
                w = max(w, check_against_oracle(pkg, ora, g, [streams[c][:taken]], n, detrend=detrend, avg=avg, window=r["window"],
                                                channel=c, what=f"{what} {when} ({taken} samples) channel {c}"))
            return w

        for i, op in enumerate(ops):
            if op[0] == "f32":
                # sample i of the stream sits 16-byte aligned where i is a multiple of 4 -- segments start aligned, the fused path -- or,
                # for the one misaligned call, 4 bytes behind that: the planner's fallback to the generic kernels
                off = taken % 4 + int(op[2])
                t = torch.empty(op[1] + 8, dtype=torch.float32, device="cuda")
                assert t.data_ptr() % 16 == 0
                t[off:off + op[1]] = torch.from_numpy(streams[0][taken:taken + op[1]]).cuda()
                torch.cuda.synchronize()
                keep.append(t)
                g.process_device(0, t.data_ptr() + 4 * off, op[1])
                taken += op[1]
            elif op[0] == "frames":
                per = 8 * batches
                data, fs = pkg.make_adcdac_frames(wire[:, taken:taken + op[1] * per], batches, seq0=seq)
                if op[2]:  # continues the held run in memory: room was left behind the call before
                    ptr = frames_end
                    keep[-1][ptr - keep[-1].data_ptr():ptr - keep[-1].data_ptr() + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
                else:
                    follow = ops[i + 1][1] * fs if i + 1 < len(ops) and ops[i + 1][0] == "frames" and ops[i + 1][2] else 0
                    # (64 spare bytes: the next call's buffer must not start where this one ends, or the two would merge into one run)
                    t = torch.empty(len(data) + follow + 64, dtype=torch.uint8, device="cuda")
                    assert t.data_ptr() % 8 == 0
                    t[:len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
                    keep.append(t)
                    ptr = t.data_ptr()
                torch.cuda.synchronize()
                assert g.process_adcdac_frames_device(ptr, fs, op[1]) == op[1]
                frames_end = ptr + len(data)
                seq = (seq + op[1] * batches) & 0xFFFFFFFF
                taken += op[1] * per
            else:
                worst = max(worst, check([checks % nch], f"after call {checks}"))  # (frames: one trace in turn, all four at the end)
                checks += 1
        assert taken == total
        if batches:
            assert g.loss() == {"received": total // 8, "dropped": 0}
        worst = max(worst, check(range(nch), "at the end"))
    finally:
        g.close()
        del keep
    err = capfd.readouterr().err
    try:
        check_plan(inst, parse_plan(err))
    except AssertionError as e:
        raise AssertionError(f"{e}\n{err}") from None
    if worst > WORST.get(fam, (0.0, ""))[0]:
        WORST[fam] = (worst, what)
    dt = time.time() - t0
    if dt > SLOWEST[0]:
        SLOWEST[:] = [dt, what]
