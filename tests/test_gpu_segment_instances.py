"""Every one of the 69 separately compiled segment kernels (tests/segment_instances.py) against the f64 restatement of its family,
on the GPU, in the job shapes at which its tile logic can go wrong.

One test an instance: a bank of two units, both fed segment_instances.shape_walk of the instance's own tile size -- a call without
a segment, then 1, SPT - 1, SPT, SPT + 1 and 2 SPT + 1 new stage-0 segments, then enough for three stage-2 segments, whose deeper
stages are jobs below one tile.  Unit 0 is fed from host memory; unit 1 from device memory behind an odd number of elements, one
call behind unit 0, so that the rounds hold jobs of two sizes.  Detrend, averaging and window are set before the first sample
(segment_instances.settings_of) and enter the restatement as the initial settings of a Schedule without events.

After each call of a unit and at the end the unit is held to the restatement over the samples it has taken, with the machinery of
tests/test_gpu_settings_midstream.py: stages, counts, averages, pendings and Breaks exactly; rows and stitched read-outs by the
family's own helpers at their own bounds, the f32 sibling as the yardstick of the widened ones.  No bound is new here."""
import numpy as np
import pytest

from segment_instances import DEFAULT_AVG, INSTANCES, TILE, instance_id, seed_of, settings_of, shape_walk
from settings_schedule import UNITS, Schedule, segments_after
from test_gpu_cross import DETRENDS
from test_gpu_settings_midstream import FAMILIES, Case, Zoom, ZoomCsd, device_buffers, exact
from test_iq_host import iq_emul  # noqa: F401
from test_zoom_host import emul  # noqa: F401

pytestmark = pytest.mark.gpu

OFFSETS = (1, 3, 5, 7)  # the elements a device call's pointer lies behind its allocation's start
# kind -> (the call that reads a stage, the stitched read-out): what the family's check reads
READS = {"cross": ("stage_spectra", "csd"), "csm": ("stage_spectra", "csd"), "zoom": ("stage_spectra", "psd"), "zcsd": ("stage_spectra", "csd"),
         "sk": ("stage_moments", "psd"), "zsk": ("stage_moments", "psd"), "zampm": ("stage_rows", "psd"), "zxampm": ("stage_rows", "csd")}


def check_no_segment(c, bank, u, st64, what):
    """a unit that has completed no segment (the walk's first call): the value helpers have nothing to hold, so the stages'
    counts, averages and pendings, the Breaks and the width of the stitched read-out, all exactly"""
    st = next(iter(st64.values())) if isinstance(st64, dict) else st64  # (csm restates pair by pair; the stages are the unit's)
    assert st and all(s["count"] == 0 for s in st), what
    stage, readout = READS[c.kind]
    exact([getattr(bank, stage)(u, k)[0] for k in range(bank.num_stages(u))], st, what)
    ref, rbr = c.pkg.stitch(c.n, [0] * len(st), [s["avg"] for s in st], [s["pending"] for s in st],
                            np.zeros((len(st), c.n // 2 + 1), np.float32), c.pkg.MergeOpts(), window=c.wt)
    out = getattr(bank, readout)(u)
    assert out[-1] == rbr, (what, out[-1], rbr)
    assert all(np.asarray(a).shape[-1] == ref.size for a in out[:-1]), (what, [np.asarray(a).shape for a in out[:-1]], ref.size)


@pytest.mark.parametrize("inst", INSTANCES, ids=instance_id)
def test_segment_instance(pkg, ora, gpu_required, emul, iq_emul, inst):  # noqa: F811
    kind, n, m = inst
    detrend, avg, wkind = settings_of(inst)
    fam = FAMILIES[kind]
    c = Case(pkg, ora, kind, n, wkind, (emul, iq_emul), **({} if m is None else {"m": m}))
    calls = shape_walk(n, c.overlap, TILE[inst])
    total = sum(calls)
    planes = [fam.input(c, total, seed_of(inst, u)) for u in range(UNITS)]
    assert all(len(p) == fam.sides_of(c) and all(v.size == total for v in p) for p in planes)
    # step i: call i of unit 0 from the host, then call i - 1 of unit 1 from the device
    steps = [[("host", 0, length, None) for length in calls[i:i + 1]] +
             [("device", 1, length, None, OFFSETS[i % 4]) for length in calls[max(i - 1, 0):i]] for i in range(len(calls) + 1)]
    walk = [op for step in steps for op in step]
    keep, ptrs = device_buffers(walk, planes, False)
    bank = fam.make(c)
    fam.carriers(c, bank)
    bank.set_detrend(DETRENDS[detrend])
    if avg != DEFAULT_AVG:
        bank.set_avg(pkg.AvgOpts(*avg))
    sched = Schedule(n, c.overlap, [], detrend=detrend, avg=avg)
    mixed = isinstance(fam, (Zoom, ZoomCsd))
    pos = [0] * UNITS
    restated = {}

    def check(u, when):
        taken = pos[u]
        segs = segments_after(n, c.overlap, taken)
        src = planes[u] if mixed else [p[:taken] for p in planes[u]]
        kw = {"taken": taken} if mixed else {}
        if (u, taken) not in restated:  # (the end reads the state of the last call again)
            restated[u, taken] = [fam.restate(c, u, src, prec, sched, **kw) for prec in ("f64", "f32")]
        st64, st32 = restated[u, taken]
        assert bank.num_stages(u) == len(segs), (when, u, bank.num_stages(u), segs)
        if not any(segs):
            return check_no_segment(c, bank, u, st64, f"{instance_id(inst)} unit {u} {when}")
        fam.check(c, bank, u, sched, segs, src, st64, st32, f"{instance_id(inst)} unit {u} {when}", **kw)

    at = 0
    for i, step in enumerate(steps):
        for op in step:
            u, length = op[1], op[2]
            parts = [p[pos[u]:pos[u] + length] for p in planes[u]]
            if op[0] == "host":
                fam.host(c, bank, u, parts, None)
            else:
                fam.device(c, bank, u, ptrs[at], length, None)
            pos[u] += length
            at += 1
        for op in step:
            check(op[1], f"after call {i - op[1]} ({pos[op[1]]} samples)")
    assert pos == [total] * UNITS
    for u in range(UNITS):
        check(u, "at the end")
    bank.close()
    del keep
