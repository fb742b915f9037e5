"""Every separately compiled fused single-pass PSD kernel behind PsdCascade, the route that reaches each through the public objects,
and the walk that holds each to the f64 oracle at its own job edges (a plain helper module, no tests of its own; tests/
test_fused_instances_host.py checks it without a GPU, tests/test_gpu_fused_instances.py runs it).

Three families -- fused_kernel<N> (the team kernels, N = 256, 512, 1024: csrc/fused.hip), bigfused3_kernel<N> (three passes, 2048 and
4096: csrc/bigfused3_impl.h) and bigfused_kernel<N> (four passes, 2048 ... 16384: csrc/bigfused_impl.h) -- are nine (family, N); each
is compiled for 4 detrends x {plain sum, EWMA} x {pair, pair + frames, SINGLE = 1, SINGLE = 2}: 288 kernels.  The launch switches
choose among them from the size, the twiddle seeds ($PSDC_FFT3), FusedBatch::detrend, any_ewma, any_frames and single; the
PSDC_DBG_PLAN line of csrc/planner.cpp prints exactly those, so a case can prove which kernel its launches went to.

A launch runs the LEAST specialised kernel that serves its jobs: an EWMA handle's launches go to the plain-sum kernel until a
stage's count passes its limit (plan_ewma: all weights 1 until then), and a frames stream's launches without a framed job (calls
too short to be read in place are decoded into the stage-0 stream; read-out rounds of the deep stages) go to the kernel without
the frame loads.  So a case's launches name its instance or a sibling with ewma / frames cleared, never another family, size,
detrend or single form; and at least one names the instance exactly.

What the kernels make impossible, and how the conditions of the issue are read there:
  * SINGLE = 2 transforms two segments at once: every job holds an even number of segments and `run` is even (np &= ~1 in
    make_jobs).  Its unit is two segments: jobs of 2, P - 2, P, P + 2 and 2 P + 2 segments, and a call that leaves an odd last
    segment to the generic kernels.
  * N >= 2048 has one team a workgroup: with PSDC_DBG_FIXED_RUN=2 no job is "small" (4 pairs <= 2 teams never holds), so the deep-
    stage condition there is a deep-stage job in one workgroup; at N <= 1024 it must be small.
  * Seams ride as job prologues only in rounds of one launch at N <= 1024 (Round::fold_seams), and never for frame spans, whose
    seams post_kernel decodes: the seam condition is held for the f32 forms at N <= 1024.
  * An in-place span is split in a buffer side (the pairs that begin in the carried tail: one or two) and an in-place side; the
    edge shapes are asked of JOBS, so a call completes the in-place job's pairs plus the buffer side's (stage0_jobs restates
    the split; the host test holds the restatement to the planner's own lines)."""
import functools

from settings_schedule import DETRENDS, U32_MAX, segments_after

HALO, DRAIN = 288, 35  # HBF_HALO, HBF_DRAIN of csrc/hbf_taps.h

# (family, n) in launch order of csrc/fused.hip launch_fused
FAMILY_SIZES = (("fused", 256), ("fused", 512), ("fused", 1024), ("bigfused3", 2048), ("bigfused3", 4096),
                ("bigfused", 2048), ("bigfused", 4096), ("bigfused", 8192), ("bigfused", 16384))
FORMS = ("pair", "frames", "single1", "single2")
INSTANCES = tuple((fam, n, d, e, form) for fam, n in FAMILY_SIZES for d in DETRENDS for e in (False, True) for form in FORMS)
assert len(INSTANCES) == 288 and len(set(INSTANCES)) == 288

FIXED_RUN = 2
EWMA = (3, U32_MAX)  # limit 3 at every stage: stage 0 is in its steady EWMA from the fifth segment on
BATCHES = (1, 7, 22)


def teams(n):
    """teams (= pairs in flight) a workgroup: FusedGeo<N>::TEAMS = 8 waves x 64 / (N / 16) lanes at N <= 1024, the whole workgroup above"""
    return {256: 32, 512: 16, 1024: 8}.get(n, 1)


def pairs_per_workgroup(n):
    return FIXED_RUN * teams(n)


def instance_id(inst):
    fam, n, d, e, form = inst
    return f"{fam}-{n}-{d}-{'ewma' if e else 'sum'}-{form}"


def seed_of(inst):
    return 7000 + INSTANCES.index(inst)


def batches_of(inst):
    """the AdcDac batches a frame of a frames instance: 1 (FrameSpan::magic's special case), 7 or 22, spread so that every
    (family, n) sees all three"""
    i = INSTANCES.index(inst)
    return BATCHES[(i // 4 + i // 32) % 3]


def route(inst):
    """how a caller reaches the instance: {env: variables set while the handle is made, window, avg (limit, count) or None,
    source: f32 | frames, single: FusedBatch::single}"""
    fam, n, d, e, form = inst
    env = {"PSDC_DBG_PLAN": "1", "PSDC_DBG_FIXED_RUN": str(FIXED_RUN)}
    if fam == "bigfused" and n in (2048, 4096):
        env["PSDC_FFT3"] = "0"
    if form == "single1":
        env["PSDC_NO_DOUBLE"] = "1"
    return {"env": env, "window": "rect" if form.startswith("single") else "hann", "avg": EWMA if e else None,
            "source": "frames" if form == "frames" else "f32", "single": {"single1": 1, "single2": 2}.get(form, 0)}


# ---- a restatement of the stage-0 split of csrc/planner.cpp (collect_work, make_jobs), used only to BUILD walks ----

def _segs(n, hop, total):
    return 0 if total < n else 1 + (total - n) // hop


def stage0_jobs(n, mode, taken, length):
    """(pairs of the buffer-side fused job, pairs of the in-place one, segments left to the generic kernel) of a device call of
    `length` samples behind `taken`, in a round of its own (0: no such job).  mode = FusedBatch::single."""
    half, hop, step = n // 2, (n if mode else n // 2), (1 if mode else 2)
    need_pre = max(0, HALO - half)
    seam = max(n + HALO, need_pre + 3 * half)
    new0 = lambda s: s * hop + (0 if mode else half)
    j_lo, j_hi = _segs(n, hop, taken), _segs(n, hop, taken + length)

    def fused(a, b):
        fs = a
        while new0(fs) // 8 < DRAIN:
            fs += step
        np_ = (b - fs) // step if fs + step <= b else 0
        return np_ & ~1 if mode == 2 else np_

    if length < 4 * (n + HALO) or j_lo == 0:
        jobs = [fused(j_lo, j_hi), 0]
    else:
        js = max(j_lo, -(-(taken + need_pre + (half if mode else 0)) // hop))
        if not mode and (js - j_lo) & 1:
            js += 1
        if js < j_hi and new0(js) <= taken + seam and length >= seam:
            split = js
        else:
            split = min(j_hi, max(j_lo, -(-taken // hop)))
        jobs = [fused(j_lo, split), fused(split, j_hi)]
    return jobs[0], jobs[1], (j_hi - j_lo) - step * (jobs[0] + jobs[1])


# ---- the walk ----

PEND = (1, 2, 3, 5, 7)


def job_targets(n, mode):
    """the pairs of the jobs the walk must show, in walk order.  P = pairs a workgroup: one pair in an otherwise idle workgroup, the
    last team short by one, exactly full, a second workgroup with one pair, three workgroups, and the one pair again (an EWMA
    stage 0 has passed its limit by then, so this one runs on the EWMA kernel); SINGLE = 2 in its unit of two segments, with
    P + 1 in between: the call that leaves an odd last segment."""
    p = pairs_per_workgroup(n)
    want = (2, p - 2, p, p + 1, p + 2, 2 * p + 2) if mode == 2 else (1, p - 1, p, p + 1, 2 * p + 1)
    out = []
    for c in want:
        if c > 0 and c not in out:
            out.append(c)
    return out + out[:1]


def shortfalls(n, mode):
    """workgroups x P - pairs that must occur among a case's jobs: exactly full, short by one unit, one unit in the last workgroup"""
    p, u = pairs_per_workgroup(n), (2 if mode == 2 else 1)
    return sorted({s for s in (0, u, p - u) if 0 <= s <= p - u})


@functools.lru_cache(maxsize=None)
def shape_walk(n, form, batches=None):
    """The operations of one instance's walk, a pure function of its arguments: ("f32", samples, misaligned), ("frames", frames,
    continues the buffer of the call before), ("check",).  Every call is followed by a check but where spans are to share a round.

    1. n - 1 samples (frames: the most whole frames below n): no segment.
    2. one call for each of job_targets: the shortest call for which stage0_jobs shows a job of exactly that many pairs (frames:
       a framed job where an in-place call can have one so small).
    3. two in-place spans in memory of their own, held into one round (coalesce = 2) that leaves nothing to the generic kernels,
       and a third that sends the round out on the ingest path -- so the round can be one launch, its seams prologues -- then the
       check.
    4. frames: a call that shows a four-trace group of exactly 8 workgroups, one of 8 k + r, and a call continuing the held run
       in memory (merged into its span: a later job of the run starts at s_off != 0).
    5. f32: one in-place call at a 4-byte offset: the planner's fallback to the generic kernels in mid-stream.
    6. two calls that bring stage 2 to its first segment: the deep stages' jobs ride in the same launches."""
    mode = {"single1": 1, "single2": 2}.get(form, 0)
    framed = form == "frames"
    q = 8 * batches if framed else 1  # samples a call's length is a multiple of
    thr = 4 * (n + HALO)
    p = pairs_per_workgroup(n)
    ops, taken = [], 0

    def add(length, flag=False, check=True):
        nonlocal taken
        assert length > 0 and length % q == 0
        ops.append(("frames", length // q, flag) if framed else ("f32", length, flag))
        taken += length
        if check:
            ops.append(("check",))

    def shortest(pred, lo, span=None):
        """the shortest call of at least `lo` samples whose stage-0 jobs meet pred; f32 calls end a few samples (PEND) behind a
        half segment.  None if no call of up to lo + span samples does."""
        span = 4 * n + thr if span is None else span
        if framed:
            cands = range(-(-max(lo, q) // q) * q, lo + span + q, q)
        else:
            pend = PEND[len(ops) % len(PEND)]
            m0 = max(0, (taken + lo - pend) // (n // 2))
            # (overlap 0: behind an odd number of half segments, so that the buffer side of the next in-place span holds two segments)
            cands = (m * (n // 2) + pend - taken for m in range(m0, m0 + 2 * span // n + 4) if m & 1 or not mode)
        for length in cands:
            if length >= max(lo, 1) and pred(stage0_jobs(n, mode, taken, length)):
                return length
        return None

    if (n - 1) // q:
        add((n - 1) // q * q)
    for c in job_targets(n, mode):
        length = shortest(lambda j: j[1] == c, c * n - n // 2) if framed else None
        if length is None and mode == 2 and c & 1:  # the odd last segment goes to the generic kernel
            length = shortest(lambda j: j[1] == c - 1 and j[2] & 1, c * n - n // 2)
        elif length is None:
            length = shortest(lambda j: c in j[:2], c * n - n // 2)
        add(length)
    for i in range(3):  # two spans a round, then the call that cannot join
        add(shortest(lambda j: j[0] > 0 and j[1] > 0 and j[2] == 0, thr), check=(i == 2))
    if framed:
        add(shortest(lambda j: -(-j[1] // p) == 8, 7 * p * n))
        add(shortest(lambda j: -(-j[1] // p) > 8 and -(-j[1] // p) % 8 != 0, 8 * p * n))
        add(shortest(lambda j: j[1] > 0, thr), check=False)
        add(-(-(n + 8) // q) * q, True)
    else:
        add(shortest(lambda j: j[1] > 0, thr), True)
    hop = n if mode else n // 2  # stage 2's first segment, in two calls
    need = taken
    while True:
        s = segments_after(n, n - hop, need)
        if len(s) >= 3 and s[2] >= 1:
            break
        need += n
    rest = -(-(need + PEND[2] - taken) // q) * q if need > taken else 0
    if rest > 0:
        first = max(q, rest // 2 // q * q)
        add(first)
        if rest - first > 0:
            add(rest - first)
    return tuple(ops)


def walk_samples(ops, batches=None):
    return sum(op[1] * (8 * batches if op[0] == "frames" else 1) for op in ops if op[0] != "check")


def host_script(insts):
    """the cases as tests/host/fused_walk_check.cpp reads them"""
    lines = []
    for inst in insts:
        fam, n, d, e, form = inst
        r = route(inst)
        b = batches_of(inst) if form == "frames" else None
        limit, count = r["avg"] or (U32_MAX, U32_MAX)
        lines.append(" ".join([f"case {instance_id(inst)} {n} {int(r['window'] == 'rect')} {4 if b else 1} {DETRENDS.index(d)} {limit} {count}"] +
                              [f"{k}={v}" for k, v in r["env"].items()]))
        for op in shape_walk(n, form, b):
            lines.append("check" if op[0] == "check" else f"{op[0]} {op[1]} {int(op[2])}" + (f" {b}" if b else ""))
        lines.append("end")
    return "\n".join(lines) + "\n"


def split_cases(text):
    """{case id: its lines} of the stderr of a run that prints `case <id>` in front of each case"""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(line.split()[1], [])
        elif cur is not None:
            cur.append(line)
    return {k: "\n".join(v) for k, v in out.items()}


# ---- the PSDC_DBG_PLAN lines of a case ----

def parse_plan(text):
    """the fused launches of a case's stderr: [{family, n, detrend, ewma, frames, single, groups: [workgroups], jobs: [{pairs, wg,
    run, seam, stage, step0, framed}]}]"""
    out = []
    for line in text.splitlines():
        if not line.startswith("fused launch:"):
            continue
        head, kern = line.split(" | kernel ")
        kw = kern.split()
        launch = {"family": kw[0]}
        for w in kw[1:]:
            key, val = w.split("=")
            launch[key] = [int(v) for v in val.strip("[]").split(",") if v] if key == "groups" else int(val)
        jobs = []
        for w in head.split("pairs:")[1].split():
            shape, at = w.split("@")
            pr, wg, run = shape.split("/")
            stage, step0 = at.rstrip("f").split(".")
            jobs.append({"pairs": int(pr[:-1]), "wg": int(wg[:-2]), "run": int(run.rstrip("s")[1:]), "seam": run.endswith("s"),
                         "stage": int(stage), "step0": int(step0), "framed": at.endswith("f")})
        launch["jobs"] = jobs
        assert len(jobs) == int(head.split()[2]), line
        out.append(launch)
    return out


def check_plan(inst, launches):
    """the conditions of a case on its launches (module docstring); raises AssertionError naming the one that is not met"""
    fam, n, d, e, form = inst
    r = route(inst)
    what = instance_id(inst)
    p, t = pairs_per_workgroup(n), teams(n)
    assert launches, what
    exact = 0
    for la in launches:
        assert (la["family"], la["n"], la["detrend"], la["single"]) == (fam, n, DETRENDS.index(d), r["single"]), (what, la)
        assert la["ewma"] <= int(e) and la["frames"] <= int(form == "frames"), (what, la)
        assert la["frames"] == int(any(j["framed"] for j in la["jobs"])), (what, la)
        exact += (la["ewma"], la["frames"]) == (int(e), int(form == "frames"))
    assert exact >= 1, f"{what}: no launch went to the instance itself"
    mine = [la for la in launches if (la["ewma"], la["frames"]) == (int(e), int(form == "frames"))]
    framed = form == "frames"
    # frames: calls too short to be read in place are decoded, their jobs are f32 jobs of the sibling kernel -- the unit job, the
    # shortfalls and the three workgroups are asked of the case's stage-0 jobs, framed or not, and of the framed ones a full and a
    # short last workgroup besides the group shapes below
    jobs = [j for la in (launches if framed else mine) for j in la["jobs"] if j["stage"] == 0]
    unit = 2 if r["single"] == 2 else 1
    assert any(j["pairs"] == unit for j in jobs), f"{what}: no job of one unit"
    got = {j["wg"] * p - j["pairs"] for j in jobs if j["run"] == FIXED_RUN}
    assert set(shortfalls(n, r["single"])) <= got, f"{what}: shortfalls {sorted(got)}"
    assert any(j["wg"] == 3 for j in jobs), f"{what}: no job of three workgroups"
    if n <= 1024 and not framed:
        assert any(j["seam"] for j in jobs), f"{what}: no seam prologue"
    deep = [j for la in mine for j in la["jobs"] if j["stage"] >= 1]
    if n <= 1024:
        assert any(4 * j["pairs"] <= FIXED_RUN * t and j["wg"] == 1 for j in deep), f"{what}: no small deep-stage job"
    else:
        assert any(j["wg"] == 1 for j in deep), f"{what}: no deep-stage job"
    assert sum(j["stage"] == 1 for la in launches for j in la["jobs"]) >= 2, f"{what}: fewer than two stage-1 jobs"
    if e:
        assert any(len({j["step0"] for j in la["jobs"] if j["stage"] == 0}) >= 2 for la in mine), f"{what}: no launch with two step0"
    if framed:
        fj = [j for la in mine for j in la["jobs"] if j["framed"]]
        short = {j["wg"] * p - j["pairs"] for j in fj if j["run"] == FIXED_RUN}
        assert 0 in short and short - {0} and any(j["wg"] >= 3 for j in fj), f"{what}: framed shortfalls {sorted(short)}"
        sizes = [g for la in mine for g in la["groups"]]
        assert any(g < 8 for g in sizes) and any(g == 8 for g in sizes) and any(g > 8 and g % 8 for g in sizes), f"{what}: groups {sizes}"
        assert any(j["stage"] >= 1 and not j["framed"] for la in mine for j in la["jobs"]), f"{what}: no f32 job in a FRAMES launch"
