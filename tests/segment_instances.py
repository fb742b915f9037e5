"""Every separately compiled segment kernel of the cross-spectral runtime, and the walk that holds each to its f64 restatement (a
plain helper module, no tests of its own; tests/test_segment_instances_host.py checks it without a GPU, tests/
test_gpu_segment_instances.py runs it).

Seven kernels are templated on N (64 ... 4096), csm_kernel on (N, M): 7 x 7 + 20 = 69 instances.  Detrend, averaging and window are
run-time arguments, so these are all the code there is; each instance has a workgroup shape of its own (cross_channel.h,
csm_fft.h), and a compiler fault hits one instance.  An instance is reached through the real-input kind that runs it.  The IQ
kinds and the waterfalls stay out: they launch the same segment kernels, and what is their own -- the complex mixers, and the
fresh-block fold of CrossFoldJob -- has no N template; their own suites and the walks of tests/test_gpu_settings_midstream.py
hold those."""
from settings_schedule import DETRENDS, U32_MAX, segments_after

SIZES = (64, 128, 256, 512, 1024, 2048, 4096)

# kind -> the kernel it launches (csrc/cross_runtime.cpp, KINDS[])
KERNELS = {"cross": "cross_kernel", "sk": "sk_kernel", "zoom": "zoom_kernel", "zsk": "zoom_sk_kernel", "zampm": "zoom_ampm_kernel",
           "zcsd": "zoom_cross_kernel", "zxampm": "zoom_ampm_cross_kernel", "csm": "csm_kernel"}
PAIR_KINDS = ("cross", "sk")  # a team takes a segment pair a tile; the zoom kernels one segment

# csm_kernel<N, M>: PSDK_CSM_CASES of csrc/csm.hip
CSM_SHAPES = tuple((n, m) for n in SIZES for m in (2, 3, 4) if (n, m) != (4096, 4))

# (kind, n, m): m is None but for csm
INSTANCES = tuple((kind, n, None) for kind in KERNELS if kind != "csm" for n in SIZES) + tuple(("csm", n, m) for n, m in CSM_SHAPES)
assert len(INSTANCES) == 69

# The workgroup of the seven team kernels, n -> (threads, teams): csrc/cross_channel.h:16-18, seg_team = n / 16, seg_block =
# max(seg_team, 128), seg_teams = seg_block / seg_team (the static_assert of lines 35-37 spells the seven out)
TEAM_SHAPE = {64: (128, 32), 128: (128, 16), 256: (128, 8), 512: (128, 4), 1024: (128, 2), 2048: (128, 1), 4096: (256, 1)}
# csm_kernel's, (n, m) -> (BLOCK, TEAMS, SPT, PG, GS): csrc/csm_fft.h:50-54.  BLOCK is 256 unless the frames of 256 threads
# overflow the LDS (64 teams of 4 frames at n = 64, m = 4); GS = min(n / 2, BLOCK) threads a product group, PG = BLOCK / GS
CSM_SHAPE = {
    (64, 2): (256, 64, 128, 8, 32), (64, 3): (256, 64, 128, 8, 32), (64, 4): (128, 32, 64, 4, 32),
    (128, 2): (256, 32, 64, 4, 64), (128, 3): (256, 32, 64, 4, 64), (128, 4): (256, 32, 64, 4, 64),
    (256, 2): (256, 16, 32, 2, 128), (256, 3): (256, 16, 32, 2, 128), (256, 4): (256, 16, 32, 2, 128),
    (512, 2): (256, 8, 16, 1, 256), (512, 3): (256, 8, 16, 1, 256), (512, 4): (256, 8, 16, 1, 256),
    (1024, 2): (256, 4, 8, 1, 256), (1024, 3): (256, 4, 8, 1, 256), (1024, 4): (256, 4, 8, 1, 256),
    (2048, 2): (256, 2, 4, 1, 256), (2048, 3): (256, 2, 4, 1, 256), (2048, 4): (256, 2, 4, 1, 256),
    (4096, 2): (256, 1, 2, 1, 256), (4096, 3): (256, 1, 2, 1, 256),
}
# Segments a tile.  cross and sk: one pair a team, seg_spt = 2 seg_teams (cross_channel.h:19; cross.hip and sk.hip call seg_pair
# with it).  The zoom kernels: one segment a team, one_seg<TEAMS> (segment_kernel.h:44-50).  csm: CsmShape<N, M>::SPT = 2 TEAMS
# (csm_fft.h:52).
PAIR_TILE = {64: 64, 128: 32, 256: 16, 512: 8, 1024: 4, 2048: 2, 4096: 2}
ZOOM_TILE = {64: 32, 128: 16, 256: 8, 512: 4, 1024: 2, 2048: 1, 4096: 1}
TILE = {inst: CSM_SHAPE[inst[1:]][2] if inst[0] == "csm" else (PAIR_TILE if inst[0] in PAIR_KINDS else ZOOM_TILE)[inst[1]]
        for inst in INSTANCES}


def instance_id(inst):
    kind, n, m = inst
    return f"{kind}-{n}" if m is None else f"{kind}-{n}x{m}"


# ---- the settings of an instance: fixed before the first sample, spread over the instances by index ----

EWMA = (3, U32_MAX)
DEFAULT_AVG = (U32_MAX, U32_MAX)
_TEAM_KINDS = [k for k in KERNELS if k != "csm"]


def _detrend(i):
    return DETRENDS[i % 4]


def _custom_size(j):
    """the first size from SIZES[(j + 2) % 5] on, other than the rectangular case's, whose detrend is none or mean: the
    anchored-detrend allowance of bins 0 and 1 (conftest.anchored_terms) is written for the Hann and the rectangular window"""
    for d in range(5):
        s = (j + 2 + d) % 5
        if s != j % 5 and _detrend(7 * j + s) in ("none", "mean"):
            return SIZES[s]


# One rectangular and one caller-window case a kernel, all others Hann: kernel j of the seven at the sizes SIZES[j % 5] and
# _custom_size(j) (up to 1024: a hop of n needs twice the samples for three stage-2 segments), csm at two shapes no parity case
# has.
WINDOWS = {(kind, SIZES[j % 5], None): "rect" for j, kind in enumerate(_TEAM_KINDS)}
WINDOWS.update({(kind, _custom_size(j), None): "custom" for j, kind in enumerate(_TEAM_KINDS)})
WINDOWS.update({("csm", 128, 2): "rect", ("csm", 512, 3): "custom"})
assert len(WINDOWS) == 16 and set(WINDOWS) <= set(INSTANCES)


def settings_of(inst):
    """(detrend, avg (limit, count), window kind) of an instance.  Index i takes detrend i mod 4 and the EWMA where i + i // 4 is
    odd, so eight consecutive instances see the eight combinations and the seven sizes of a kernel seven of them."""
    i = INSTANCES.index(inst)
    return _detrend(i), EWMA if (i + i // 4) % 2 else DEFAULT_AVG, WINDOWS.get(inst, "hann")


def seed_of(inst, unit):
    return 5000 + 10 * INSTANCES.index(inst) + unit


# ---- the walk ----

PEND = (1, 2, 3, 5, 7)  # the samples a call leaves pending, in turn; the last call leaves 3
LAST_PEND = 3


def _samples(n, hop, nseg):
    return n + (nseg - 1) * hop if nseg else 0


def shape_walk(n, overlap, spt):
    """The call lengths of one unit, a pure function of its arguments.  The first call has n - 1 samples: no segment, a job of no
    workgroup.  Then one call for each of these counts of new stage-0 segments, duplicates and zeros dropped: 1, spt - 1, spt,
    spt + 1, 2 spt + 1 -- fewer segments than a tile has, exactly one tile, one tile and a segment, two tiles and an odd one --
    each leaving a few samples pending.  A last call brings stage 2 to three completed segments, if it has not got them."""
    hop = n - overlap
    counts = []
    for c in (1, spt - 1, spt, spt + 1, 2 * spt + 1):
        if c > 0 and c not in counts:
            counts.append(c)
    calls, taken, nseg = [n - 1], n - 1, 0
    for i, c in enumerate(counts):
        nseg += c
        upto = _samples(n, hop, nseg) + PEND[i]
        calls.append(upto - taken)
        taken = upto
    last = nseg
    while True:
        s = segments_after(n, overlap, _samples(n, hop, last) + LAST_PEND)
        if len(s) >= 3 and s[2] >= 3:
            break
        last += 1
    if last > nseg:
        calls.append(_samples(n, hop, last) + LAST_PEND - taken)
    assert all(c > 0 for c in calls)
    return calls


def overlap_of(n, wkind):
    """the overlap of the window kinds of test_zoom_host.windows_of: Hann n / 2, rectangular none, the caller's sqrt-Hann n / 4"""
    return {"hann": n // 2, "rect": 0, "custom": n // 4}[wkind]
