"""tests/fused_instances.py held to the source and to the planner, without a GPU: INSTANCES is exactly the product the three launch
switches compile (tests/host/fused_walk_check.cpp --instances prints families, sizes and teams from the launch switch's own family
function and the geometry headers; the switches' template arguments are read from the source), every instance's walk meets its
conditions when the library's host runtime plans it on the CPU model of tests/host/sim (the PSDC_DBG_PLAN lines are parsed by the
functions the GPU test uses), also under AddressSanitizer + UBSan, and the settings spread over every variant.  A walk that cannot
meet a condition fails here; tests/test_gpu_fused_instances.py skips nothing."""
import os
import re
import subprocess

import pytest

from fused_instances import (BATCHES, FAMILY_SIZES, FORMS, INSTANCES, batches_of, check_plan, host_script, instance_id, job_targets,
                             pairs_per_workgroup, parse_plan, route, shape_walk, shortfalls, split_cases, teams, walk_samples)
from settings_schedule import DETRENDS, segments_after

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
CSRC = os.path.join(ROOT, "stabilizer-stream_amd", "csrc")
_EXE = {}


@pytest.fixture(scope="module")
def fwc_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("fused_walk_check")


def fwc_exe(tmp_dir, key):
    """tests/host/fused_walk_check.cpp with the library's host runtime and the CPU model, plain or under the sanitizers"""
    if key not in _EXE:
        exe = os.path.join(str(tmp_dir), "fused_walk_check_" + key)
        flags = {"plain": ["-O2"], "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]}[key]
        src = ["fused_walk_check.cpp", "sim/sim_kernels.cpp"] + [os.path.join(CSRC, f + ".cpp") for f in ("runtime", "planner", "frames_ingest", "readout")]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas"] + flags +
                       ["-Isim", "-I" + CSRC] + src + ["-o", exe, "-lpthread"], cwd=HOST, check=True, timeout=600)
        _EXE[key] = exe
    return _EXE[key]


def run_walks(exe, insts):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], input=host_script(insts), capture_output=True, text=True, timeout=800, env=env)
    assert r.returncode == 0 and "every segment and every decimator output exactly once" in r.stdout, (r.stdout + r.stderr)[-3000:]
    return split_cases(r.stderr)


def test_instances_are_what_the_launch_switches_compile(fwc_dir):
    """families, sizes and teams from the launch switch's family function and the geometry headers; the variants from the template
    arguments the three launch switches spell out"""
    r = subprocess.run([fwc_exe(fwc_dir, "plain"), "--instances"], capture_output=True, text=True, timeout=60, check=True)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [tuple(w) for w in lines[:-1]] == [(fam, str(n), "teams", str(teams(n))) for fam, n in FAMILY_SIZES], r.stdout
    assert tuple(lines[-1][1:]) == FORMS
    assert [teams(n) for n in (256, 512, 1024)] == [32, 16, 8] and all(teams(n) == 1 for _, n in FAMILY_SIZES[3:])
    # the switches: each names <N, D, EWMA, FRAMES, SINGLE> for D = 0 ... 3 over {plain, EWMA} x {pair, frames, single 1, single 2}
    variants = {(False, False, 0): "pair", (False, True, 0): "frames", (False, False, 1): "single1", (False, False, 2): "single2"}
    for path, kernel in (("fused.hip", "fused_kernel"), ("bigfused3_impl.h", "bigfused3_kernel"), ("bigfused_impl.h", "bigfused_kernel")):
        text = open(os.path.join(CSRC, path)).read()
        got = set()
        for m in re.finditer(r"\(" + kernel + r"<N, D((?:, \w+)*)>\)", text):
            a = [w for w in m.group(1).split(", ") if w]
            a += ["false"] * (2 - len(a))
            ew, fr, single = a[0] == "true", a[1] == "true", int(a[2]) if len(a) > 2 else 0
            got.add((ew, variants[(False, fr, single)]))
        assert got == {(e, f) for e in (False, True) for f in FORMS}, (path, sorted(got))
        cases = set(re.findall(r"PSDK_\w+_(?:CASE|SINGLE)\((\d)\)", text))
        assert cases == {"0", "1", "2", "3"}, (path, cases)
    assert set(INSTANCES) == {(fam, n, d, e, f) for fam, n in FAMILY_SIZES for d in DETRENDS for e in (False, True) for f in FORMS}
    assert len(INSTANCES) == 288


def test_single_2_comment_agrees_with_the_code():
    """csrc/kernels.h said SINGLE = 2 is for N <= 1024; fused_double_supported (fused.hip) is every fused size, and so say both now"""
    text = open(os.path.join(CSRC, "kernels.h")).read()
    assert "2 (N <= 1024)" not in text and "2 (every fused size: fused_double_supported)" in text
    fused = open(os.path.join(CSRC, "fused.hip")).read()
    assert "bool fused_double_supported(int n) { return fused_supported(n); }" in fused


def test_settings_spread():
    """every (family, N) sees all four detrends under each of the eight variants, all three batch counts in its frames cases, and
    the two environment routes are set exactly where they are needed"""
    for fam, n in FAMILY_SIZES:
        mine = [i for i in INSTANCES if i[:2] == (fam, n)]
        for e in (False, True):
            for form in FORMS:
                assert {i[2] for i in mine if i[3:] == (e, form)} == set(DETRENDS), (fam, n, e, form)
        assert {batches_of(i) for i in mine if i[4] == "frames"} == set(BATCHES), (fam, n)
    for inst in INSTANCES:
        env = route(inst)["env"]
        assert ("PSDC_FFT3" in env) == (inst[0] == "bigfused" and inst[1] in (2048, 4096)) and env.get("PSDC_FFT3", "0") == "0"
        assert ("PSDC_NO_DOUBLE" in env) == (inst[4] == "single1")
        assert env["PSDC_DBG_FIXED_RUN"] == "2" and "PSDC_DBG_VARIANT" not in env
    assert len({(i[0], i[1], i[4], batches_of(i)) for i in INSTANCES if i[4] == "frames"}) == 27


def test_walks_are_what_they_say():
    """from the walk alone: n - 1 samples first, the job targets, one misaligned call (f32) or one continuing call (frames), spans
    held into one round, stage 2 reaches a segment, and the length stays near 80 n where n is large"""
    for fam, n in FAMILY_SIZES:
        for form in FORMS:
            for b in (BATCHES if form == "frames" else (None,)):
                ops = shape_walk(n, form, b)
                what = (n, form, b)
                q = 8 * b if b else 1
                assert ops[0][1] * q <= n - 1 < (ops[0][1] + 1) * q and ops[1] == ("check",), what
                calls = [op for op in ops if op[0] != "check"]
                assert sum(bool(op[2]) for op in calls) == 1, what
                held = [i for i, op in enumerate(ops[:-1]) if op[0] != "check" and ops[i + 1][0] != "check"]
                assert len(held) >= 2 and ops[-1] == ("check",), what
                total = walk_samples(ops, b)
                mode = {"single1": 1, "single2": 2}.get(form, 0)
                segs = segments_after(n, 0 if mode else n // 2, total)
                assert len(segs) >= 3 and segs[2] >= 1, (what, segs)
                p = pairs_per_workgroup(n)
                floor = sum(job_targets(n, mode)) + (17 * p if b else 0)  # (the targets, and the groups of 8 and 8 k + r workgroups)
                assert total <= max(80, 2 * floor + 40) * n, (what, total / n)
    assert shortfalls(1024, 0) == [0, 1, 15] and shortfalls(1024, 2) == [0, 2, 14] and shortfalls(2048, 0) == [0, 1] and shortfalls(8192, 2) == [0]


def test_every_walk_meets_its_conditions_on_the_cpu_model(fwc_dir):
    """all 288 walks through csrc/planner.cpp with PSDC_DBG_PLAN and PSDC_DBG_FIXED_RUN=2: the model finds every read inside its
    source and every segment and decimator output produced once, and the plan lines show each case's instance and shapes"""
    cases = run_walks(fwc_exe(fwc_dir, "plain"), INSTANCES)
    for inst in INSTANCES:
        check_plan(inst, parse_plan(cases[instance_id(inst)]))


def test_walks_under_sanitizers(fwc_dir):
    """the same program built with -fsanitize=address,undefined, as a stand-alone executable: a quarter of the cases, every
    (family, N, averaging, form) with its detrend rotating"""
    sel = [inst for i, inst in enumerate(INSTANCES) if DETRENDS.index(inst[2]) == (i // 4 + i // 32) % 4]
    assert len(sel) == 72 and {i[:2] + i[3:] for i in sel} == {i[:2] + i[3:] for i in INSTANCES}
    cases = run_walks(fwc_exe(fwc_dir, "san"), sel)
    for inst in sel:
        check_plan(inst, parse_plan(cases[instance_id(inst)]))


def test_a_wrong_walk_is_reported():
    """check_plan is not vacuous: plan lines of another instance, and a case without its edge shapes, fail"""
    line = ("fused launch: 2 jobs, 4 workgroups (+0 aux), 40 pairs: 8p/1wg/r2s@0.1 32p/2wg/r2@0.9 | kernel fused n=1024 detrend=3 ewma=0 "
            "frames=0 single=0 groups=[]")
    la = parse_plan(line)
    assert la[0]["jobs"][0] == {"pairs": 8, "wg": 1, "run": 2, "seam": True, "stage": 0, "step0": 1, "framed": False} and la[0]["groups"] == []
    with pytest.raises(AssertionError, match="no job of one unit"):
        check_plan(("fused", 1024, "mean", False, "pair"), la)
    with pytest.raises(AssertionError):
        check_plan(("fused", 1024, "none", False, "pair"), la)
    with pytest.raises(AssertionError):
        check_plan(("bigfused", 2048, "mean", False, "pair"), parse_plan(line.replace("n=1024", "n=2048").replace("fused n", "bigfused3 n")))
