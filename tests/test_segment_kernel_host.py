"""The skeleton of the eight segment kernels (csrc/segment_kernel.h) on the CPU: tile addressing and the two team-combine forms,
walked by tests/host/segment_kernel_check.cpp for every (workgroup, tile, team) and every thread of a workgroup.  This file compiles
the program itself, as tests/test_sk_host.py compiles its emulation: plainly, under the address and undefined-behaviour sanitizers
(a stand-alone program; nothing is loaded into Python), and once with each of the two mistakes the program can seed into its own
calls, which it must report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stabilizer-stream_amd", "csrc")

_EXE = {}


@pytest.fixture(scope="session")
def segk_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("segment_kernel_check")


def segk_exe(tmp_dir, key):
    if key not in _EXE:
        exe = os.path.join(str(tmp_dir), "segment_kernel_check_" + key)
        flags = {"plain": ["-O2"], "san": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                 "seed1": ["-O2", "-DSEGK_SEED=1"], "seed2": ["-O2", "-DSEGK_SEED=2"]}[key]
        subprocess.run(["g++", *flags, "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "host", "segment_kernel_check.cpp"),
                        "-o", exe], check=True)
        _EXE[key] = exe
    return _EXE[key]


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    return r


def passes(r):
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-3000:]
    assert "FAIL" not in r.stdout
    # both tile forms at the seven sizes and csm's tiles at its 20 shapes: lanes with and without a segment were walked
    lanes, idle = [int(v) for v in r.stdout.split("addressing: ")[1].split(" without")[0].replace(" lanes walked,", "").split()]
    assert lanes > 20000 and 0 < idle < lanes
    assert "7 team kernels at 7 sizes, N = 64 ... 4096, and csm at 20 shapes (N, M), 9 of them with product groups" in r.stdout


def test_segment_skeleton(segk_dir):
    """every segment of a job exactly once at its offset and EWMA step, idle lanes inside the job's first segment; every partial
    element of every kernel's combine written once, summed over the groups in ascending order, inside the kernel's LDS"""
    passes(run(segk_exe(segk_dir, "plain")))


def test_segment_skeleton_under_sanitizers(segk_dir):
    """the same program built with -fsanitize=address,undefined: the LDS image, the accumulators and the partial have their exact sizes"""
    passes(run(segk_exe(segk_dir, "san")))


def test_seeded_idle_lane_offset_is_reported(segk_dir):
    """SEGK_SEED=1: a lane without a segment takes its offset from the previous job's base.  Only the addressing walk complains."""
    r = run(segk_exe(segk_dir, "seed1"))
    assert r.returncode != 0 and "failure(s)" in r.stdout
    fails = [line for line in r.stdout.splitlines() if line.startswith("FAIL")]
    assert fails and all("a lane without a segment reads at" in line for line in fails), fails[:5]
    assert any(line.startswith("FAIL seg_pair") for line in fails)


def test_seeded_dropped_turn_offset_is_reported(segk_dir):
    """SEGK_SEED=2: the sum phase loses its turn offset.  The kernels of more than one turn (zoom_ampm first) write the rows of
    turn 0 again and again; the addressing walk stays clean."""
    r = run(segk_exe(segk_dir, "seed2"))
    assert r.returncode != 0 and "failure(s)" in r.stdout
    fails = [line for line in r.stdout.splitlines() if line.startswith("FAIL")]
    assert fails and fails[0].startswith("FAIL zoom_ampm N=64: partial [0][0] written 2 times"), fails[:5]
    assert not any("lane" in line or "segment" in line for line in fails)
