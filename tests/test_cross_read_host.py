"""The host read-outs of the cross-spectral runtime (csrc/cross_runtime.cpp) on the CPU, byte for byte against the golden dump."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_cross_readouts_on_the_cpu_match_the_golden_dump(tmp_path):
    """tests/host/cross_read_check: csrc/cross_runtime.cpp, unchanged, linked with the host model of the HIP runtime (tests/host/sim/)
    and the launcher models of sim/sim_cross_kernels.cpp, whose fold gives every accumulator a definite f64 value; built with
    -fsanitize=address,undefined.  Two objects of each of the fifteen families at n = 64 (default settings; set_avg / set_detrend
    mid-stream), three units (three stages, one segment, nothing fed), every stage read-out at every stage and one past the last,
    every stitched read-out over keep_overlap x min_count x keep_transition_band and at absent, exact and too small capacities
    of the outputs and of the Breaks.  Return codes, error texts, lengths, Breaks and every output buffer with its guard go to a
    dump, which must equal tests/golden/cross_read_dump.bin: the dump of the same program linked with the runtime as it was before
    its read-outs were unified into one snapshot, one stitch path and one row copier."""
    host = os.path.join(ROOT, "tests", "host")
    subprocess.run(["make", "-C", host, "cross_read_check"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dump = tmp_path / "cross_read_dump.bin"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([os.path.join(host, "cross_read_check"), str(dump)], capture_output=True, text=True, timeout=550, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "every read-out answered" in r.stdout
    got = dump.read_bytes()
    with open(os.path.join(ROOT, "tests", "golden", "cross_read_dump.bin"), "rb") as f:
        want = f.read()
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        record = got.rfind(b"\n== ", 0, at) + 1
        pytest.fail(f"the dump ({len(got)} bytes) differs from the golden ({len(want)} bytes) at byte {at}, in the record "
                    f"{got[record:got.find(10, record)].decode(errors='replace')!r}")
