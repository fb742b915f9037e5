"""The N = 1024 team FFT's second exchange as re / im planes (add-tid stores, 16-byte reads): no GPU needed.

tests/host/fft_planes_check.cpp runs csrc/fft_team.h's store1_planes / load2_planes addressing lane by lane under the gfx950
LDS banking rules and compares the transform with the cf-frame path (store1 / load2) bit for bit.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planes_exchange(tmp_path):
    exe = str(tmp_path / "fft_planes_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "stabilizer-stream_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "fft_planes_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
    # zero bank conflicts on the eight 16-byte reads (4 lane groups each), the exchange inside the 2176-dword frame
    m = re.search(r"extent (\d+) of (\d+) dwords; 8 ds_read_b128: (\d+) LDS cycles \(ideal (\d+)\)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) <= int(m.group(2)) == 2176
    assert int(m.group(3)) == int(m.group(4)) == 32
    assert len(re.findall(r"planes bit-identical to the cf frame", r.stdout)) == 8, r.stdout


def test_device_listing_has_the_planes_offsets(tmp_path):
    """The device branches are code of their own (byte offsets spliced into inline assembly): compile fused.hip for gfx950
    (device side only, no GPU needed) and hold the headline kernel's add-tid stores to the layout, stated here independently
    of csrc/fft_team.h: rows in order of their bank quad a, row k at dword 64 k + 4 a, the im plane 1088 dwords on; plus the
    eight stage-A outputs.  M0 may appear only where a block saves, sets and restores it."""
    csrc = os.path.join(ROOT, "stabilizer-stream_amd", "csrc")
    asm = str(tmp_path / "fused.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-fPIC", "-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-Xclang", "-target-feature",
                    "-Xclang", "-packed-fp32-ops", "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, "fused.hip"),
                    "-o", asm], check=True, stderr=subprocess.DEVNULL, timeout=800)
    s = open(asm).read()
    m = re.search(r"^_ZN4psdk12fused_kernelILi1024ELi0ELb0ELb0ELi0EE\w*:.*?s_endpgm", s, re.M | re.S)
    assert m, "headline kernel not in the listing"
    body = m.group(0)
    q1, q2, xs = [0, 1, 2, 3, 12, 13, 14, 15], list(range(4, 12)), [0, 1, 2, 3, 8, 9, 10, 11]
    row = {}
    for j in range(8):
        row[q1[j]] = 64 * (2 * j) + 4 * xs[j]
        row[q2[j]] = 64 * (2 * j + 1) + 4 * xs[j]
    n = 1024
    xo = 6 + n // 2
    ae = xo + 6 + n // 2
    ao = ae + 12 + n // 4  # (csrc/fused_common.h FusedDec)
    want = {4 * (p * 1088 + row[q]) for p in (0, 1) for q in range(16)}
    want |= {4 * (a + 11 + 64 * r) for a in (ae, ao) for r in range(4)}
    got = [int(o, 0) for o in re.findall(r"ds_write_addtid_b32 v\d+ offset:(0x[0-9a-fA-F]+|\d+)", body)]
    got += [0] * len(re.findall(r"ds_write_addtid_b32 v\d+\s*$", body, re.M))  # (a zero offset may be left out)
    assert len(re.findall(r"ds_write_addtid_b32", body)) == len(got), "an add-tid store in another form"
    assert set(got) == want and len(want) == 40
    assert len(got) % 40 == 0  # every pair body issues each of them once
    assert max(got) <= 0xFFFF
    for line in s.splitlines():
        if re.search(r"\bm0\b", line) and not line.lstrip().startswith(";"):
            assert re.fullmatch(r"\s*s_mov_b32 (m0, s\d+|s\d+, m0)\s*", line), line
    # the 16-byte reads of the exchange: one base register, immediates 256 B apart, the im plane 4352 B on
    assert len(re.findall(r"ds_read_b128 v\[\d+:\d+\], v\d+ offset:4352\b", body)) >= 1
