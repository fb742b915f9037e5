"""tests/segment_instances.py held to the library and to the kernels' headers, without a GPU: INSTANCES is exactly what the library
supports, TILE and the shape tables are what csrc/cross_channel.h and csrc/csm_fft.h compute (printed by tests/host/
segment_kernel_check.cpp --shapes), and every instance's walk meets the conditions that make it worth running.  A walk that
cannot meet one fails here; tests/test_gpu_segment_instances.py skips nothing."""
import subprocess

from segment_instances import (CSM_SHAPE, INSTANCES, KERNELS, PAIR_KINDS, SIZES, TEAM_SHAPE, TILE, instance_id, overlap_of, settings_of,
                               shape_walk)
from settings_schedule import DETRENDS, segments_after
from test_segment_kernel_host import segk_dir, segk_exe  # noqa: F401


def constructor_takes(pkg, cls, n):
    """cross and zoom have no *_supported call: the constructor is asked.  It checks its arguments before it looks for a device
    (create_impl of csrc/cross_runtime.cpp), so a size it refuses is ERR_ARG with or without a GPU, and a size it takes is an
    object, or ERR_DEVICE where there is no GPU."""
    try:
        getattr(pkg, cls)(n, 1).close()
    except pkg.PsdError as e:
        if e.code == pkg.ERR_ARG:
            assert "n must be a power of two" in str(e), e
            return False
        assert e.code == pkg.ERR_DEVICE, e
    return True


def test_instances_are_the_supported_set(pkg):
    """over n = 1 ... 8192 (csm: m = 1 ... 5 too) the library takes exactly the sizes INSTANCES lists for the kind"""
    asked = {
        "cross": lambda n: constructor_takes(pkg, "CsdCascadeBank", n), "zoom": lambda n: constructor_takes(pkg, "ZoomCascadeBank", n),
        "sk": pkg.sk_supported, "zsk": pkg.zoom_sk_supported, "zampm": pkg.zoom_ampm_supported, "zcsd": pkg.zcsd_supported,
        "zxampm": pkg.zoom_ampm_cross_supported,
    }
    assert set(asked) | {"csm"} == set(KERNELS)
    for kind, fn in asked.items():
        took = [n for n in range(1, 8193) if fn(n)]
        assert took == [n for k, n, _ in INSTANCES if k == kind] == list(SIZES), (kind, took)
    took = {(n, m) for n in range(1, 8193) for m in range(1, 6) if pkg.csm_supported(n, m)}
    assert took == {(n, m) for k, n, m in INSTANCES if k == "csm"} == set(CSM_SHAPE), sorted(took)
    assert len(INSTANCES) == len(set(INSTANCES)) == 69


def test_tile_equals_the_headers(segk_dir):  # noqa: F811
    """seg_teams, seg_block and CsmShape<N, M>::{BLOCK, TEAMS, SPT, PG, GS} as g++ computes them from csrc"""
    r = subprocess.run([segk_exe(segk_dir, "plain"), "--shapes"], capture_output=True, text=True, timeout=60, check=True)
    team, csm = {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "team":
            assert w[2::2] == ["teams", "block"], line
            team[int(w[1])] = (int(w[5]), int(w[3]))
        else:
            assert w[0] == "csm" and w[3::2] == ["block", "teams", "spt", "pg", "gs"], line
            csm[int(w[1]), int(w[2])] = tuple(int(v) for v in w[4::2])
    assert team == TEAM_SHAPE and csm == CSM_SHAPE
    for inst in INSTANCES:
        kind, n, m = inst
        if kind == "csm":
            assert TILE[inst] == csm[n, m][2] == 2 * csm[n, m][1]
        else:
            assert TILE[inst] == (2 if kind in PAIR_KINDS else 1) * team[n][1], inst


def test_settings_spread():
    """no kernel sees one combination only: every detrend and both averagings at every kernel, one rectangular and one caller's
    window each, and a caller's window never under an anchored detrend"""
    for kind in KERNELS:
        got = [settings_of(i) for i in INSTANCES if i[0] == kind]
        assert {g[0] for g in got} == set(DETRENDS) and len({g[1] for g in got}) == 2, kind
        assert len({g[:2] for g in got}) >= 6, kind
        assert sorted(g[2] for g in got if g[2] != "hann") == ["custom", "rect"], kind
        assert all(g[0] in ("none", "mean") for g in got if g[2] == "custom")


def test_walk_conditions():
    """every instance's walk, from segments_after alone"""
    for inst in INSTANCES:
        kind, n, m = inst
        spt = TILE[inst]
        overlap = overlap_of(n, settings_of(inst)[2])
        calls = shape_walk(n, overlap, spt)
        what = (instance_id(inst), calls)
        assert calls[0] == n - 1 and sum(calls) <= (1 << 19) + (1 << 15), what
        taken, before, new = 0, [], []
        for c in calls:
            taken += c
            after = segments_after(n, overlap, taken)
            new.append([a - (before[k] if k < len(before) else 0) for k, a in enumerate(after)])
            before = after
        new0 = {s[0] for s in new}
        assert {0, 1, spt, spt + 1} <= new0, what
        assert spt - 1 < 1 or spt - 1 in new0, what
        assert any(c % 2 and c > 2 * spt for c in new0), what
        assert len(before) >= 3 and before[2] >= 3, what
        if spt > 2:
            assert any(0 < c < spt for s in new for c in s[1:]), what
    hann = {n: sum(shape_walk(n, n // 2, 2)) for n in (64, 4096)}
    assert hann == {64: 10787, 4096: 542723}, hann
    assert segments_after(64, 32, hann[64]) == [336, 40, 3] and segments_after(4096, 2048, hann[4096])[:3] == [264, 32, 3]
