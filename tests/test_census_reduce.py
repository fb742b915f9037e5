"""tools/stamps/census.py reduce_census on a synthetic launch whose figures can be worked out by hand: one CU, two SIMDs of four
compute wavefronts, one aux wavefront, a record left over from a launch of another grid and an empty record."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("psd_census", os.path.join(ROOT, "tools", "stamps", "census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(entry, first, exit_, slot, simd, wg, wave, kind=1, job=0, run=10, nrun=10, npairs=80, grid=2, xcd=3, se=2, cu=5):
    hw = slot | simd << 4 | cu << 8 | se << 13
    u = lambda v: v & 0xFFFFFFFF
    return [entry, first, exit_, xcd << 32 | hw, wave << 32 | wg, kind << 32 | u(job), u(nrun) << 32 | u(run), grid << 32 | u(npairs)]


@pytest.fixture(scope="module")
def launch():
    rows = [record(1000, 1000, 1100, 4, 0, 0, 0, kind=2, job=-1, run=0, nrun=0, npairs=0)]  # the aux wavefront: the first entry
    for i, ex in enumerate([2000, 1900, 1800, 1700]):  # SIMD 0: four full runs that leave one after the other
        rows.append(record(1000, 1010, ex, i, 0, 1, i))
    for i, (ex, nrun) in enumerate([(1900, 10), (1900, 10), (1900, 10), (1500, 5)]):  # SIMD 1: later, together, one half run
        rows.append(record(1100, 1110, ex, i, 1, 1, 4 + i, nrun=nrun))
    rows.append(record(10, 10, 5000, 0, 0, 7, 0, grid=99))  # a launch of another grid
    rows.append([0] * 8)                                     # an empty record
    return np.array(rows, dtype=np.uint64)


def test_residency_and_the_split_of_the_loss(census, launch):
    r = census.reduce_census(launch)
    assert (r["grid"], r["compute_waves"], r["aux_waves"]) == (2, 8, 1)
    assert r["span_us"] == pytest.approx(10.0)  # 1000 ticks of 10 ns
    assert r["residency"] == pytest.approx(6200 / 8000)
    mean_full = (3400 + 2400) / 7
    quant = 0.5 * mean_full
    lo = r["loss"]
    assert lo["total"] == pytest.approx(0.225)
    assert lo["ramp"] == pytest.approx(400 / 8000)
    assert lo["quantisation"] == pytest.approx(quant / 8000)
    assert lo["within_simd"] == pytest.approx((600 + 500 - quant) / 8000)
    assert lo["empty_simd"] == pytest.approx(300 / 8000)
    assert lo["quantisation"] + lo["within_simd"] + lo["empty_simd"] + lo["ramp"] == pytest.approx(lo["total"])
    assert r["quantisation_by_construction"] == pytest.approx(1 - 75 / 80)
    assert r["runs"] == {"5": 1, "10": 7}


def test_exit_distributions(census, launch):
    r = census.reduce_census(launch)
    assert r["slots_seen"] == [0, 1, 2, 3]
    assert r["simd_exit_spread"]["mean"] == pytest.approx(0.15)  # 0.3 in SIMD 0, 0 among the full runs of SIMD 1
    assert r["simd_exit_spread"]["max"] == pytest.approx(0.3)
    e = r["exit_frac"]
    assert e["by_slot"]["0"]["mean"] == pytest.approx((1.0 + 0.9) / 2)
    assert e["by_slot"]["3"]["mean"] == pytest.approx((0.7 + 0.5) / 2)
    assert e["by_wave_half"]["0"]["mean"] == pytest.approx(0.85) and e["by_wave_half"]["1"]["mean"] == pytest.approx(0.8)
    assert e["by_nrun"]["5"]["mean"] == pytest.approx(0.5)
    assert list(e["by_xcd"]) == ["3"] and list(e["by_se"]) == ["2"] and list(e["by_stage"]) == ["0"]
    assert r["start_ramp_us"]["max"] == pytest.approx(1.0)
    assert r["warmup_us"]["p50"] == pytest.approx(0.1)


def test_stages_are_ranked_by_job_length(census):
    rows = [record(0, 0, 100, i, 0, 0, i, job=0, npairs=65536) for i in range(4)]
    rows += [record(0, 0, 90, i, 1, 1, i, job=1, npairs=8192) for i in range(4)]
    rows += [record(0, 0, 80, i, 2, 2, i, job=2, npairs=1024) for i in range(4)]
    r = census.reduce_census(np.array(rows, dtype=np.uint64))
    s = r["exit_frac"]["by_stage"]
    assert [s[k]["mean"] for k in ("0", "1", "2")] == pytest.approx([1.0, 0.9, 0.8])
    assert r["exit_frac"]["by_placement"]["0"]["n"] == 4  # three workgroups on the one CU, in the order they came
    assert r["residency"] == pytest.approx(0.9)


def test_no_compute_record_is_an_error(census):
    with pytest.raises(ValueError):
        census.reduce_census(np.zeros((4, 8), dtype=np.uint64))
