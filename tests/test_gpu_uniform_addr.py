"""The N = 1024 team kernel carries its run's stream positions, run length and loop counter as wavefront-uniform scalars
(csrc/fused.hip, PSDK_UADDR / PSDK_ULOOP): short runs through both halves of the two-pair loop, different runs side by side in
one workgroup, stream bases more than 4 GiB apart, and the Mean and EWMA instantiations of the same loop -- device-fed through
the C ABI, against the CPU oracle with the comparison helpers of the parity tests.

A wavefront's run is ceil(pairs of the job / (workgroups x 8)) pairs (csrc/planner.cpp), so a span of up to eight pairs gives
every wavefront at most ONE pair, whatever the span's length: the cases with PSDC_DBG_FIXED_RUN = 4 feed spans of 13 ... 32
pairs to a single workgroup, whose wavefronts then hold runs of 4, 3, 2, 1 and 0 pairs next to each other."""
import numpy as np
import pytest

from conftest import test_signal as make_signal
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

N = 1024


def span_len(pairs):
    """samples that hold `pairs` segment pairs at half overlap: pair p = samples N p ... N p + 3N/2"""
    return pairs * N + N // 2


@pytest.fixture(scope="module")
def noise(pkg):
    """one seeded stream shared (read-only) by the cases: noise, a weak tone, a small offset"""
    x = make_signal(pkg, span_len(32) + 3 * span_len(8), seed=0x1024A, tone=0.2, dc=0.05)
    x.setflags(write=False)
    return x


def feed_one_span(pkg, ora, x, detrend="none", avg=None, what=""):
    import torch
    x = np.array(x)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()  # the library runs on its own stream
    g = pkg.PsdCascadeBank(N)
    g.set_detrend(pkg.Detrend[detrend.upper()])
    a = pkg.AvgOpts(*avg) if avg else None
    if a:
        g.set_avg(a)
    g.process_device(0, d.data_ptr(), x.size)
    g.sync()
    check_against_oracle(pkg, ora, g, [x], N, detrend=detrend, avg=a, what=what)
    g.close()


@pytest.mark.parametrize("pairs", [1, 2, 3, 4])
def test_short_spans(pkg, ora, gpu_required, noise, pairs):
    """Spans of 1 ... 4 segment pairs, a handle each: `more` false on a run's first pair, and wavefronts with no pair at all."""
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs}-pair span")


@pytest.mark.parametrize("pairs", [13, 19, 23, 27, 32])
def test_short_runs_both_halves_of_the_loop(pkg, ora, gpu_required, monkeypatch, noise, pairs):
    """One workgroup, runs of ceil(pairs / 8): 13 -> 2 2 2 2 2 2 1 0, 19 -> 3 x 6, 1, 0, 23 -> 3 x 7, 2, 27 -> 4 x 6, 3, 0,
    32 -> 4 x 8: odd and even exits of the unrolled loop, `more` false on the first and on the second pair of a step."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", "4")  # (read when the handle is made)
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs} pairs in one workgroup")


@pytest.mark.parametrize("fixed_run", [None, "4"])
def test_different_runs_in_one_round(pkg, ora, gpu_required, monkeypatch, noise, fixed_run):
    """Three channels fed spans of 5, 6 and 7 pairs in one round (and 21, 22, 23 pairs in runs of 3 and 2 ... 0): the wavefronts
    of a workgroup start at different pairs of their job, the workgroups of a launch read different streams -- a base made
    uniform over more than the wavefront gives wrong spectra here."""
    import torch
    if fixed_run:
        monkeypatch.setenv("PSDC_DBG_FIXED_RUN", fixed_run)
    pairs = [21, 22, 23] if fixed_run else [5, 6, 7]
    off = [0, 777, 4242]  # (different samples a channel)
    xs = [np.array(noise[o:o + span_len(p)]) for o, p in zip(off, pairs)]
    ds = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()
    g = pkg.PsdCascadeBank(N, 3)
    for c in range(3):
        g.process_device(c, ds[c].data_ptr(), xs[c].size)
    g.sync()
    for c in range(3):
        check_against_oracle(pkg, ora, g, [xs[c]], N, channel=c, what=f"channel {c}: {pairs[c]} pairs")
    g.close()


def test_spans_more_than_4_gib_apart(pkg, gpu_required, noise):
    """Two 8-pair spans at the two ends of one allocation of a little over 4 GiB (allocated, not filled), fed as two calls of one
    handle, against copies of the same samples in a small allocation of their own fed to a second handle: bit for bit.  A stream base cut to 32
    bits reads the second span from the first one's neighbourhood."""
    import torch
    m = span_len(8)
    total = (1 << 30) + 2 * m  # floats: 4 GiB + 68 KiB
    a, b = noise[span_len(32):span_len(32) + m], noise[span_len(32) + m:span_len(32) + 2 * m]
    big = torch.empty(total, dtype=torch.float32, device="cuda")
    big[:m] = torch.from_numpy(np.array(a)).cuda()
    big[total - m:] = torch.from_numpy(np.array(b)).cuda()
    # (the copies apart from each other as well: calls that continue each other in memory merge into one span, which is planned,
    # and so rounded, as one job -- the big tensor's two ends never do)
    pool = torch.empty(2 * m + N, dtype=torch.float32, device="cuda")
    da, db = pool[:m], pool[m + N:]
    da.copy_(big[:m])
    db.copy_(big[total - m:])
    torch.cuda.synchronize()
    assert 4 * (total - m) > 1 << 32
    g, h = pkg.PsdCascadeBank(N), pkg.PsdCascadeBank(N)
    g.process_device(0, big.data_ptr(), m)
    g.process_device(0, big.data_ptr() + 4 * (total - m), m)
    h.process_device(0, da.data_ptr(), m)
    h.process_device(0, db.data_ptr(), m)
    g.sync()
    h.sync()
    assert g.num_stages(0) == h.num_stages(0) >= 2
    for k in range(g.num_stages(0)):
        assert g.stage_info(0, k) == h.stage_info(0, k)
        assert np.array_equal(g.stage_spectrum(0, k).view(np.uint32), h.stage_spectrum(0, k).view(np.uint32)), f"stage {k}"
        assert np.array_equal(g.stage_buf(0, k).view(np.uint32), h.stage_buf(0, k).view(np.uint32)), f"stage {k} pending"
    assert g.stage_info(0, 0)["count"] >= 32  # (both spans went through)
    assert np.all(g.stage_spectrum(0, 0) > 0)
    g.close()
    h.close()
    del big


@pytest.mark.parametrize("detrend,avg", [("mean", None), ("none", (3, 1000)), ("mean", (3, 1000))])
@pytest.mark.parametrize("pairs,fixed_run", [(3, None), (19, "4")])
def test_other_instantiations_of_the_loop(pkg, ora, gpu_required, monkeypatch, noise, detrend, avg, pairs, fixed_run):
    """The 3-pair span (and 19 pairs in runs of 3, 1 and 0) through the Mean and the EWMA kernels, which share the loop."""
    if fixed_run:
        monkeypatch.setenv("PSDC_DBG_FIXED_RUN", fixed_run)
    feed_one_span(pkg, ora, noise[:span_len(pairs)], detrend=detrend, avg=avg, what=f"{pairs} pairs, {detrend}, avg {avg}")
