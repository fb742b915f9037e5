"""The N = 1024 f32 team kernels choose the FFT-phase priority of a wavefront from a progress table in device memory
(csrc/fused.hip, PSDK_FAIR_FB): every K = 4 pairs, in the first half of the two-pair loop, a wavefront stores the pairs left in its
run into its SIMD's row, reads the row with one scalar load and takes level 2, 1 or 0 by how many of the other three have more
left (none: 2, all three: 0).  It stores its run's length at the start and 0 when it leaves.  The table is a hint: whatever it holds, the same bits come out.  Runs around the publish period against the CPU oracle
(runs that never reach a periodic step, that end on one and just past one, and a last workgroup whose wavefronts leave early),
the Mean + EWMA instantiation of the loop, spans of one and two pairs, and equal bits with and without a foreign handle's
wavefronts writing the same rows, with the compared handles made in either order."""
import numpy as np
import pytest

from conftest import test_signal as make_signal
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

N = 1024
K = 4  # PSDK_FAIR_FB_K of the shipped build


def span_len(pairs, n=N):
    """samples that hold `pairs` segment pairs at half overlap: pair p = samples N p ... N p + 3N/2"""
    return pairs * n + n // 2


CUTS = np.cumsum([0, span_len(8 * (2 * K + 1) + 3), span_len(19), span_len(7)])  # (the first span also serves the 43-pair cases)


@pytest.fixture(scope="module")
def noise(pkg):
    """one seeded stream shared (read-only) by the cases: noise, a weak tone, a small offset"""
    x = make_signal(pkg, int(CUTS[-1]), seed=0xFEEDB, tone=0.2, dc=0.05)
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


@pytest.mark.parametrize("run", [1, K - 1, K, K + 1, 2 * K + 1])
def test_runs_around_the_publish_period(pkg, ora, gpu_required, monkeypatch, noise, run):
    """8 x run + 3 pairs in runs of `run`: eight wavefronts with a full run -- shorter than the period (only the step of the
    first pair), exactly one period, one pair past it, two periods and a pair --, then a workgroup whose wavefronts hold a short
    run or none and leave, publishing 0, while the others of their SIMD go on."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", str(run))  # (read when the handle is made)
    pairs = 8 * run + 3
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs} pairs in runs of {run}")


def test_mean_ewma_instantiation(pkg, ora, gpu_required, monkeypatch, noise):
    """The Mean + EWMA kernel shares the loop: 43 pairs in runs of 5."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", "5")
    feed_one_span(pkg, ora, noise[:span_len(43)], detrend="mean", avg=(3, 1000), what="43 pairs in runs of 5, mean, avg (3, 1000)")


@pytest.mark.parametrize("pairs", [1, 2])
def test_spans_of_one_and_two_pairs(pkg, ora, gpu_required, noise, pairs):
    """A fresh handle, one span of 1 or 2 pairs: seven or six wavefronts of the one workgroup publish nothing but zeros."""
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs}-pair span")


@pytest.mark.parametrize("quiet_first", [True, False], ids=["quiet-made-first", "contended-made-first"])
def test_the_table_cannot_change_bits(pkg, gpu_required, noise, quiet_first):
    """Two handles are fed the same three spans (43, 19 and 7 pairs), one on a quiet device, the other while a third handle's
    2^22-sample stream runs on a stream of its own: its wavefronts share the SIMDs and write their progress into the same rows.
    Stage spectra, counts and pending samples bit for bit; the two handles made in either order."""
    import torch
    spans = [torch.from_numpy(np.array(noise[a:a + span_len(p)])).cuda() for a, p in zip(CUTS[:-1], (43, 19, 7))]
    other = torch.empty(1 << 22, dtype=torch.float32, device="cuda")
    pkg.fill_noise_device(other.data_ptr(), other.numel(), seed=0xB052)
    torch.cuda.synchronize()
    if quiet_first:
        quiet, contended = pkg.PsdCascadeBank(N), pkg.PsdCascadeBank(N)
    else:
        contended, quiet = pkg.PsdCascadeBank(N), pkg.PsdCascadeBank(N)
    busy = pkg.PsdCascadeBank(N)
    for s in spans:
        quiet.process_device(0, s.data_ptr(), s.numel())
    quiet.sync()
    for s in spans:  # (nothing orders these calls against the busy handle's)
        for _ in range(4):
            busy.process_device(0, other.data_ptr(), other.numel())
        contended.process_device(0, s.data_ptr(), s.numel())
    contended.sync()
    busy.sync()
    assert quiet.num_stages(0) == contended.num_stages(0) >= 2
    for k in range(quiet.num_stages(0)):
        assert quiet.stage_info(0, k) == contended.stage_info(0, k), f"stage {k}"
        assert np.array_equal(quiet.stage_spectrum(0, k).view(np.uint32), contended.stage_spectrum(0, k).view(np.uint32)), f"stage {k}"
        assert np.array_equal(quiet.stage_buf(0, k).view(np.uint32), contended.stage_buf(0, k).view(np.uint32)), f"stage {k} pending"
    assert quiet.stage_info(0, 0)["count"] >= 2 * (43 + 19 + 7) - 2
    assert np.all(quiet.stage_spectrum(0, 0) > 0)
    assert busy.stage_info(0, 0)["count"] > 0
    for h in (quiet, contended, busy):
        h.close()
