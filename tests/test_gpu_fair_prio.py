"""The f32 team kernels run the FFT phase of a pair at a priority that rotates with the pair and the wavefront's rank in its
SIMD (csrc/fused.hip, PSDK_FAIR): the level of pair p for rank r is entry (p + r) mod 4 of 0 1 2 1, chosen by scalar branches in
both halves of the two-pair loop.  Priorities decide who issues first, never what is computed: short runs through every residue
of the rotation against the CPU oracle, the N = 512 kernel (two teams a wavefront, which leave the loop at different pairs;
the switch does not reach N = 256), the Mean + EWMA instantiation of the same loop, equal bits with and without an unrelated stream competing
for the device, and spans so short that most wavefronts of the workgroup have no pair."""
import numpy as np
import pytest

from conftest import test_signal as make_signal
from test_gpu_parity import check_against_oracle

pytestmark = pytest.mark.gpu

N = 1024


def span_len(pairs, n=N):
    """samples that hold `pairs` segment pairs at half overlap: pair p = samples N p ... N p + 3N/2"""
    return pairs * n + n // 2


@pytest.fixture(scope="module")
def noise(pkg):
    """one seeded stream shared (read-only) by the cases: noise, a weak tone, a small offset"""
    x = make_signal(pkg, span_len(43) + span_len(19) + span_len(7), seed=0xFA1B, tone=0.2, dc=0.05)
    x.setflags(write=False)
    return x


def feed_one_span(pkg, ora, x, detrend="none", avg=None, what="", n=N):
    import torch
    x = np.array(x)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()  # the library runs on its own stream
    g = pkg.PsdCascadeBank(n)
    g.set_detrend(pkg.Detrend[detrend.upper()])
    a = pkg.AvgOpts(*avg) if avg else None
    if a:
        g.set_avg(a)
    g.process_device(0, d.data_ptr(), x.size)
    g.sync()
    check_against_oracle(pkg, ora, g, [x], n, detrend=detrend, avg=a, what=what)
    g.close()


@pytest.mark.parametrize("run", [1, 3, 4, 5])
def test_every_rotation_residue(pkg, ora, gpu_required, monkeypatch, noise, run):
    """8 x run + 3 pairs in runs of `run`: eight wavefronts with a full run (pairs at every residue of the period of four, through
    both halves of the loop, odd and even exits), then a workgroup whose wavefronts hold a run of `run` or a shorter one and
    none at all, which leave while the others of their SIMD go on."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", str(run))  # (read when the handle is made)
    pairs = 8 * run + 3
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs} pairs in runs of {run}")


@pytest.mark.parametrize("n", [512])
def test_other_sizes(pkg, ora, gpu_required, monkeypatch, noise, n):
    """N = 512: a workgroup holds 16 teams, two to a wavefront.  One workgroup of full runs of 5 and one with a run of 3: in its
    first wavefront one team works while the other has nothing, so the priority key is read from whichever lane is active."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", "5")
    pairs = (8 * 1024 // n) * 5 + 3
    feed_one_span(pkg, ora, noise[:span_len(pairs, n)], what=f"N={n}: {pairs} pairs in runs of 5", n=n)


def test_mean_ewma_instantiation(pkg, ora, gpu_required, monkeypatch, noise):
    """The Mean + EWMA kernel shares the loop: 43 pairs in runs of 5."""
    monkeypatch.setenv("PSDC_DBG_FIXED_RUN", "5")
    feed_one_span(pkg, ora, noise[:span_len(43)], detrend="mean", avg=(3, 1000), what="43 pairs in runs of 5, mean, avg (3, 1000)")


def test_priorities_cannot_change_bits(pkg, gpu_required, noise):
    """Two handles are fed the same three spans, the second while a third handle's unrelated stream keeps the device busy (its
    wavefronts share the SIMDs, so who wins an issue slot differs between the two): every stage's spectrum, count and pending
    samples bit for bit."""
    import torch
    cuts = [0, span_len(43), span_len(43) + span_len(19), span_len(43) + span_len(19) + span_len(7)]
    # (a tensor each, so that no two calls continue each other in memory and merge into one span)
    spans = [torch.from_numpy(np.array(noise[a:b])).cuda() for a, b in zip(cuts[:-1], cuts[1:])]
    other = torch.empty(1 << 22, dtype=torch.float32, device="cuda")
    pkg.fill_noise_device(other.data_ptr(), other.numel(), seed=0xB051)
    torch.cuda.synchronize()
    quiet, contended, busy = pkg.PsdCascadeBank(N), pkg.PsdCascadeBank(N), pkg.PsdCascadeBank(N)
    for s in spans:
        quiet.process_device(0, s.data_ptr(), s.numel())
    quiet.sync()
    for s in spans:  # (each handle runs on a stream of its own: nothing orders these calls against the busy handle's)
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


@pytest.mark.parametrize("pairs", [1, 2])
def test_spans_of_one_and_two_pairs(pkg, ora, gpu_required, noise, pairs):
    """A fresh handle, one span of 1 or 2 pairs: seven or six wavefronts of the one workgroup have no pair and leave at once."""
    feed_one_span(pkg, ora, noise[:span_len(pairs)], what=f"{pairs}-pair span")
