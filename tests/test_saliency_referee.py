"""The referee of the input gradient (tests/saliency_referee.py) on the CPU: the float32 PyTorch chain meets the acceptance rule
against the float64 chain on exactly the seeds and shapes the GPU tests use, so the 2 % cap on windows with a turned mask is left
to the reference alone; and the referee's own pieces are what they say (no GPU needed)."""
import numpy as np
import pytest

import saliency_referee as sr


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: "{}x{}".format(c[2], c[3]))
def test_float32_cpu_chain_meets_the_rule_on_the_gpu_tests_inputs(case):
    ref = sr.referee(*case)
    assert ref.G64.shape == ref.x.shape and ref.margin.shape == (case[4],) and np.all(ref.margin >= 0)
    assert np.abs(ref.G64).reshape(case[4], -1).max(axis=1).min() > 0      # every window has a gradient to compare against
    sr.accept(ref.G32, ref, "float32 CPU chain {}".format(case))


def test_gradient_matches_a_finite_difference():
    """dP/dx of the float64 chain against a central difference along a random direction (h small enough to turn no mask)"""
    import torch
    seed, xseed, rows, channels, _ = sr.CASES[0]
    ref = sr.referee(seed, xseed, rows, channels, 4)
    d = np.random.default_rng(1).standard_normal(ref.x.shape)
    h = 1e-7
    xp, xm = ref.x.astype(np.float64) + h * d, ref.x.astype(np.float64) - h * d
    pp = sr.chain(ref.model, xp, torch.float64)[1][:, 1]
    pm = sr.chain(ref.model, xm, torch.float64)[1][:, 1]
    want = (ref.G64 * d).reshape(4, -1).sum(axis=1)
    np.testing.assert_allclose((pp - pm) / (2 * h), want, rtol=1e-5, atol=1e-12)


def test_acceptance_rule_rejects_what_it_should():
    ref = sr.referee(*sr.CASES[0][:4], 4)
    bad = ref.G64.copy()
    clear = int(np.argmax(ref.margin))
    if ref.margin[clear] > sr.MARGIN:
        bad[clear] *= 1.0 + 1e-4       # a window far from every decision, off by 20 tolerances
        with pytest.raises(AssertionError):
            sr.accept(bad, ref)
    with pytest.raises(AssertionError):
        sr.accept(ref.G64 * (1.0 + 1e-4), ref)      # every window off: beyond the cap whatever the margins
    sr.accept(ref.G64.astype(np.float32), ref)
