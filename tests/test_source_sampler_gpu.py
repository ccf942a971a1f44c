"""Posterior sampling on models whose dynamics are given as source (the RTS_EXT_USER route of csrc/ffbs_sampler.hpp):
parity with the float64 oracle of tests/test_sampler_cpu.py under the analytic Jacobian, the zero-noise identity with the
smoother, key mode, the samples-per-lane counts and chunking, on the register and the run-time-dimension kernels."""
import numpy as np
import pytest

from tests import common as cm
from tests import source_smoother_cases as sc
from tests.test_sampler_gpu import _np, _dev, _oracle, _check, _noise, SPLS

pytestmark = pytest.mark.gpu

F32 = np.float32
GENERIC = {"force_generic": 1}


# 8 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_inputs", [False, True])
def test_sampler_parity(with_inputs):
    import torch
    import bayesianfiltering_amd as bfa
    c = sc.case("lorenz63", 5, 16, with_inputs)
    S = 3
    xi = _noise((c.B, S, c.T, c.n), 909)
    ref = _oracle(c.post, None, xi, inputs_F=c.jac)
    tag = "source_lorenz63" + ("_u" if with_inputs else "")
    _check(bfa.posterior_sample(c.p, c.post, S, noise=_dev(xi), inputs=c.u), ref, c.post, tag)
    _check(bfa.posterior_sample(c.p, c.post, S, noise=_dev(xi), inputs=c.u, options=GENERIC), ref, c.post, tag + "_generic")
    # zero noise: the smoothed means of the same route
    z = torch.zeros((c.B, S, c.T, c.n), device="cuda")
    for opt in (None, GENERIC):
        x0 = bfa.posterior_sample(c.p, c.post, S, noise=z, inputs=c.u, options=opt)
        sm = bfa.rts_smoother(c.p, c.post, inputs=c.u, options=opt).smoothed_means
        for s in range(S):
            assert cm.rel_err(_np(x0[:, s]), _np(sm[:, 0])) <= 1e-6, (opt, s)
    key = bfa.PRNGKey(5)
    es = bfa.extended_kalman_posterior_sample(c.p, c.ys, S, key, inputs=c.u)
    assert np.array_equal(_np(es), _np(bfa.posterior_sample(c.p, c.post, S, key=key, inputs=c.u)))


def test_sampler_above_the_register_limit():
    import bayesianfiltering_amd as bfa
    c = sc.case("lorenz96", 3, 12)    # n = 10
    S = 3
    xi = _noise((c.B, S, c.T, c.n), 910)
    _check(bfa.posterior_sample(c.p, c.post, S, noise=_dev(xi)), _oracle(c.post, None, xi, inputs_F=c.jac), c.post,
           "source_lorenz96_n10")


def test_samples_per_lane_counts_agree():
    import bayesianfiltering_amd as bfa
    c = sc.case("lorenz63", 5, 16)
    S = 8
    xi = _dev(_noise((c.B, S, c.T, c.n), 911))
    ref = _np(bfa.posterior_sample(c.p, c.post, S, noise=xi))
    for spl in SPLS:
        assert np.array_equal(_np(bfa.posterior_sample(c.p, c.post, S, noise=xi, options={"ffbs_spl": spl})), ref), spl


# 9 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [0, 1])
def test_chunks_bit_for_bit(generic):
    import bayesianfiltering_amd as bfa
    c = sc.case("lorenz63", 5, 16)
    S, s = 3, 9
    opt = {"force_generic": generic}
    xi = _noise((c.B, S, c.T, c.n), 707)
    full = _np(bfa.posterior_sample(c.p, c.post, S, noise=_dev(xi), options=opt))
    late, carry = bfa.posterior_sample(c.p, sc.cut(c.post, s, c.T), S, noise=_dev(xi[:, :, s:]), return_carry=True, options=opt)
    early = bfa.posterior_sample(c.p, sc.cut(c.post, 0, s), S, noise=_dev(xi[:, :, :s]), carry=carry, options=opt)
    assert np.array_equal(np.concatenate([_np(early), _np(late)], axis=2), full)
    assert np.array_equal(_np(carry.states), _np(late[:, :, 0]))
