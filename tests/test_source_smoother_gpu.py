"""The extended RTS smoother on models whose dynamics are given as source or as a recorded Python function (the
RTS_EXT_USER route of csrc/rts_smoother.hpp): F_t from forward-mode dual numbers inside kernels built at run time, against
the float64 oracle of tests/test_smoother_cpu.py with the analytic Jacobian, over the GPU's own fp32 streams.  Tolerances
are the registry tests': 1e-5 against the oracle, 1e-6 between two routes of one linear model."""
import ctypes as C

import numpy as np
import pytest

from tests import common as cm
from tests import source_smoother_cases as sc
from tests.test_smoother_gpu import _np, _oracle, _check

pytestmark = pytest.mark.gpu

F32 = np.float32
GENERIC = {"force_generic": 1}


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lorenz63", "growth"])
def test_source_twins_against_the_oracle(kind):
    import bayesianfiltering_amd as bfa
    c = sc.case(kind, 66, 24)     # one wave and a ragged two
    ref = _oracle(c.post, None, c.jac)
    sm = bfa.rts_smoother(c.p, c.post, inputs=c.u, cross_covariances=True)
    _check(sm, ref, name="source_" + kind)
    gen = bfa.rts_smoother(c.p, c.post, inputs=c.u, cross_covariances=True, options=GENERIC)
    _check(gen, ref, name="source_generic_" + kind)
    es = bfa.extended_kalman_smoother(c.p, c.ys, inputs=c.u)
    assert np.array_equal(_np(es.smoothed_means), _np(sm.smoothed_means))
    assert np.array_equal(_np(es.smoothed_covariances), _np(sm.smoothed_covariances))


# 2 -----------------------------------------------------------------------------------------------------------------
def test_above_the_register_limit():
    import bayesianfiltering_amd as bfa
    c = sc.case("lorenz96", 3, 12)    # n = 10: only the run-time-dimension kernel exists
    sm = bfa.rts_smoother(c.p, c.post, cross_covariances=True)
    _check(sm, _oracle(c.post, None, c.jac), name="source_lorenz96_n10")


# 3 -----------------------------------------------------------------------------------------------------------------
def test_recorded_lambda_with_scalar_noise():
    import bayesianfiltering_amd as bfa
    c = sc.pendulum_case()
    assert not isinstance(c.p.dynamics_function, bfa.nonlinearities.DeviceFunction)
    ref = _oracle(c.post, None, c.jac)
    _check(bfa.rts_smoother(c.p, c.post, cross_covariances=True), ref, name="source_pendulum")
    _check(bfa.rts_smoother(c.p, c.post, cross_covariances=True, options=GENERIC), ref, name="source_generic_pendulum")
    es = bfa.extended_kalman_smoother(c.p, c.ys)      # the README's call site, end to end
    assert np.array_equal(_np(es.smoothed_means), _np(bfa.rts_smoother(c.p, c.post).smoothed_means))


# 4 -----------------------------------------------------------------------------------------------------------------
def test_linear_map_as_source():
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    a = cm.random_stable_lgssm(4, 2, seed=8, dq=2)
    B, T = 64, 20
    ys = cm.simulate_batch(a, B, T, seed=8)
    p = cm.product_params(a)
    post = bfa.kalman_filter(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
    theta = np.concatenate([a["A"].ravel(), a["G"].ravel()])
    src = p._replace(dynamics_function=nl.user_dynamics(sc.LIN_SRC, 4, 2, theta=theta))
    lin = bfa.rts_smoother(p, post, cross_covariances=True)           # bf_rts_smoother_f32 on the same streams
    for opt in (None, GENERIC):
        usr = bfa.rts_smoother(src, post, cross_covariances=True, options=opt)
        for x, y in zip(lin[2:], usr[2:]):
            assert cm.rel_err(_np(y), _np(x)) <= 1e-6, opt


# 5 -----------------------------------------------------------------------------------------------------------------
def test_data_paths_and_chunks_bit_for_bit():
    import torch
    import bayesianfiltering_amd as bfa
    # rows on 16 bytes: T n = 48, T n^2 = 144 and, for the T-1 cross-covariances of a call without a carry, (T-1) n^2 = 135 is
    # not -- rts_pick_path's rule then takes the T-step pitch the allocation has (the view is a slice of a (B, 1, T, n, n) buffer)
    B, T, s = 130, 16, 8
    c = sc.case("lorenz63", B, T)
    staged = bfa.rts_smoother(c.p, c.post, cross_covariances=True, options={"rts_load_mode": 2})
    strided = bfa.rts_smoother(c.p, c.post, cross_covariances=True, options={"rts_load_mode": 0})
    for x, y in zip(staged[2:], strided[2:]):
        assert torch.equal(x, y)
    _check(staged, _oracle(c.post, None, c.jac), name="source_staged")
    for opt in ({"rts_load_mode": 2}, {"rts_load_mode": 0}):
        late, carry = bfa.rts_smoother(c.p, sc.cut(c.post, s, T), cross_covariances=True, return_carry=True, options=opt)
        early = bfa.rts_smoother(c.p, sc.cut(c.post, 0, s), carry=carry, cross_covariances=True, options=opt)
        for k in ("smoothed_means", "smoothed_covariances", "smoothed_cross_covariances"):
            assert torch.equal(torch.cat([getattr(early, k), getattr(late, k)], dim=2), getattr(staged, k)), (k, opt)
    post_bi = sc._filtered(c.p, c.ys, None, B, 3, layout="batch_inner")
    bi = bfa.rts_smoother(c.p, post_bi, cross_covariances=True, layout="batch_inner")
    for x, y in zip(staged[2:], bi[2:]):
        assert np.array_equal(_np(x), _np(y))


# 6 -----------------------------------------------------------------------------------------------------------------
def test_emission_from_source_runs_the_registry_instance():
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    B, T = 66, 12
    m0, Q, R = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32), 0.5 * np.eye(1, dtype=F32)
    reg = bfa.ParamsNLSSM(m0, np.eye(3, dtype=F32), nl.lorenz63(), np.zeros(3, F32), Q, nl.quadratic(3, c=0.1), np.zeros(1, F32), R)
    usr = reg._replace(emission_function=nl.user_emission(sc.QUAD_EMI_SRC, 3, 1, theta=[0.1]))
    ys = np.random.default_rng(4).normal(size=(B, T, 1)).astype(F32) + 0.3
    post = sc._filtered(reg, ys, None, B, 3)
    for opt in (None, GENERIC):
        a = bfa.rts_smoother(reg, post, cross_covariances=True, options=opt)
        b = bfa.rts_smoother(usr, post, cross_covariances=True, options=opt)
        for x, y in zip(a[2:], b[2:]):
            assert np.array_equal(_np(x), _np(y)), opt


# 7 -----------------------------------------------------------------------------------------------------------------
def test_refusals_that_stay():
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import _lib
    from bayesianfiltering_amd.inference import _Model, _stream_desc
    c = sc.case("lorenz63", 5, 16)
    lib = _lib.require_gpu()
    mdl = _Model(c.p)
    fd, sd = _lib.bf_out_desc(), _lib.bf_smooth_desc()
    fd.means, fd.covs = _stream_desc(c.post.means, 1), _stream_desc(c.post.covariances, 2)
    fd.pred_means, fd.pred_covs = _stream_desc(c.post.predicted_means, 1), _stream_desc(c.post.predicted_covariances, 2)
    import torch
    ms, Ps = torch.empty_like(c.post.means), torch.empty_like(c.post.covariances)
    sd.means, sd.covs = _stream_desc(ms, 1), _stream_desc(Ps, 2)
    ud = _lib.bf_cstream()
    call = lambda m_: lib.bf_eks_smoother_f32(C.byref(m_), C.byref(ud), C.byref(fd), 5, 16, None, C.byref(sd), None)
    assert call(mdl.c) == _lib.BF_OK
    other = _lib.bf_model.from_buffer_copy(mdl.c)     # a handle compiled for other dimensions
    other.user = _Model(sc.case("growth", 66, 24).p).c.user
    assert call(other) == _lib.BF_EINVAL
    leg = _lib.bf_model.from_buffer_copy(mdl.c)
    leg.flags = _lib.BF_MODEL_PREDICT_FIRST
    assert call(leg) == _lib.BF_EUNSUPPORTED
    torch.cuda.synchronize()
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    for fn in (lambda: bfa.rts_smoother(c.p, c.post, uparams=up),
               lambda: bfa.posterior_sample(c.p, c.post, 2, key=bfa.PRNGKey(0), uparams=up)):
        with pytest.raises(bfa.BayesFiltError) as e:      # the unscented route does not serve functions from source
            fn()
        assert e.value.code == -2 and "source" in str(e.value)
