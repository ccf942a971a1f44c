"""Unscented RTS smoother and posterior sampler on the MI355X (bf_uks_smoother_f32, bf_uffbs_sample_f32): parity with the
float64 restatement of tests/unscented_smoother_cases.py (pinned without a GPU by tests/test_unscented_smoother_cpu.py) over
the GPU's own filtered streams, on the register kernels and on the run-time-dimension kernels.

Tolerance: 1e-5 norm-wise (cm.rel_err), the project's bar for every smoother, sampler and unscented-filter parity test.  A
float32 NumPy emulation of the recursion gave <= 1.6e-6 on the nonlinear cases and <= 4.9e-6 on the linear identity (worst
at n = 12).  Measured on MI355X (cm.record: "usmoother_*" / "usampler_*"): linear identity <= 7.6e-6 on the register kernel
(n = 4, alpha = 1, covariances) and <= 3.0e-6 on the run-time-dimension kernel; nonlinear cases <= 2.2e-6 on both; sampler
<= 2.0e-7 at n <= 3 and 3.8e-6 on Lorenz-96 at n = 12, zero noise against the smoothed means <= 5.1e-8."""
import functools

import numpy as np
import pytest

from tests import common as cm
from tests import unscented_smoother_cases as uc
from tests.test_smoother_cpu import rts_f64
from tests.test_sampler_cpu import TAU

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 1e-5
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")
SMOOTHED = ("smoothed_means", "smoothed_covariances", "smoothed_cross_covariances")
UPARAMS = [(1.0, 0.0, 0.0), (0.5, 2.0, 1.0)]
GEN = {"force_generic": 1}


def _np(x):
    return x.detach().cpu().numpy()


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _streams(post):
    return tuple(_np(getattr(post, k))[:, 0] for k in STREAMS)


def _check_smoothed(sm, ref, name):
    ms, Ps, Cs = ref
    e = (cm.rel_err(_np(sm.smoothed_means)[:, 0], ms), cm.rel_err(_np(sm.smoothed_covariances)[:, 0], Ps),
         cm.rel_err(_np(sm.smoothed_cross_covariances)[:, 0], Cs[:, :-1]))
    cm.record("usmoother_" + name, errs=list(e))
    print(f"  {name}: means {e[0]:.2e} covariances {e[1]:.2e} cross-covariances {e[2]:.2e}")
    assert max(e) < TOL, (name, e)


# ---- 1: linear dynamics: the unscented and the linear smoother are the same function of the streams -----------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 12])
def test_linear_identity(n):
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(n, min(n, 2), seed=60 + n)
    B, T = 70, 20
    ys = cm.simulate_batch(a, B, T, seed=n)
    p = cm.product_params(a)
    post = bfa.kalman_filter(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
    m, P, pm, pP = _streams(post)
    out = [rts_f64(m[b], P[b], pm[b], pP[b], a["A"]) for b in range(B)]
    ref = tuple(np.stack([o[i] for o in out]) for i in range(3))
    for up in UPARAMS:
        tag = f"linear_n{n}_a{up[0]}"
        _check_smoothed(bfa.rts_smoother(p, post, uparams=bfa.ParamsUKF(*up), cross_covariances=True), ref, tag)
        if n <= 8:
            _check_smoothed(bfa.rts_smoother(p, post, uparams=up, cross_covariances=True, options=GEN), ref, tag + "_generic")


# ---- 2: nonlinear dynamics against the float64 restatement over the GPU's own unscented streams --------------------------
class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(kind, up):
    """Model, data, the GPU's unscented streams for ``up`` and the float64 X_t / smoothed reference over them (built once)."""
    # (Lorenz-63 under the quadratic emission alone leaves directions unobserved: P_t grows and the float64 pivots of Sigma_t
    # fall to 5.5e-4 d_j, under the 100 tau the sampler test asks of them -- the sampler takes "lorenz63_lin" instead)
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    rng = np.random.default_rng(17)
    c = Case()
    c.B, c.T, c.u, c.small = 66, 24, None, True
    if kind == "lorenz63":      # quadratic emission (Experiment_TSP_2023)
        n, f, c.f64 = 3, nl.lorenz63(), uc.lorenz63_f()
        m0, P0, Q = np.array([0.0, 1.0, 1.05], F32), np.eye(3, dtype=F32), 0.1 * np.eye(3, dtype=F32)
        h, r0, R = nl.quadratic(3, 0.05), np.zeros(1, F32), np.eye(1, dtype=F32)
    elif kind == "lorenz63_lin":    # every state observed: Sigma_t stays a fixed fraction of P_t (the sampler's case)
        n, f, c.f64 = 3, nl.lorenz63(), uc.lorenz63_f()
        m0, P0, Q = np.array([0.0, 1.0, 1.05], F32), np.eye(3, dtype=F32), 0.1 * np.eye(3, dtype=F32)
        h, r0, R = nl.linear_emission(np.eye(3, dtype=F32)), np.zeros(3, F32), 0.5 * np.eye(3, dtype=F32)
    elif kind == "sine":
        n, f, c.f64 = 2, nl.sine(2, w0=1.0), uc.sine_f(1.0)
        m0, P0, Q = np.array([0.3, -0.2], F32), np.eye(2, dtype=F32), 0.1 * np.eye(2, dtype=F32)
        h, r0, R = nl.linear_emission(np.eye(2, dtype=F32)), np.zeros(2, F32), 0.2 * np.eye(2, dtype=F32)
    elif kind == "growth":      # with inputs
        n, f, c.f64 = 1, nl.growth(), uc.growth_f()
        m0, P0, Q = np.array([0.1], F32), np.eye(1, dtype=F32), np.eye(1, dtype=F32)
        h, r0, R = nl.linear_emission(np.eye(1, dtype=F32)), np.zeros(1, F32), np.eye(1, dtype=F32)
        c.u = (8 * np.cos(1.2 * np.arange(c.T))).astype(F32)
    elif kind == "maneuver":    # bearing + range, inputs in {0, 1, 2}; dq = 2 != n = 4
        n, f, c.f64 = 4, nl.maneuver_bot(), uc.maneuver_f()
        m0, P0 = np.array([2.0, 0.3, 3.0, -0.2], F32), np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
        Q = 1e-3 * np.eye(2, dtype=F32)
        h, r0, R = nl.bearing_range(), np.zeros(2, F32), np.diag([1e-3, 1e-2]).astype(F32)
        c.u = np.array([1] * 8 + [0] * 8 + [2] * 8, F32)
    else:                       # Lorenz-96 at n = 12: the run-time-dimension kernels only
        n, f, c.f64 = 12, nl.lorenz96(12), uc.lorenz96_f()
        m0, P0, Q = np.zeros(12, F32), np.eye(12, dtype=F32), 1e-2 * np.eye(12, dtype=F32)
        h, r0, R = nl.pick_even(12), np.zeros(6, F32), 1e-1 * np.eye(6, dtype=F32)
        c.T, c.small = 12, False
    dq = Q.shape[0]
    c.n, c.q0, c.up = n, np.zeros(dq, F32), up
    c.p = bfa.ParamsNLSSM(m0, P0, f, c.q0, Q, h, r0, R)
    LQ, LR, L0 = (np.linalg.cholesky(v.astype(np.float64)) for v in (Q, R, P0))
    x = (m0 + rng.normal(size=(c.B, n)) @ L0.T).astype(F32)
    ys = np.empty((c.B, c.T, R.shape[0]), F32)
    for t in range(c.T):
        ut = F32(0.0 if c.u is None else c.u[t])
        x = np.stack([f(x[b], (rng.normal(size=dq) @ LQ.T).astype(F32), ut) for b in range(c.B)]).astype(F32)
        ys[:, t] = np.stack([h(x[b], (rng.normal(size=R.shape[0]) @ LR.T).astype(F32), ut) for b in range(c.B)])
    c.ys = ys
    c.init = np.tile(m0, (c.B, 1)).reshape(c.B, 1, n)
    c.post = bfa.unscented_gaussian_sum_filter(c.p, bfa.ParamsUKF(*up), ys, 1, 1, c.u, initial_means=c.init)
    m, P, pm, pP = _streams(c.post)
    assert np.all(np.isfinite(pP)), kind
    c.X = np.stack([uc.ucross_stream(m[b], P[b], c.f64, c.u, up, c.q0) for b in range(c.B)])
    out = [uc.urts_f64(m[b], P[b], pm[b], pP[b], c.X[b]) for b in range(c.B)]
    c.ref = tuple(np.stack([o[i] for o in out]) for i in range(3))
    return c


KINDS = ["lorenz63", "sine", "growth", "maneuver", "lorenz96"]


@pytest.mark.parametrize("up", UPARAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_nonlinear_parity(kind, up):
    import bayesianfiltering_amd as bfa
    c = _case(kind, up)
    tag = f"{kind}_a{up[0]}"
    _check_smoothed(bfa.rts_smoother(c.p, c.post, inputs=c.u, uparams=up, cross_covariances=True), c.ref, tag)
    if c.small:
        _check_smoothed(bfa.rts_smoother(c.p, c.post, inputs=c.u, uparams=up, cross_covariances=True, options=GEN), c.ref,
                        tag + "_generic")


# ---- 3: bit for bit -----------------------------------------------------------------------------------------------------
def _cut(post, lo, hi):
    return post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in STREAMS})


@pytest.mark.parametrize("generic", [0, 1])
def test_bit_for_bit(generic):
    import torch
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    up = UPARAMS[0]
    c = _case("maneuver", up)       # inputs, dq != n, T = 24
    p, post, u, B, T, n, S, s = c.p, c.post, c.u, c.B, c.T, c.n, 3, 10
    opt = {"force_generic": generic}
    before = [getattr(post, k).clone() for k in STREAMS]
    full = bfa.rts_smoother(p, post, inputs=u, uparams=up, cross_covariances=True, options=opt)
    # the last step is the filtered step
    assert torch.equal(full.smoothed_means[:, :, -1], post.means[:, :, -1])
    assert torch.equal(full.smoothed_covariances[:, :, -1], post.covariances[:, :, -1])
    # a 10 / 14 backward split through the carry is the single call
    late, carry = bfa.rts_smoother(p, _cut(post, s, T), inputs=u[s:], uparams=up, cross_covariances=True, return_carry=True,
                                   options=opt)
    early = bfa.rts_smoother(p, _cut(post, 0, s), inputs=u[:s], uparams=up, carry=carry, cross_covariances=True, options=opt)
    for k in SMOOTHED:
        assert torch.equal(torch.cat([getattr(early, k), getattr(late, k)], dim=2), getattr(full, k)), k
    assert torch.equal(carry.means, late.smoothed_means[:, 0, 0])
    xi = np.random.default_rng(5).normal(size=(B, S, T, n)).astype(F32)
    xfull = bfa.posterior_sample(p, post, S, noise=_dev(xi), inputs=u, uparams=up, options=opt)
    xl, xc = bfa.posterior_sample(p, _cut(post, s, T), S, noise=_dev(xi[:, :, s:]), inputs=u[s:], uparams=up, return_carry=True,
                                  options=opt)
    xe = bfa.posterior_sample(p, _cut(post, 0, s), S, noise=_dev(xi[:, :, :s]), inputs=u[:s], uparams=up, carry=xc, options=opt)
    assert torch.equal(torch.cat([xe, xl], dim=2), xfull)
    assert torch.equal(xc.states, xl[:, :, 0])
    # T = 1: the filtered step, no cross-covariance; the sampler's first line
    one = bfa.rts_smoother(p, _cut(post, T - 1, T), inputs=u[T - 1:], uparams=up, cross_covariances=True, options=opt)
    assert torch.equal(one.smoothed_means, post.means[:, :, T - 1:]) and torch.equal(one.smoothed_covariances, post.covariances[:, :, T - 1:])
    assert tuple(one.smoothed_cross_covariances.shape) == (B, 1, 0, n, n)
    x1 = bfa.posterior_sample(p, _cut(post, T - 1, T), S, noise=_dev(xi[:, :, T - 1:]), inputs=u[T - 1:], uparams=up, options=opt)
    assert torch.equal(x1, xfull[:, :, T - 1:])
    # key = noise filled from random.normal
    key = bfa.PRNGKey(7)
    keys = bfr.split(key, B)
    zk = np.stack([bfr.normal(keys[b], (S, T, n)) for b in range(B)])
    by_key = bfa.posterior_sample(p, post, S, key=key, inputs=u, uparams=up, options=opt)
    assert torch.equal(by_key, bfa.posterior_sample(p, post, S, noise=_dev(zk), inputs=u, uparams=up, options=opt))
    # out= reuse
    again = bfa.rts_smoother(p, post, inputs=u, uparams=up, out=full, options=opt)
    for k in SMOOTHED:
        assert getattr(again, k).data_ptr() == getattr(full, k).data_ptr()
    keep = xfull.clone()
    xo = bfa.posterior_sample(p, post, S, noise=_dev(xi), inputs=u, uparams=up, out=xfull, options=opt)
    assert xo.data_ptr() == xfull.data_ptr() and torch.equal(xo, keep)
    # the wrappers are the filter followed by the backward pass
    ws = bfa.unscented_kalman_smoother(p, up, c.ys, inputs=u, cross_covariances=True, options=opt)
    for k in SMOOTHED:
        assert torch.equal(getattr(ws, k), getattr(full, k)), k
    wx = bfa.unscented_kalman_posterior_sample(p, up, c.ys, S, key, inputs=u, options=opt)
    assert torch.equal(wx, by_key)
    # the input streams are as they were
    for k, b in zip(STREAMS, before):
        assert torch.equal(getattr(post, k), b), k


# ---- 4: the sampler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,S,generic", [("lorenz63_lin", 1, 0), ("lorenz63_lin", 5, 0), ("lorenz63_lin", 5, 1), ("sine", 5, 0),
                                            ("growth", 5, 0), ("lorenz96", 1, 1), ("lorenz96", 5, 1)])
def test_sampler_parity(kind, S, generic):
    import torch
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    up = UPARAMS[0]
    c = _case(kind, up)
    opt = {"force_generic": generic}
    B, T, n = c.B, c.T, c.n
    tag = f"{kind}_S{S}_g{generic}"
    # xi = 0 is the smoothed mean (1e-6: the bar tests/test_sampler_gpu.py sets for the existing routes)
    sm = bfa.rts_smoother(c.p, c.post, inputs=c.u, uparams=up, options=opt)
    x0 = bfa.posterior_sample(c.p, c.post, S, noise=torch.zeros((B, S, T, n), device="cuda"), inputs=c.u, uparams=up, options=opt)
    e0 = max(cm.rel_err(_np(x0[:, s_]), _np(sm.smoothed_means[:, 0])) for s_ in range(S))
    # xi from a key, against the restatement on the same xi; full-rank Q: no pivot of Sigma_t may come near the threshold
    key = bfa.PRNGKey(11)
    keys = bfr.split(key, B)
    xi = np.stack([bfr.normal(keys[b], (S, T, n)) for b in range(B)])
    m, P, pm, pP = _streams(c.post)
    piv = []
    ref = np.stack([uc.uffbs_f64(m[b], P[b], pm[b], pP[b], c.X[b], xi[b], pivots=piv) for b in range(B)])
    assert len(piv) == B * T
    ratios = np.array([r for rec in piv for r, _ in rec])
    kept = np.array([k for rec in piv for _, k in rec])
    assert kept.all() and np.all(ratios >= 100 * TAU), float(ratios.min())
    x = bfa.posterior_sample(c.p, c.post, S, key=key, inputs=c.u, uparams=up, options=opt)
    assert tuple(x.shape) == (B, S, T, n)
    e = cm.rel_err(_np(x), ref)
    cm.record("usampler_" + tag, zero_noise=e0, err=e, smallest_pivot=float(ratios.min()))
    print(f"  {tag}: zero noise {e0:.2e}, samples {e:.2e}, smallest pivot ratio {ratios.min():.2e}")
    assert e0 <= 1e-6, e0
    assert e < TOL, e


# ---- 5: errors --------------------------------------------------------------------------------------------------------
L63_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  const float s = th[0], r = th[1], b = th[2], dt = th[3];
  out[0] = dt * s * (x[1] - x[0]) + x[0] + q[0];
  out[1] = dt * (x[0] * r - x[1] - x[0] * x[2]) + x[1] + q[1];
  out[2] = dt * (x[0] * x[1] - b * x[2]) + x[2] + q[2];
}
"""


def test_errors():
    import torch
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    key = bfa.PRNGKey(0)
    c = _case("lorenz63", UPARAMS[0])
    ys = c.ys[:4, :8]
    two = bfa.unscented_gaussian_sum_filter(c.p, up, ys, 2)
    bare = bfa.unscented_gaussian_sum_filter(c.p, up, ys, 1, fields=("means", "covariances"))
    small = _cut(c.post, 0, 4)
    for call in (lambda post, pp=c.p, **kw: bfa.rts_smoother(pp, post, **kw),
                 lambda post, pp=c.p, **kw: bfa.posterior_sample(pp, post, 2, key=key, **kw)):
        with pytest.raises(ValueError, match="one component"):
            call(two, uparams=up)
        with pytest.raises(ValueError, match="predicted"):
            call(bare, uparams=up)
        with pytest.raises(ValueError, match="extended=True"):
            call(small, uparams=up, extended=True)
        with pytest.raises(bfa.BayesFiltError) as e:      # L + lambda = alpha^2 (L + kappa) <= 0
            call(small, uparams=bfa.ParamsUKF(0.0, 2, 0))
        assert e.value.code == -1
        with pytest.raises(bfa.BayesFiltError) as e:      # dynamics from source
            usr = c.p._replace(dynamics_function=nl.user_dynamics(L63_SRC, 3, theta=[10.0, 28.0, 2.667, 0.01]))
            call(small, pp=usr, uparams=up)
        assert e.value.code == -2 and "source" in str(e.value)
    # n beyond the LDS capacity of the run-time-dimension kernels: refused with the limit, before any launch
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    for n, limit, call in ((80, "n <= 75", lambda p_, f_: bfa.rts_smoother(p_, f_, uparams=up)),
                           (84, "n <= 81", lambda p_, f_: bfa.posterior_sample(p_, f_, 2, key=key, uparams=up))):
        big = cm.product_params(cm.random_stable_lgssm(n, 2, seed=2))
        fake = bfa.PosteriorGaussianSumFiltered(None, z(2, 1, 3, n), z(2, 1, 3, n, n), z(2, 1, 3, n), z(2, 1, 3, n, n))
        with pytest.raises(bfa.BayesFiltError) as e:
            call(big, fake)
        assert e.value.code == -2 and limit in str(e.value), str(e.value)
