"""GPU parity of the run-time-dimension unscented Gaussian-sum filter (csrc/ugsf_generic.hip: state in LDS, any of n, dq, m,
dr above 8, any number of components) against the NumPy oracle (gaussfiltax/inference.py:379-456, 146-174, 198-224).

Tolerance.  The oracle takes sqrtm from a float64 eigh, the device from a float32 parallel Jacobi, so the comparison has a
model-dependent noise floor.  It is measured here, on the CPU: the oracle is run a second time with ``go.sym_sqrtm`` replaced
(in this file only) by a float32 eigh, and d32 is the largest deviation between the two oracle runs.  Means, covariances and
predicted streams: max(2e-5, 8 d32) relative; weights: max(5e-5, 8 d32) absolute (2e-5 / 5e-5 are test_ugsf_gpu.py's figures
for the register kernel; the factor 8 covers the different rotation order of a parallel Jacobi).  Every figure is printed before
it is asserted (pytest -s shows them; DESIGN.md 4c records them)."""
import contextlib

import numpy as np
import pytest

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import common as cm

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("means", "covariances", "predicted_means", "predicted_covariances")
ALL5 = ("weights",) + FIELDS
UP = (1.0, 0.0, 0.0)


def _nl():
    import bayesianfiltering_amd as bfa
    return bfa, bfa.nonlinearities


def _sqrtm_f32(P):
    """go.sym_sqrtm with the eigen-decomposition in float32: the precision the device works in."""
    P = np.asarray(P, dtype=F32)
    if not np.all(np.isfinite(P)):
        return np.full(P.shape, np.nan, dtype=F32)
    lam, V = np.linalg.eigh(P)
    return ((V * np.sqrt(np.maximum(lam, F32(0)))) @ V.T).astype(F32)


@contextlib.contextmanager
def _float32_sqrtm():
    keep = go.sym_sqrtm
    go.sym_sqrtm = _sqrtm_f32
    try:
        yield
    finally:
        go.sym_sqrtm = keep


def _oracle_batch(p, up, ys, K, init, inputs=None):
    outs = {k: [] for k in ALL5 + ("loglik",)}
    for b in range(ys.shape[0]):
        post, ll = go.unscented_gaussian_sum_filter(p, go.ParamsUKF(*up), ys[b], K, initial_means=init[b], inputs=inputs, return_ll=True)
        for k in ALL5:
            outs[k].append(getattr(post, k))
        outs["loglik"].append(ll)
    return {k: np.stack(v) for k, v in outs.items()}


def _reference(p, up, ys, K, init, inputs=None):
    """(oracle streams, relative tolerance, weight tolerance): the float64-sqrtm oracle and the tolerances from its float32 twin."""
    ref = _oracle_batch(p, up, ys, K, init, inputs)
    with _float32_sqrtm():
        r32 = _oracle_batch(p, up, ys, K, init, inputs)
    assert all(np.isfinite(ref[k]).all() for k in ALL5), "the oracle itself is not finite on this model"
    d32 = max(cm.rel_err(r32[k], ref[k]) for k in FIELDS)
    dw = float(np.max(np.abs(r32["weights"] - ref["weights"])))
    tol, wtol = max(2e-5, 8 * d32), max(5e-5, 8 * dw)
    print(f"  oracle float32-sqrtm floor: d32 = {d32:.2e}, weights {dw:.2e} -> tolerances {tol:.1e} / {wtol:.1e}")
    return ref, tol, wtol


def _np(post):
    return {k: getattr(post, k).cpu().numpy() for k in ALL5}


def _check(got, ref, tol, wtol, what=""):
    errs = {k: cm.rel_err(got[k], ref[k]) for k in FIELDS}
    ew = float(np.max(np.abs(got["weights"] - ref["weights"])))
    print(f"  {what} device vs oracle: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f", weights {ew:.2e} (abs)")
    for k in FIELDS:
        assert got[k].shape == ref[k].shape, k
        assert errs[k] < tol, (what, k, errs[k], tol)
    assert ew < wtol, (what, ew, wtol)


def _l96(n, mode="matrix_power"):
    bfa, nl = _nl()
    m = n // 2
    args = (np.zeros(n, F32), np.eye(n, dtype=F32))
    noise = (np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32)), (np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Lorenz96(n, mode=mode), *noise[0], om.PickEven(n), *noise[1])
    pp = bfa.ParamsNLSSM(*args, nl.lorenz96(n, mode=mode), *noise[0], nl.pick_even(n), *noise[1])
    return po, pp


def _l96_data(po, n, B, T, K):
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(b), T)[1] for b in range(B)])
    init = np.random.default_rng(K).normal(size=(B, K, n)).astype(F32)
    return ys, init


@pytest.mark.parametrize("uparams", [(1.0, 0.0, 0.0), (0.5, 2.0, 1.0)])
def test_linear_model_awkward_sizes(uparams):
    """n = 9, dq = 3 (non-identity G), m = dr = 5, K = 3: nothing is a multiple of 4 and every size sits just past the register
    kernel's limit.  The unscented transform is exact for linear f, h, so the extended filter is a second reference (5e-5, as in
    test_ugsf_gpu.py).  Measured on MI355X: streams <= 9.9e-7, weights <= 6.6e-7, log-likelihood <= 7.2e-7, vs the extended
    filter <= 1.6e-6."""
    bfa, nl = _nl()
    n, T, B, K = 9, 12, 3, 3
    a = cm.random_stable_lgssm(n, 5, seed=9, dq=3, dr=5, bias=True)
    po, pp = cm.oracle_params(a), cm.product_params(a)
    ys = cm.simulate_batch(a, B, T, seed=1)
    init = (a["m0"] + np.random.default_rng(0).normal(size=(B, K, n))).astype(F32)
    ref, tol, wtol = _reference(po, uparams, ys, K, init)
    post, ll = bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*uparams), ys, K, 1, initial_means=init, return_loglik=True)
    assert tuple(post.means.shape) == (B, K, T, n) and tuple(post.covariances.shape) == (B, K, T, n, n)
    _check(_np(post), ref, tol, wtol)
    e_ll = cm.rel_err(ll.cpu().numpy(), ref["loglik"])
    print(f"  loglik {e_ll:.2e}")
    assert e_ll < 5e-5
    ekf = bfa.gaussian_sum_filter(pp, ys, K, 1, initial_means=init)
    for k in FIELDS:
        e = cm.rel_err(getattr(post, k).cpu().numpy(), getattr(ekf, k).cpu().numpy())
        print(f"  vs extended filter: {k} {e:.2e}")
        assert e < 5e-5, k
    one = bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*uparams), ys[0], K, 1, initial_means=init[0])   # unbatched: (K, T, ...)
    assert tuple(one.means.shape) == (K, T, n) and tuple(one.covariances.shape) == (K, T, n, n)
    assert np.array_equal(one.means.cpu().numpy(), post.means[0].cpu().numpy())


@pytest.mark.parametrize("n,K,T,mode", [(12, 3, 12, "matrix_power"), (12, 3, 12, "as_written"), (20, 2, 12, "matrix_power"),
                                        (40, 2, 8, "matrix_power")])
def test_lorenz96_with_pick_even(n, K, T, mode):
    """n = 12: one wave per trajectory, the 48 sigma points of a prediction fit it; n = 20: the four-wave instance (above 16), 80
    points; n = 40: 160 points, 55 KiB of LDS.  Measured on MI355X (worst stream / weights): n = 12 matrix_power 9.6e-7 / 1.8e-7,
    as_written 9.1e-7 / 1.2e-7; n = 20 1.6e-6 / 1.1e-6; n = 40 2.6e-6 / 7.8e-7.  (Without the Newton step on the square root
    the n = 12 matrix_power covariances were at 2.3e-5, above the tolerance: csrc/ugsf_generic_device.hpp, ug_sym_sqrt.)"""
    bfa, nl = _nl()
    po, pp = _l96(n, mode)
    ys, init = _l96_data(po, n, 2, T, K)
    ref, tol, wtol = _reference(po, UP, ys, K, init)
    post = bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init)
    _check(_np(post), ref, tol, wtol, f"n = {n} {mode}")


def test_more_components_than_lanes():
    """K = 260: the components take turns in the LDS tile, so the register kernel's limit of 256 does not exist on this path.
    Measured on MI355X: streams 1.0e-6, weights 2.4e-7."""
    bfa, nl = _nl()
    n, K, T = 12, 260, 4
    po, pp = _l96(n)
    ys, init = _l96_data(po, n, 1, T, K)
    ref, tol, wtol = _reference(po, UP, ys, K, init)
    post = bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init)
    assert tuple(post.weights.shape) == (1, K, T)
    _check(_np(post), ref, tol, wtol, "K = 260")


def test_sine_dynamics_with_quadratic_emission():
    """n = 12, m = dr = 1 (f1 / g1 of Experiment_TSP_2023.ipynb at a larger state).  Measured on MI355X: streams 9.7e-7, weights 2.4e-7."""
    bfa, nl = _nl()
    n, K, T, B = 12, 3, 12, 2
    args = (np.zeros(n, F32), np.eye(n, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Sine(n, 1.5), np.zeros(n, F32), 0.1 * np.eye(n, dtype=F32), om.Quadratic(n, 0.05), np.zeros(1, F32),
                        0.5 * np.eye(1, dtype=F32))
    pp = bfa.ParamsNLSSM(*args, nl.sine(n, 1.5), np.zeros(n, F32), 0.1 * np.eye(n, dtype=F32), nl.quadratic(n, 0.05), np.zeros(1, F32),
                         0.5 * np.eye(1, dtype=F32))
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(5 + b), T)[1] for b in range(B)])
    init = np.random.default_rng(2).normal(size=(B, K, n)).astype(F32)
    ref, tol, wtol = _reference(po, UP, ys, K, init)
    _check(_np(bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init)), ref, tol, wtol)


def _stoch_vol(n, R):
    bfa, nl = _nl()
    Phi = 0.8 * np.eye(n, dtype=F32)
    Q = 0.5 * np.eye(n, dtype=F32)
    r0 = (0.1 * np.cos(np.arange(n))).astype(F32)
    args = (np.zeros(n, F32), np.eye(n, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Linear(Phi), np.zeros(n, F32), Q, om.StochVol(n), r0, R)
    pp = bfa.ParamsNLSSM(*args, nl.linear_dynamics(Phi), np.zeros(n, F32), Q, nl.stoch_vol(n), r0, R)
    return po, pp


def test_stochastic_volatility_multiplicative_noise():
    """h(x, r, u) = u beta exp(x / sigma) r + (1 - u)(c x + r) at n = m = dr = 10, the input switching 0 -> 1 halfway, nonzero
    r0: the noise the augmented sigma points exist for.  Measured on MI355X: streams 3.5e-7, weights 1.3e-6."""
    bfa, nl = _nl()
    n, K, T, B = 10, 3, 12, 2
    R = 1e-1 * np.eye(n, dtype=F32)
    po, pp = _stoch_vol(n, R)
    inputs = np.array([0] * 6 + [1] * 6, F32)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(3 + b), T, inputs.reshape(T, 1))[1] for b in range(B)])
    init = np.random.default_rng(1).normal(size=(B, K, n)).astype(F32)
    ref, tol, wtol = _reference(po, UP, ys, K, init, inputs.reshape(T, 1))
    _check(_np(bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, inputs, initial_means=init)), ref, tol, wtol)


def _spd_table(rng, base, T):
    d = base.shape[0]
    out = []
    for _ in range(T):
        w = rng.normal(size=(d, d)) * 0.3
        out.append(base * (0.5 + rng.uniform()) + 0.2 * np.mean(np.diag(base)) * (w @ w.T))
    return np.stack(out).astype(F32)


def test_time_varying_covariances():
    """Non-diagonal SPD tables Q_t / R_t at n = 12 on the linear model -- both, Q only, R only -- index the host's per-step
    sqrtm tables; the constant-covariance posterior is a different one (> 1e-2).  And R_t with the multiplicative-noise emission
    (R only enters the sigma points).  Measured on MI355X: streams <= 1.1e-6, weights <= 2.7e-6."""
    bfa, nl = _nl()
    rng = np.random.default_rng(5)
    n, T, B, K = 12, 12, 2, 3
    a = cm.random_stable_lgssm(n, 6, seed=12)
    po, pp = cm.oracle_params(a), cm.product_params(a)
    Qt, Rt = _spd_table(rng, a["Q"], T), _spd_table(rng, a["R"], T)
    ys = cm.simulate_batch(a, B, T, seed=2)
    init = (a["m0"] + rng.normal(size=(B, K, n))).astype(F32)
    for kw in ({"dynamics_noise_covariance": Qt, "emission_noise_covariance": Rt}, {"dynamics_noise_covariance": Qt},
               {"emission_noise_covariance": Rt}):
        ref, tol, wtol = _reference(po._replace(**kw), UP, ys, K, init)
        post, ll = bfa.unscented_gaussian_sum_filter(pp._replace(**kw), bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init, return_loglik=True)
        _check(_np(post), ref, tol, wtol, "+".join(k[:3] for k in kw))
        assert cm.rel_err(ll.cpu().numpy(), ref["loglik"]) < 5e-5
    const = bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init)
    assert cm.rel_err(const.covariances.cpu().numpy(), ref["covariances"]) > 1e-2

    n2, K2 = 10, 3
    R = 1e-1 * np.eye(n2, dtype=F32)
    Rt2 = _spd_table(rng, R, T)
    po2, pp2 = _stoch_vol(n2, Rt2)
    inputs = np.array([0] * 6 + [1] * 6, F32)
    ys2 = np.stack([go.sample_ssm(po2._replace(emission_noise_covariance=R), otf.PRNGKey(3 + b), T, inputs.reshape(T, 1))[1] for b in range(B)])
    init2 = rng.normal(size=(B, K2, n2)).astype(F32)
    ref2, tol, wtol = _reference(po2, UP, ys2, K2, init2, inputs.reshape(T, 1))
    _check(_np(bfa.unscented_gaussian_sum_filter(pp2, bfa.ParamsUKF(*UP), ys2, K2, 1, inputs, initial_means=init2)), ref2, tol, wtol, "stoch_vol R_t")


def test_bit_for_bit_equalities():
    """Two chunks through the carry equal one scan; layout='batch_inner' equals layout='reference'; a fields subset equals the
    corresponding streams of the full call; a batch of B equals B single calls -- all exactly."""
    bfa, nl = _nl()
    n, K, T, B = 12, 3, 12, 3
    po, pp = _l96(n)
    ys, init = _l96_data(po, n, B, T, K)
    up = bfa.ParamsUKF(*UP)
    full, ll = bfa.unscented_gaussian_sum_filter(pp, up, ys, K, 1, initial_means=init, return_loglik=True)
    full = _np(full)
    assert all(np.isfinite(v).all() for v in full.values())
    p1, c1 = bfa.unscented_gaussian_sum_filter(pp, up, ys[:, :5], K, 1, initial_means=init, return_carry=True)
    p2 = bfa.unscented_gaussian_sum_filter(pp, up, ys[:, 5:], K, 1, carry=c1)
    p1, p2 = _np(p1), _np(p2)
    for k in ALL5:
        assert np.array_equal(np.concatenate([p1[k], p2[k]], axis=2), full[k]), k
    bi = bfa.unscented_gaussian_sum_filter(pp, up, ys, K, 1, initial_means=init, layout="batch_inner")
    for k in ALL5:
        assert np.array_equal(getattr(bi, k).cpu().numpy(), full[k]), k
    sub, ll2 = bfa.unscented_gaussian_sum_filter(pp, up, ys, K, 1, initial_means=init, fields=("weights", "predicted_covariances"),
                                                 return_loglik=True)
    assert sub.means is None and sub.covariances is None and sub.predicted_means is None
    assert np.array_equal(sub.weights.cpu().numpy(), full["weights"])
    assert np.array_equal(sub.predicted_covariances.cpu().numpy(), full["predicted_covariances"])
    assert np.array_equal(ll2.cpu().numpy(), ll.cpu().numpy())
    again = bfa.unscented_gaussian_sum_filter(pp, up, ys, K, 1, initial_means=init, out=bi, layout="batch_inner")   # out= reuse
    assert again.means.data_ptr() == bi.means.data_ptr() and np.array_equal(again.means.cpu().numpy(), full["means"])
    for b in range(B):
        one = _np(bfa.unscented_gaussian_sum_filter(pp, up, ys[b], K, 1, initial_means=init[b]))
        for k in ALL5:
            assert np.array_equal(one[k], full[k][b]), (k, b)


def test_both_kernels_on_one_model():
    """Lorenz-96 at n = 8 through options={"ugsf_force_generic": 1} and through the default register kernel: each is within
    the parity tolerance of the oracle, so they are within twice that of each other.  Measured on MI355X: this kernel vs oracle
    5.9e-7 (weights 8.9e-7), register kernel vs oracle 3.7e-6 (weights 2.0e-6), the two kernels 4.1e-6 apart."""
    bfa, nl = _nl()
    n, K, T, B = 8, 3, 12, 2
    po, pp = _l96(n)
    ys, init = _l96_data(po, n, B, T, K)
    ref, tol, wtol = _reference(po, UP, ys, K, init)
    gen = _np(bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init, options={"ugsf_force_generic": 1}))
    reg = _np(bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), ys, K, 1, initial_means=init))
    _check(gen, ref, tol, wtol, "run-time-dimension kernel")
    _check(reg, ref, tol, wtol, "register kernel")
    assert not all(np.array_equal(gen[k], reg[k]) for k in ALL5), "the option did not select another kernel"
    for k in FIELDS:
        e = cm.rel_err(gen[k], reg[k])
        print(f"  between the kernels: {k} {e:.2e}")
        assert e < 2 * tol, k
    assert np.max(np.abs(gen["weights"] - reg["weights"])) < 2 * wtol


SINE_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  for (int i = 0; i < BF_N; ++i) out[i] = sin(th[0] * x[i]) + q[i];
}
"""
LINEAR_EMI_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  for (int a = 0; a < BF_M; ++a) {
    T s = th[a * BF_N] * x[0];
    for (int k = 1; k < BF_N; ++k) s = s + th[a * BF_N + k] * x[k];
    out[a] = s + r[a];
  }
}
"""


def test_functions_from_source_and_recorded_python_functions():
    """Sine dynamics + a dense linear emission at n = 12, m = 6, three ways: registry functions (ahead-of-time kernel), their
    twins as source (the same kernel built at run time around the caller's float functions; 72 emission parameters), and plain
    Python lambdas of NumPy operations (recorded by trace.py into source).  The lambdas give the arrays of the source twin; the
    twin agrees with the registry path and with the oracle at the parity tolerance.  Measured on MI355X: source twin vs oracle
    3.8e-6 (weights 1.6e-6), registry path vs oracle 5.0e-6, source twin vs the registry path 1.5e-6."""
    bfa, nl = _nl()
    n, m, K, T, B = 12, 6, 3, 12, 2
    w0 = 1.5
    H = (np.random.default_rng(7).normal(size=(m, n)) / np.sqrt(n)).astype(F32)
    args = (np.zeros(n, F32), np.eye(n, dtype=F32))
    qn, rn = (np.zeros(n, F32), 0.1 * np.eye(n, dtype=F32)), (np.zeros(m, F32), 0.2 * np.eye(m, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Sine(n, w0), *qn, om.Linear(H), *rn)
    reg = bfa.ParamsNLSSM(*args, nl.sine(n, w0), *qn, nl.linear_emission(H), *rn)
    src = bfa.ParamsNLSSM(*args, nl.user_dynamics(SINE_SRC, n, theta=[w0]), *qn, nl.user_emission(LINEAR_EMI_SRC, n, m, theta=H.reshape(-1)), *rn)
    lam = bfa.ParamsNLSSM(*args, lambda x, q, u: np.sin(F32(w0) * x) + q, *qn, lambda x, r, u: H @ x + r, *rn)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(7 + b), T)[1] for b in range(B)])
    init = np.random.default_rng(3).normal(size=(B, K, n)).astype(F32)
    ref, tol, wtol = _reference(po, UP, ys, K, init)
    up = bfa.ParamsUKF(*UP)
    a = _np(bfa.unscented_gaussian_sum_filter(reg, up, ys, K, 1, initial_means=init))
    b = _np(bfa.unscented_gaussian_sum_filter(src, up, ys, K, 1, initial_means=init))
    c = _np(bfa.unscented_gaussian_sum_filter(lam, up, ys, K, 1, initial_means=init))
    _check(a, ref, tol, wtol, "registry")
    _check(b, ref, tol, wtol, "source twin")
    _check(b, a, tol, wtol, "source twin vs registry:")
    for k in ALL5:
        assert np.array_equal(c[k], b[k]), k


def test_lds_limit_is_reported_with_the_byte_count():
    """n = dq = 80, m = dr = 40, K = 2 needs 215,424 bytes of LDS (ug_carve in csrc/ugsf_generic_device.hpp), above the 160 KiB of a
    workgroup: refused before anything is launched, with the figure."""
    bfa, nl = _nl()
    n = 80
    _, pp = _l96(n)
    with pytest.raises(bfa.BayesFiltError, match="need 215424 bytes of LDS"):
        bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), np.zeros((2, n // 2), F32), 2)


def test_nan_emission_stays_in_its_trajectory():
    """One trajectory of three gets a NaN observation at step 5: its means, weights and log-likelihoods are NaN from that step
    on and its covariances from the prediction of that step on (P - K S K^T itself does not read y); the other two
    trajectories are untouched, bit for bit.  The Jacobi sweep loop has a compile-time bound (UG_MAX_SWEEPS) and leaves on one
    LDS value every lane reads -- a NaN matrix fails the first `off > 1e-14 diag` test on every lane alike -- so the call returns."""
    bfa, nl = _nl()
    n, K, T, B = 12, 2, 8, 3
    po, pp = _l96(n)
    ys, init = _l96_data(po, n, B, T, K)
    up = bfa.ParamsUKF(*UP)
    clean, ll0 = bfa.unscented_gaussian_sum_filter(pp, up, ys, K, 1, initial_means=init, return_loglik=True)
    clean = _np(clean)
    bad = ys.copy()
    bad[1, 5, 0] = np.nan
    post, ll = bfa.unscented_gaussian_sum_filter(pp, up, bad, K, 1, initial_means=init, return_loglik=True)
    post = _np(post)
    for k in ALL5:
        assert np.array_equal(post[k][[0, 2]], clean[k][[0, 2]]), k
        assert np.array_equal(post[k][1, :, :5], clean[k][1, :, :5]), k
    for k in ("means", "weights", "predicted_means", "predicted_covariances"):
        assert np.isnan(post[k][1, :, 5:]).all(), k
    assert np.isnan(ll.cpu().numpy()[1, :, 5:]).all()
    assert np.isfinite(post["covariances"][1, :, 5]).all() and np.isnan(post["covariances"][1, :, 6:]).all()
