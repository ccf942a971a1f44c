"""Unscented smoother, no GPU: the float64 restatement of its contract (tests/unscented_smoother_cases.py) pinned against
the linear identity X_t = A P_t, against the textbook augmented unscented cross-covariance over all 2 L + 1 sigma points,
and -- through the smoother's recursion -- against the exact dense joint Gaussian of a linear model."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import unscented_smoother_cases as uc
from tests.test_smoother_cpu import kalman_f64, rts_f64, dense_posterior

F64 = np.float64
UPARAMS = [(1.0, 0.0, 0.0), (1.0, 2.0, 0.5), (0.5, 2.0, 1.0)]


def _spd(rng, n, scale):
    L = rng.normal(size=(n, n))
    return scale * (L @ L.T / n + 0.3 * np.eye(n))


@pytest.mark.parametrize("uparams", UPARAMS)
@pytest.mark.parametrize("n,dq", [(1, 1), (3, 3), (4, 2), (12, 12)])
def test_linear_dynamics_give_a_times_p(n, dq, uparams):
    """f = A x + G q: X = A P exactly (2 w c^2 = 1), whatever G, q0 and the unscented parameters."""
    rng = np.random.default_rng(n)
    A, G = rng.normal(size=(n, n)), rng.normal(size=(n, dq))
    m, P, q0 = rng.normal(size=n), _spd(rng, n, 0.7), rng.normal(size=dq)
    X = uc.ucross_f64(m, P, uc.linear_f(A, G), 0.0, uparams, q0)
    assert np.max(np.abs(X - A @ P)) <= 1e-12 * np.max(np.abs(A @ P))


def _textbook_cross(monkeypatch, m, P, f, u, uparams, q0, Q):
    """The state block of the augmented unscented cross-covariance (gaussfiltax/inference.py:146-174 with the points of
    utils.py:247-254): all 2 L sigma points of (m, q0), blockdiag(P, Q) from the oracle's _get_sigma_points -- run in float64,
    the oracle module's float32 type swapped for the call -- plus the centre."""
    monkeypatch.setattr(go, "F32", F64)
    n, d = m.shape[0], q0.shape[0]
    L = n + d
    alpha, _, kappa = uparams
    lam = alpha * alpha * (L + kappa) - L
    mA = np.concatenate([m, q0])
    PA = np.zeros((L, L))
    PA[:n, :n], PA[n:, n:] = P, Q
    sp = go._get_sigma_points(mA, PA, lam)
    assert sp.dtype == F64 and sp.shape == (2 * L, L)
    new = np.stack([f(x[:n], x[n:], u) for x in sp])
    f0 = f(m, q0, u)
    den = 2.0 * (lam + L)
    mu = new.sum(axis=0) / den + f0 * (lam / (lam + L))
    dev = new - mu
    # (the centre's term has the state deviation m - m = 0)
    return dev.T @ (sp[:, :n] - m) / den


@pytest.mark.parametrize("uparams", UPARAMS)
@pytest.mark.parametrize("kind", ["lorenz63", "maneuver", "stoch_vol"])
def test_cross_covariance_is_the_state_block_of_the_augmented_one(monkeypatch, kind, uparams):
    rng = np.random.default_rng(5)
    if kind == "lorenz63":
        n, dq, f, u = 3, 3, uc.lorenz63_f(), 0.0
        m = np.array([1.5, -2.0, 20.0])
    elif kind == "maneuver":       # dq = 2 != n = 4: the noise enters through G, its sigma points do not move the state
        n, dq, f, u = 4, 2, uc.maneuver_f(), 1.0
        m = np.array([2.0, 0.3, 3.0, -0.2])
    else:                           # the stochastic-volatility model's dynamics: Phi x + q
        n, dq, f, u = 2, 2, uc.linear_f(0.8 * np.eye(2)), 1.0
        m = rng.normal(size=2)
    P, Q, q0 = _spd(rng, n, 0.05), _spd(rng, dq, 0.1), 0.1 * rng.normal(size=dq)
    X = uc.ucross_f64(m, P, f, u, uparams, q0)
    ref = _textbook_cross(monkeypatch, m, P, f, u, uparams, q0, Q)
    assert X.shape == ref.shape == (n, n)
    assert np.max(np.abs(X - ref)) <= 1e-10 * np.max(np.abs(ref))


@pytest.mark.parametrize("seed", [0, 1])
def test_linear_model_smoother_and_sampler_restatements(seed):
    """On a linear model urts_f64 over ucross_f64 is rts_f64 with F = A, and both are the exact posterior; uffbs_f64 at
    xi = 0 is its mean, and a backward split through the carry is the single pass."""
    T, n, m = 12, 4, 2
    a = cm.random_stable_lgssm(n, m, seed=200 + seed, bias=True)
    ys = cm.simulate_batch(a, 1, T, seed=seed)[0].astype(F64)
    kf = kalman_f64(a, ys, a["m0"], a["P0"])
    X = uc.ucross_stream(kf["m"], kf["P"], uc.linear_f(a["A"], a["G"]), None, (0.5, 2.0, 1.0), a["q0"])
    got = uc.urts_f64(kf["m"], kf["P"], kf["pm"], kf["pP"], X)
    lin = rts_f64(kf["m"], kf["P"], kf["pm"], kf["pP"], a["A"])
    dense = dense_posterior(a, ys, a["m0"], a["P0"])
    for g, l, d in zip(got, lin, dense):
        g, l = g[:d.shape[0]], l[:d.shape[0]]
        assert np.max(np.abs(g - l)) <= 1e-12 * max(1.0, np.max(np.abs(l)))
        assert np.max(np.abs(g - d)) <= 1e-9 * max(1.0, np.max(np.abs(d)))
    assert np.all(np.isnan(got[2][T - 1]))
    x0 = uc.uffbs_f64(kf["m"], kf["P"], kf["pm"], kf["pP"], X, np.zeros((T, n)))
    assert np.max(np.abs(x0 - got[0])) <= 1e-12 * max(1.0, np.max(np.abs(got[0])))
    xi = np.random.default_rng(seed).normal(size=(3, T, n))
    s = 5
    cut = lambda lo, hi: [kf[k][lo:hi] for k in ("m", "P", "pm", "pP")] + [X[lo:hi]]
    full = uc.uffbs_f64(*cut(0, T), xi)
    late = uc.uffbs_f64(*cut(s, T), xi[:, s:])
    early = uc.uffbs_f64(*cut(0, s), xi[:, :s], carry=late[:, 0])
    np.testing.assert_allclose(np.concatenate([early, late], axis=1), full, rtol=1e-12, atol=1e-12)
    l2 = uc.urts_f64(*cut(s, T))
    e2 = uc.urts_f64(*cut(0, s), carry=(l2[0][0], l2[1][0]))
    np.testing.assert_allclose(np.concatenate([e2[0], l2[0]]), got[0], rtol=1e-12, atol=1e-12)


def test_python_argument_checks_need_no_device():
    """uparams with extended=True, more than one component and missing predicted streams are refused before any device work."""
    import torch
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    p = cm.product_params(a)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    post = lambda K, pred: bfa.PosteriorGaussianSumFiltered(None, z(2, K, 5, 4), z(2, K, 5, 4, 4), z(2, K, 5, 4) if pred else None,
                                                            z(2, K, 5, 4, 4) if pred else None)
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    for call in (lambda **kw: bfa.rts_smoother(p, kw.pop("post"), **kw),
                 lambda **kw: bfa.posterior_sample(p, kw.pop("post"), 2, key=np.array([0, 1], np.uint32), **kw)):
        with pytest.raises(ValueError, match="extended=True"):
            call(post=post(1, True), uparams=up, extended=True)
        with pytest.raises(ValueError, match="one component"):
            call(post=post(2, True), uparams=up)
        with pytest.raises(ValueError, match="predicted"):
            call(post=post(1, False), uparams=(1.0, 0.0, 0.0))
    assert callable(bfa.unscented_kalman_smoother) and callable(bfa.unscented_kalman_posterior_sample)
