"""The Lorenz-96 n = 12 case of tests/test_backward_contract_gpu.py, no GPU: is the families' tolerance (1e-5, tests/test_smoother_gpu.py
and tests/test_sampler_gpu.py) a fair demand on ANY float32 evaluation of the backward recursions at this model?

A float32 NumPy restatement of the smoothing recursion (csrc/rts_smoother.hpp) and of the sampling recursion
(csrc/ffbs_sampler.hpp) runs on the float32 oracle's filtered streams (oracle/gaussfilt_oracle.py: gaussian_sum_filter with one
component, the extended Kalman filter) and must stay within ONE TENTH of that tolerance of the float64 oracles ``rts_f64`` /
``ffbs_f64``; every P- must be positive definite in float32.  The setting (``L96``) is what the GPU test imports.

Why this setting.  n = 12 is the smallest even n > 8 whose n^2 = 144 elements make the 64-lane loops of the run-time-dimension
kernels wrap (twice) and whose rows are padded in LDS.  dt = 0.01 is the model's own step.  Q = 0.1 I against P0 = I keeps P- well
conditioned over the T = 12 steps: the unobserved odd states are only reached through the Jacobian's off-diagonals, dt-small, so
their variance grows by about Q per step while the observed ones settle near R = 0.1 I, and the solves against P- lose about one
digit.  The test prints and records the float32 errors and the largest cond(P-) it measures."""
import functools

import numpy as np

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import common as cm
from tests.test_smoother_cpu import rts_f64
from tests.test_sampler_cpu import ffbs_f64, TAU

F32 = np.float32
FAMILY_TOL = 1e-5       # tests/test_smoother_gpu.py: _check(tol=1e-5); tests/test_sampler_gpu.py: TOL
L96 = dict(n=12, dt=0.01, q=1e-1, r=1e-1, B=5, T=12, S=5, m0=8.0, spread=0.5)


def l96_oracle_params():
    n = L96["n"]
    m = n // 2
    return go.ParamsNLSSM((L96["m0"] * np.ones(n)).astype(F32), np.eye(n, dtype=F32), om.Lorenz96(n, dt=L96["dt"]), np.zeros(n, F32),
                          (L96["q"] * np.eye(n)).astype(F32), om.PickEven(n), np.zeros(m, F32), (L96["r"] * np.eye(m)).astype(F32))


def l96_product_params():
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    po = l96_oracle_params()
    n = L96["n"]
    return bfa.ParamsNLSSM(po.initial_mean, po.initial_covariance, nl.lorenz96(n, dt=L96["dt"]), po.dynamics_noise_bias,
                           po.dynamics_noise_covariance, nl.pick_even(n), po.emission_noise_bias, po.emission_noise_covariance)


@functools.lru_cache(maxsize=None)
def l96_data():
    """(emissions (B, T, m), initial means (B, 1, n)), float32, read-only."""
    po = l96_oracle_params()
    B, T, n = L96["B"], L96["T"], L96["n"]
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(40 + b), T, None)[1] for b in range(B)]).astype(F32)
    init = (po.initial_mean + L96["spread"] * np.random.default_rng(96).normal(size=(B, 1, n))).astype(F32)
    ys.setflags(write=False)
    init.setflags(write=False)
    return ys, init


def l96_jacobians(m):
    """F_t at the filtered means m (T, n), as the filter's predict used it (q = 0, no input)."""
    f = om.Lorenz96(L96["n"], dt=L96["dt"])
    z = np.zeros(L96["n"], F32)
    return np.stack([f.jac_x(np.asarray(m[t], F32), z, np.zeros(1, F32)) for t in range(m.shape[0])])


# ---- float32 restatements -------------------------------------------------------------------------------------------------
def _chol32(A):
    """Lower Cholesky factor, left-looking, every operation rounded to float32; NaN for a non-positive pivot."""
    n = A.shape[0]
    L = np.zeros((n, n), F32)
    for j in range(n):
        d = F32(A[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j, j] = np.sqrt(d) if d > 0 else F32(np.nan)
        for i in range(j + 1, n):
            L[i, j] = F32(A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def _solve_lower32(L, X):
    n = L.shape[0]
    W = np.zeros_like(X, dtype=F32)
    for i in range(n):
        W[i] = (X[i] - L[i, :i] @ W[:i]).astype(F32) / L[i, i]
    return W


def _solve_upper32(L, W):
    """L^T X = W."""
    n = L.shape[0]
    X = np.zeros_like(W, dtype=F32)
    for i in range(n - 1, -1, -1):
        X[i] = (W[i] - L[i + 1:, i] @ X[i + 1:]).astype(F32) / L[i, i]
    return X


def rts_f32(m, P, pm, pP, F):
    m, P, pm, pP, F = (np.asarray(x, F32) for x in (m, P, pm, pP, F))
    T = m.shape[0]
    ms, Ps, Cs = m.copy(), P.copy(), np.full_like(P, np.nan)
    for t in range(T - 2, -1, -1):
        L = _chol32(pP[t])
        X = _solve_upper32(L, _solve_lower32(L, F[t] @ P[t]))
        G = X.T
        Cs[t] = G @ Ps[t + 1]
        ms[t] = m[t] + G @ (ms[t + 1] - pm[t])
        Ps[t] = P[t] + (G @ (Ps[t + 1] - pP[t])) @ G.T
    assert ms.dtype == F32 and Ps.dtype == F32 and Cs.dtype == F32
    return ms, Ps, Cs


def _psdchol32(S, d):
    n = S.shape[0]
    L = np.zeros((n, n), F32)
    for j in range(n):
        p = F32(S[j, j] - np.dot(L[j, :j], L[j, :j]))
        if p > F32(TAU) * d[j]:
            L[j, j] = np.sqrt(p)
            for i in range(j + 1, n):
                L[i, j] = F32(S[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def ffbs_f32(m, P, pm, pP, F, xi):
    m, P, pm, pP, F, xi = (np.asarray(x, F32) for x in (m, P, pm, pP, F, xi))
    T = m.shape[0]
    x = np.empty(xi.shape, F32)
    x[:, T - 1] = m[T - 1] + xi[:, T - 1] @ _psdchol32(P[T - 1], np.diag(P[T - 1])).T
    for t in range(T - 2, -1, -1):
        Lp = _chol32(pP[t])
        W = _solve_lower32(Lp, F[t] @ P[t])
        G = _solve_upper32(Lp, W).T
        Sig = (np.tril(P[t]) + np.tril(P[t], -1).T - W.T @ W).astype(F32)
        L = _psdchol32(Sig, np.diag(P[t]))
        x[:, t] = m[t] + (x[:, t + 1] - pm[t]) @ G.T + xi[:, t] @ L.T
    assert x.dtype == F32
    return x


def sampler_err(x, ref, P):
    """tests/test_sampler_gpu.py: _err."""
    scale = max(1.0, float(np.max(np.abs(ref))), float(np.sqrt(np.max(np.diagonal(P, axis1=-2, axis2=-1)))))
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref)) / scale)


def test_lorenz96_n12_float32_recursions_have_headroom_under_the_family_tolerance():
    po = l96_oracle_params()
    ys, init = l96_data()
    B, T, n, S = L96["B"], L96["T"], L96["n"], L96["S"]
    assert n > 8 and n * n > 64
    xi = np.random.default_rng(12).normal(size=(B, S, T, n)).astype(F32)
    worst_s, worst_x, worst_cond = 0.0, 0.0, 0.0
    for b in range(B):
        post = go.gaussian_sum_filter(po, ys[b], 1, initial_means=init[b])
        m, P, pm, pP = (np.asarray(getattr(post, k))[0] for k in ("means", "covariances", "predicted_means", "predicted_covariances"))
        assert m.dtype == F32 and np.all(np.isfinite(P))
        for t in range(T):                       # every P- positive definite in float32 (the GPU takes its Cholesky factor unjittered)
            assert np.all(np.isfinite(_chol32(pP[t]))), (b, t)
            worst_cond = max(worst_cond, float(np.linalg.cond(pP[t].astype(np.float64))))
        F = l96_jacobians(m)
        ref = rts_f64(m, P, pm, pP, F)
        got = rts_f32(m, P, pm, pP, F)
        e = (cm.rel_err(got[0], ref[0]), cm.rel_err(got[1], ref[1]), cm.rel_err(got[2][:-1], ref[2][:-1]))
        xr = ffbs_f64(m, P, pm, pP, F, xi[b])
        ex = sampler_err(ffbs_f32(m, P, pm, pP, F, xi[b]), xr, P)
        print(f"lorenz96 n = {n}, trajectory {b}: float32 smoother {max(e):.2e} (means, covariances, cross {e}), sampler {ex:.2e}")
        worst_s, worst_x = max(worst_s, max(e)), max(worst_x, ex)
    print(f"lorenz96 n = {n}: worst float32 smoother {worst_s:.2e}, sampler {worst_x:.2e}, largest cond(P-) {worst_cond:.1f}; "
          f"allowed {FAMILY_TOL / 10:.0e}")
    cm.record("backward_contract_l96_fp32_headroom", smoother=worst_s, sampler=worst_x, cond=worst_cond)
    assert worst_s <= FAMILY_TOL / 10, worst_s
    assert worst_x <= FAMILY_TOL / 10, worst_x
