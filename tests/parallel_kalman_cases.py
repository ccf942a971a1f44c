"""Yardsticks and cases of the parallel-in-time Kalman filter's tests (csrc/kf_pscan.hpp), float64 NumPy throughout.

* :func:`kalman_f64` -- the recursion of ``kalman_filter``: update -> predict, gain from a solve with S + 1e-6 on every entry
  (``jitter=0`` gives the textbook filter), un-jittered S in P - K S K^T and in the log-likelihood; batched over trajectories.
* :func:`element`, :func:`combine`, :func:`apply_span` -- the filtering element of one step, the associative combination of
  two spans and a span applied to a filtered state, restated from the header.
* :func:`model`, :func:`case` -- models from ``tests/common.py`` and data from ``cm.simulate_batch``.
"""
import functools

import numpy as np

from tests import common as cm

STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")


def terms(a):
    """A, H, Qb = G Q G^T, Rb = D R D^T, u = G q0, d = D r0 in float64 from the model's float32 arrays."""
    A, G, H, D, Q, R, q0, r0 = (np.asarray(a[k], np.float64) for k in ("A", "G", "H", "D", "Q", "R", "q0", "r0"))
    return A, H, G @ Q @ G.T, D @ R @ D.T, G @ q0, D @ r0


def kalman_f64(a, ys, m0, P0, jitter=1e-6):
    """ys (B, T, m), m0 (B, n), P0 (B, n, n) or (n, n): dict of (B, 1, T, ...) arrays, keys STREAMS + loglik."""
    A, H, Qb, Rb, u, d = terms(a)
    ys = np.asarray(ys, np.float64)
    B, T, mdim = ys.shape
    n = A.shape[0]
    m = np.array(np.broadcast_to(np.asarray(m0, np.float64), (B, n)))
    P = np.array(np.broadcast_to(np.asarray(P0, np.float64), (B, n, n)))
    out = {k: np.empty((B, 1, T) + ((n,) if "means" in k else (n, n))) for k in STREAMS}
    out["loglik"] = np.empty((B, 1, T))
    for t in range(T):
        v = ys[:, t] - (m @ H.T + d)
        HP = H @ P
        S = HP @ H.T + Rb
        K = np.swapaxes(np.linalg.solve(S + jitter, HP), 1, 2)
        P = P - K @ S @ np.swapaxes(K, 1, 2)
        m = m + np.einsum("bia,ba->bi", K, v)
        L = np.linalg.cholesky(S)
        z = np.linalg.solve(L, v[..., None])[..., 0]
        out["loglik"][:, 0, t] = (-0.5 * np.sum(z * z, -1) - 0.5 * mdim * np.log(2 * np.pi)
                                  - np.sum(np.log(np.diagonal(L, axis1=1, axis2=2)), -1))
        out["means"][:, 0, t], out["covariances"][:, 0, t] = m, P
        m = m @ A.T + u
        P = A @ P @ A.T + Qb
        out["predicted_means"][:, 0, t], out["predicted_covariances"][:, 0, t] = m, P
    return out


def element(a, y):
    """(A_e, b_e, C_e, eta_e, J_e) of one step with observation y."""
    A, H, Qb, Rb, u, d = terms(a)
    n = A.shape[0]
    S = H @ Qb @ H.T + Rb
    Si = np.linalg.inv(S)
    K = Qb @ H.T @ Si
    v = np.asarray(y, np.float64) - H @ u - d
    IKH = np.eye(n) - K @ H
    W = A.T @ H.T @ Si
    return IKH @ A, u + K @ v, IKH @ Qb, W @ v, W @ H @ A


def _sym(X):
    return 0.5 * (X + X.T)


def combine(si, sj):
    """The earlier span si followed by the later span sj."""
    Ai, bi, Ci, ei, Ji = si
    Aj, bj, Cj, ej, Jj = sj
    n = Ai.shape[0]
    M1 = np.eye(n) + Ci @ Jj
    M2 = np.eye(n) + Jj @ Ci
    A = Aj @ np.linalg.solve(M1, Ai)
    b = Aj @ np.linalg.solve(M1, bi + Ci @ ej) + bj
    C = Aj @ np.linalg.solve(M1, Ci) @ Aj.T + Cj
    e = Ai.T @ np.linalg.solve(M2, ej - Jj @ bi) + ei
    J = Ai.T @ np.linalg.solve(M2, Jj @ Ai) + Ji
    return A, b, _sym(C), e, _sym(J)


def apply_span(s, m, P):
    """The span s applied to the filtered state (m, P)."""
    A, b, C, e, J = s
    M = np.eye(A.shape[0]) + P @ J
    return A @ np.linalg.solve(M, m + P @ e) + b, _sym(A @ np.linalg.solve(M, P) @ A.T + C)


@functools.lru_cache(maxsize=None)
def model(name):
    """The named model's arrays: 'n x m' -> cm.random_stable_lgssm(n, m), 'bias' -> (4, 2) with noise biases and dq = 2 < n,
    'cv' -> the constant-velocity model (unit eigenvalues, singular G Q G^T)."""
    if name == "cv":
        return cm.cv_model_arrays()
    if name == "bias":
        return cm.random_stable_lgssm(4, 2, seed=46, dq=2, bias=True)
    n, m = (int(v) for v in name.split("x"))
    return cm.random_stable_lgssm(n, m, seed=40 + 7 * n + m)


@functools.lru_cache(maxsize=None)
def case(name, B, T):
    """(arrays, ys (B, T, m) float32, initial means (B, n) float32, the jittered float64 yardstick); shared, never modified.
    The filter is causal: the first T' steps of the yardstick are the yardstick of ys[:, :T']."""
    a = model(name)
    ys = cm.simulate_batch(a, B, T, seed=1000 + B)
    rng = np.random.default_rng(5)
    init = (a["m0"] + 0.1 * rng.normal(size=(B, a["m0"].shape[0]))).astype(np.float32)
    ref = kalman_f64(a, ys, init, a["P0"])
    for v in ref.values():
        v.setflags(write=False)
    ys.setflags(write=False)
    return a, ys, init, ref
