"""Float64 statements of the Gaussian-sum backward passes and the models their tests share
(tests/test_gaussian_sum_backward_cpu.py, tests/test_gaussian_sum_smoother_gpu.py).

In ``gaussian_sum_filter`` the K components are independent Kalman chains coupled only through the weight recursion, so the
model is a mixture over the index of the initial component: the smoothed mixture is the per-chain RTS pass with the
filter's FINAL weights, constant in time.  ``gs_smooth_f64`` states that; ``dense_mixture`` is the exact answer for a
linear model with a K-component prior, by dense algebra that shares nothing with the recursions."""
import numpy as np

from tests.test_smoother_cpu import rts_f64, dense_posterior

F32, F64 = np.float32, np.float64


def collapse_f64(w, ms, Ps):
    """Moment match of a mixture with time-constant weights: w (K,), ms (K, T, n), Ps (K, T, n, n) -> (T, n), (T, n, n)."""
    w, ms, Ps = (np.asarray(x, F64) for x in (w, ms, Ps))
    mu = np.einsum("k,kti->ti", w, ms)
    d = ms - mu[None]
    return mu, np.einsum("k,ktij->tij", w, Ps + d[..., :, None] * d[..., None, :])


def gs_smooth_f64(m, P, pm, pP, F, w, carry=None):
    """The Gaussian-sum smoother for ONE trajectory in float64: streams (K, T, ...), F (n, n), (T, n, n) or a function
    k -> Jacobians of chain k, weights w (K,).  Returns the per-chain smoothed means, covariances, cross-covariances
    (``rts_f64`` on every chain) and the collapsed mean and covariance."""
    K = np.asarray(m).shape[0]
    out = [rts_f64(m[k], P[k], pm[k], pP[k], F(k) if callable(F) else F,
                   None if carry is None else (carry[0][k], carry[1][k])) for k in range(K)]
    ms, Ps, Cs = (np.stack([o[i] for o in out]) for i in range(3))
    mu, Sigma = collapse_f64(w, ms, Ps)
    return ms, Ps, Cs, mu, Sigma


def kalman_loglik_f64(a, ys, m_init, P_init):
    """Jitter-free float64 Kalman filter (update -> predict) of ONE chain: the streams of ``kalman_f64`` and log p(y_{0:T-1})."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    mp, Pp = np.asarray(m_init, F64), np.asarray(P_init, F64)
    out = {k: [] for k in ("m", "P", "pm", "pP")}
    ll = 0.0
    for t in range(ys.shape[0]):
        S = H @ Pp @ H.T + D @ R @ D.T
        e = ys[t] - H @ mp - D @ r0
        ll += -0.5 * (e @ np.linalg.solve(S, e) + np.linalg.slogdet(S)[1] + e.size * np.log(2 * np.pi))
        K = np.linalg.solve(S, H @ Pp).T
        m = mp + K @ e
        P = Pp - K @ S @ K.T
        mp = A @ m + G @ q0
        Pp = A @ P @ A.T + G @ Q @ G.T
        for k, v in (("m", m), ("P", P), ("pm", mp), ("pP", Pp)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, ll


def dense_evidence(a, ys, m_init, P_init):
    """log p(y_{0:T-1}) of the linear model from the dense Gaussian of the stacked observations (no recursion)."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    T, n, m = ys.shape[0], A.shape[0], H.shape[0]
    mean = np.zeros((T, n))
    cov = np.zeros((T, n, T, n))
    mean[0], cov[0, :, 0, :] = np.asarray(m_init, F64), np.asarray(P_init, F64)
    for t in range(1, T):
        mean[t] = A @ mean[t - 1] + G @ q0
        cov[t, :, t, :] = A @ cov[t - 1, :, t - 1, :] @ A.T + G @ Q @ G.T
        for s in range(t):
            cov[t, :, s, :] = A @ cov[t - 1, :, s, :]
            cov[s, :, t, :] = cov[t, :, s, :].T
    Hs = np.kron(np.eye(T), H)
    Sy = Hs @ cov.reshape(T * n, T * n) @ Hs.T + np.kron(np.eye(T), D @ R @ D.T)
    e = (ys - mean @ H.T - D @ r0).reshape(-1)
    return -0.5 * (e @ np.linalg.solve(Sy, e) + np.linalg.slogdet(Sy)[1] + e.size * np.log(2 * np.pi))


def dense_mixture(a, ys, m_inits, P_init, w0=None):
    """Exact smoothed mixture of the linear model with prior sum_k w0_k N(m_inits[k], P_init) on x_0: the weights
    w_k ~ w0_k p(y | k) from the dense evidences, per-component marginals from ``dense_posterior``, and their moment
    match.  Returns w (K,), means (K, T, n), covariances (K, T, n, n), collapsed mean (T, n) and covariance (T, n, n)."""
    K = len(m_inits)
    w0 = np.full(K, 1.0 / K) if w0 is None else np.asarray(w0, F64)
    le = np.array([dense_evidence(a, ys, m_inits[k], P_init) for k in range(K)])
    w = w0 * np.exp(le - le.max())
    w /= w.sum()
    parts = [dense_posterior(a, ys, m_inits[k], P_init) for k in range(K)]
    ms, Ps = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    mu, Sigma = collapse_f64(w, ms, Ps)
    return w, ms, Ps, mu, Sigma


def mixture_case(n, m, K, T, seed):
    """A stable linear model, one observed trajectory and K initial means m0 + chol(P0) xi."""
    from tests import common as cm
    a = cm.random_stable_lgssm(n, m, seed=seed, bias=True)
    ys = cm.simulate_batch(a, 1, T, seed=seed + 1)[0].astype(F64)
    rng = np.random.default_rng(seed + 2)
    m_inits = a["m0"].astype(F64) + rng.normal(size=(K, n)) @ np.linalg.cholesky(a["P0"].astype(F64)).T
    return a, ys, m_inits


def draw_components_f32(w, v):
    """The component draw of the Gaussian-sum sampler, restated in NumPy float32: w (B, K) weights, v (B, S) uniforms in
    [0, 1).  c_j = the inclusive cumulative sum of w[b, :j+1] by sequential float32 adds; z = the smallest j with
    c_j > v c_{K-1}, clamped to K-1; -1 where c_{K-1} is not finite or not positive."""
    w, v = np.asarray(w, F32), np.asarray(v, F32)
    B, K = w.shape
    z = np.empty(v.shape, np.int32)
    for b in range(B):
        c = np.empty(K, F32)
        acc = F32(0.0)
        for j in range(K):
            with np.errstate(all="ignore"):
                acc = F32(acc + w[b, j])
            c[j] = acc
        tot = c[K - 1]
        if not np.isfinite(tot) or not tot > 0:
            z[b] = -1
            continue
        for s in range(v.shape[1]):
            thr = F32(v[b, s] * tot)
            hit = np.nonzero(c > thr)[0]
            z[b, s] = hit[0] if hit.size else K - 1
    return z
