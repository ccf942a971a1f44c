"""The unscented smoother's contract (csrc/rts_smoother.hpp, RTS_UNSC) restated in float64 for ONE trajectory: the
sigma-point cross-covariance X_t, and the smoother's and the sampler's recursions with X_t supplied in place of F_t P_t.
A plain module: tests/test_unscented_smoother_cpu.py pins it without a GPU, tests/test_unscented_smoother_gpu.py compares
the device against it.  The dynamics below are the registry's formulas (oracle/models.py, which evaluates them in float32)
written for float64 arguments, with the float32 parameter values the device holds."""
import numpy as np

from oracle import models as om
from tests.test_sampler_cpu import psdchol_f64

F64 = np.float64
F32 = np.float32


def _p(v):
    """A parameter as the device holds it: rounded to float32, then exact in float64."""
    return F64(F32(v))


# ---- float64 dynamics f(x, q, u), u a scalar -----------------------------------------------------------------------
def linear_f(A, G=None):
    A = np.asarray(A, F64)
    G = np.eye(A.shape[0]) if G is None else np.asarray(G, F64)
    return lambda x, q, u: A @ x + G @ q


def lorenz63_f(sigma=10.0, rho=28.0, beta=2.667, dt=0.01):
    s, r, b, dt = _p(sigma), _p(rho), _p(beta), _p(dt)

    def f(x, q, u):
        return np.array([dt * s * (x[1] - x[0]) + x[0], dt * (x[0] * r - x[1] - x[0] * x[2]) + x[1],
                         dt * (x[0] * x[1] - b * x[2]) + x[2]], F64) + q
    return f


def lorenz96_f(alpha=1.0, beta=1.0, gamma=8.0, dt=0.01):
    al, be, ga, dt = _p(alpha), _p(beta), _p(gamma), _p(dt)
    return lambda x, q, u: x + dt * (al * (np.roll(x, 1) * (np.roll(x, -1) - np.roll(x, 2))) - be * x + ga) + q


def sine_f(w0):
    w0 = _p(w0)
    return lambda x, q, u: np.sin(w0 * x) + q


def growth_f():
    return lambda x, q, u: x / 2.0 + 25.0 * x / (1.0 + x * x) + u + q


def maneuver_f(dt=0.5, acc=0.5):
    bot = om.ManeuverBOT(dt, acc)
    G = bot.G.astype(F64)

    def f(x, q, u):
        c0, c1, c2 = 0.5 * (u - 1) * (u - 2), -u * (u - 2), 0.5 * u * (u - 1)
        M = c0 * bot._fcv(F64) + c1 * bot._mats(x, bot.acc, F64)[0] + c2 * bot._mats(x, -bot.acc, F64)[0]
        return M @ x + G @ q
    return f


# ---- the contract ------------------------------------------------------------------------------------------------------
def ukf_constants(uparams, L):
    """c = sqrt(L + lambda), w = 1 / (2 (L + lambda)), lambda = alpha^2 (L + kappa) - L."""
    alpha, _, kappa = (F64(v) for v in uparams)
    lam = alpha * alpha * (L + kappa) - L
    return np.sqrt(L + lam), 1.0 / (2.0 * (L + lam))


def sym_sqrt_f64(P):
    """Symmetric square root through the lower triangle (numpy.linalg.eigh), eigenvalues clamped at 0."""
    lam, V = np.linalg.eigh(np.asarray(P, F64))
    return (V * np.sqrt(np.maximum(lam, 0.0))) @ V.T


def ucross_f64(m, P, f, u, uparams, q0):
    """X = w sum_j (f(m + s_j, q0, u) - f(m - s_j, q0, u)) s_j^T with s_j = c R[j, :]: X[k][i] = Cov(x_{t+1,k}, x_{t,i})."""
    m, q0 = np.asarray(m, F64), np.asarray(q0, F64)
    n = m.shape[0]
    c, w = ukf_constants(uparams, n + q0.shape[0])
    R = sym_sqrt_f64(P)
    X = np.zeros((n, n), F64)
    for j in range(n):
        s = c * R[j]
        X += np.outer(f(m + s, q0, u) - f(m - s, q0, u), s)
    return w * X


def ucross_stream(m, P, f, us, uparams, q0):
    """X_t for every step of one trajectory: m (T, n), P (T, n, n), us (T,) inputs or None."""
    T = np.asarray(m).shape[0]
    return np.stack([ucross_f64(m[t], P[t], f, 0.0 if us is None else F64(us[t]), uparams, q0) for t in range(T)])


def urts_f64(m, P, pm, pP, X, carry=None):
    """rts_f64's recursion (tests/test_smoother_cpu.py) with X (T, n, n) in place of F_t P_t."""
    m, P, pm, pP, X = (np.asarray(x, F64) for x in (m, P, pm, pP, X))
    T = m.shape[0]
    ms, Ps, Cs = np.empty_like(m), np.empty_like(P), np.full_like(P, np.nan)
    if carry is None:
        ms[T - 1], Ps[T - 1] = m[T - 1], P[T - 1]
        a, b, t0 = m[T - 1], P[T - 1], T - 2
    else:
        a, b, t0 = np.asarray(carry[0], F64), np.asarray(carry[1], F64), T - 1
    for t in range(t0, -1, -1):
        L = np.linalg.cholesky(pP[t])
        Gt = np.linalg.solve(L.T, np.linalg.solve(L, X[t])).T
        Cs[t] = Gt @ b
        a = m[t] + Gt @ (a - pm[t])
        b = P[t] + Gt @ (b - pP[t]) @ Gt.T
        ms[t], Ps[t] = a, b
    return ms, Ps, Cs


def uffbs_f64(m, P, pm, pP, X, xi, carry=None, pivots=None):
    """ffbs_f64's recursion (tests/test_sampler_cpu.py) with X (T, n, n) in place of F_t P_t; xi (..., T, n).
    ``pivots`` receives one list of (p_j / d_j, kept) per factorised step, last step first."""
    m, P, pm, pP, X, xi = (np.asarray(x, F64) for x in (m, P, pm, pP, X, xi))
    T = m.shape[0]
    x = np.empty(xi.shape, F64)

    def factor(Sig, d):
        rec = [] if pivots is not None else None
        L = psdchol_f64(Sig, d, rec)
        if pivots is not None:
            pivots.append(rec)
        return L

    if carry is None:
        L = factor(P[T - 1], np.diag(P[T - 1]))
        x[..., T - 1, :] = m[T - 1] + xi[..., T - 1, :] @ L.T
        nxt, t0 = x[..., T - 1, :], T - 2
    else:
        nxt, t0 = np.asarray(carry, F64), T - 1
    for t in range(t0, -1, -1):
        Lp = np.linalg.cholesky(pP[t])
        W = np.linalg.solve(Lp, X[t])
        G = np.linalg.solve(Lp.T, W).T
        Sig = np.tril(P[t]) + np.tril(P[t], -1).T - W.T @ W
        L = factor(Sig, np.diag(P[t]))
        nxt = m[t] + (nxt - pm[t]) @ G.T + xi[..., t, :] @ L.T
        x[..., t, :] = nxt
    return x
