"""Cases for the Kalman filter with missing observations (``kalman_filter(..., missing="nan")``,
``bf_kalman_filter_missing_f32``): a float64 NumPy reference written from the contract, a float64 RTS pass over that reference's
own streams, the gap patterns, and the models.  Shared by tests/test_kalman_missing_cpu.py and tests/test_kalman_missing_gpu.py.

The contract.  At step t of a trajectory let o be the components whose observation is not NaN.  The update is
``_condition_on`` on the sub-model of those rows -- H[o, :], (D r0)[o], (D R D^T)[o, o], the reference's +1e-6 on EVERY entry of
the reduced S_oo in the gain solve --, the log-likelihood is log N(v_o; 0, S_oo) with |o| in the log 2 pi term and no jitter.
o empty: m+ = m-, P+ = P-, log-likelihood 0.  The weight of the single component is 1 while everything is finite.  The predict
step always runs.  The reference SELECTS rows per step (it never builds the m x m embedding the kernel uses)."""
import functools

import numpy as np

from tests import common as cm

F32, F64 = np.float32, np.float64
STREAMS = ("weights", "means", "covariances", "predicted_means", "predicted_covariances")
LOG2PI = float(np.log(2.0 * np.pi))

# (n, m): one lane per trajectory, two lanes, two lanes with a padding lane (n = 3), four lanes
SHAPES = [(2, 1), (4, 2), (3, 3), (8, 4)]
BATCHES = (1, 37)      # 37: a partial wave at every lane count, and with it the tail launch of the staged route
HORIZONS = (19, 64)    # 19: no multiple of 4 (scalar weight rows) nor of the observation block (8 / m steps)
FORECAST = 5           # the last steps of every gapped trajectory are unobserved
FULL, NONE, NO_COMP1 = 1, 2, 3   # trajectories of a batch with a fixed pattern (those that exist at the batch size)


def model(n, m, tv=False, T=None):
    """Random stable A, well-conditioned Q, R, P0 (R = Lr Lr^T + 0.1 I is of the order of H P H^T: every reduced S_oo is
    benign), biases on.  ``tv``: per-step Q_t, R_t tables of ``T`` steps."""
    a = dict(cm.random_stable_lgssm(n, m, seed=100 * n + m, bias=True))
    if tv:
        rng = np.random.default_rng(7)
        a["Q"] = (a["Q"][None] * (1 + rng.random((T, 1, 1)))).astype(F32)
        a["R"] = (a["R"][None] * (1 + rng.random((T, 1, 1)))).astype(F32)
    return a


def row_reduced(a, keep):
    """The model that observes only the components ``keep``: rows of H and D; r0, R stay."""
    r = dict(a)
    r["H"], r["D"] = np.ascontiguousarray(a["H"][keep]), np.ascontiguousarray(a["D"][keep])
    return r


def observed_mask(B, T, m, seed=11, wholly_missing_at=None):
    """(B, T, m) bool, true = observed.  Every trajectory but the fixed ones: about 30 % of the entries missing
    independently, step 0 missing, one wholly missing step (``wholly_missing_at``, default T // 2), the last FORECAST steps
    missing.  Trajectory FULL is fully observed, NONE has nothing observed, NO_COMP1 lacks component 1 and nothing else (at
    m = 1: component 0, which leaves nothing)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((B, T, m)) >= 0.3
    mask[:, 0] = False
    mask[:, T // 2 if wholly_missing_at is None else wholly_missing_at] = False
    mask[:, T - FORECAST:] = False
    if B > FULL:
        mask[FULL] = True
    if B > NONE:
        mask[NONE] = False
    if B > NO_COMP1:
        mask[NO_COMP1] = True
        mask[NO_COMP1, :, min(1, m - 1)] = False
    return mask


def gapped(ys, mask):
    """A float32 copy of ``ys`` with NaN where ``mask`` is false."""
    out = np.array(ys, dtype=F32)
    out[~np.broadcast_to(mask, out.shape)] = np.nan
    return out


def kalman_missing_f64(a, ys, m_init, P_init):
    """The contract in float64 for ONE trajectory ys (T, m), NaN = missing.  Returns dict of the five streams (T, ...), the
    log-likelihood (T,), and the carry-out (w, m-, P-)."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    ys = np.asarray(ys, F64)
    T = ys.shape[0]
    mp, Pp, w = np.asarray(m_init, F64).copy(), np.asarray(P_init, F64).copy(), 1.0
    out = {k: [] for k in STREAMS + ("loglik",)}
    for t in range(T):
        Qt = Q[t] if Q.ndim == 3 else Q
        Rt = R[t] if R.ndim == 3 else R
        o = ~np.isnan(ys[t])
        if o.any():
            Ho = H[o]
            S = (D @ Rt @ D.T)[np.ix_(o, o)] + Ho @ Pp @ Ho.T
            K = np.linalg.solve(S + 1e-6, Ho @ Pp).T            # the 1e-6 on every entry of the REDUCED matrix
            v = ys[t, o] - Ho @ mp - (D @ r0)[o]
            m = mp + K @ v
            P = Pp - K @ S @ K.T
            L = np.linalg.cholesky(S)
            z = np.linalg.solve(L, v)
            ll = -0.5 * float(z @ z) - 0.5 * int(o.sum()) * LOG2PI - float(np.sum(np.log(np.diag(L))))
        else:
            m, P, ll = mp.copy(), Pp.copy(), 0.0
        w = 1.0 if (np.isfinite(ll) and np.isfinite(w) and w != 0.0) else np.nan    # reweight of one component
        mp = A @ m + G @ q0
        Pp = A @ P @ A.T + G @ Qt @ G.T
        for k, x in zip(STREAMS + ("loglik",), (w, m, P, mp, Pp, ll)):
            out[k].append(np.array(x, F64))
    res = {k: np.stack(x) for k, x in out.items()}
    res["carry"] = (w, mp, Pp)
    return res


def rts_f64(a, streams):
    """Float64 RTS pass over the streams of :func:`kalman_missing_f64` (one trajectory): the backward recursion reads no
    observation, so gaps change nothing in it.  Returns smoothed means (T, n) and covariances (T, n, n)."""
    A = np.asarray(a["A"], F64)
    m, P, pm, pP = (streams[k] for k in ("means", "covariances", "predicted_means", "predicted_covariances"))
    T = m.shape[0]
    ms, Ps = m.copy(), P.copy()
    for t in range(T - 2, -1, -1):
        Gt = np.linalg.solve(pP[t], A @ P[t]).T
        ms[t] = m[t] + Gt @ (ms[t + 1] - pm[t])
        Ps[t] = P[t] + Gt @ (Ps[t + 1] - pP[t]) @ Gt.T
    return ms, Ps


def batch_reference(a, ys, init_means):
    """:func:`kalman_missing_f64` trajectory by trajectory from ``init_means`` (B, n) and P0: the streams and the
    log-likelihood shaped (B, 1, T, ...) like the product's, the carry-out (B, 1), (B, 1, n), (B, 1, n, n), and the smoothed
    means / covariances of :func:`rts_f64`."""
    per = [kalman_missing_f64(a, ys[b], init_means[b], a["P0"]) for b in range(ys.shape[0])]
    ref = {k: np.stack([p[k] for p in per])[:, None] for k in STREAMS + ("loglik",)}
    ref["carry"] = tuple(np.stack([np.asarray(p["carry"][i], F64) for p in per])[:, None] for i in range(3))
    sm = [rts_f64(a, p) for p in per]
    ref["smoothed_means"] = np.stack([s[0] for s in sm])[:, None]
    ref["smoothed_covariances"] = np.stack([s[1] for s in sm])[:, None]
    return ref


def _frozen(d):
    for v in d.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(n, m, B, T, tv=False):
    """One test case, computed once and shared (no test writes into it): the model, the complete float32 emissions, the mask, the gapped
    emissions, the initial means and the float64 reference of the gapped run."""
    a = model(n, m, tv, T)
    ys = cm.simulate_batch(model(n, m), B, T, seed=3)    # (drawn from the constant model: the filter's tables need not match)
    mask = observed_mask(B, T, m)
    init = (np.tile(a["m0"], (B, 1)) + 0.3 * np.random.default_rng(5).normal(size=(B, n))).astype(F32)
    yg = gapped(ys, mask)
    # (the reference is frozen; the model and the inputs are handed to torch as they are, which wants writable arrays)
    return dict(a=a, ys=ys, mask=mask, gapped=yg, init=init, ref=_frozen(batch_reference(a, yg, init)))
