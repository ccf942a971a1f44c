"""Cases and yardsticks of ``parallel_kalman_filter(..., missing="nan")`` (``bf_kalman_filter_pscan_missing_f32``), float64
NumPy throughout, built on tests/kalman_missing_cases.py (the contract, the masks) and tests/parallel_kalman_cases.py (the
models, the combination, a span applied to a state).  Shared by tests/test_parallel_kalman_missing_cpu.py and
tests/test_parallel_kalman_missing_gpu.py.

Two yardsticks.

1. The contract: :func:`tests.kalman_missing_cases.kalman_missing_f64`, the serial filter on the observed rows of each step
   with the reference's 1e-6 jitter at every step.
2. The scheme (:func:`scheme_f64`): what the three launches compute, in float64.  Block 0 runs by the contract; the filtered
   state at the end of block k >= 1 is block k's per-pattern elements (jitter-free), combined left to right and applied to the
   filtered state at the end of block k - 1; its prediction starts block k + 1, inside which the contract runs.  With
   T <= block the scheme is the contract.

The two differ by the jitter of the steps the elements stand for, and by nothing else (:func:`jitter_gap`).
"""
import functools

import numpy as np

from tests import common as cm
from tests import kalman_missing_cases as kc
from tests import parallel_kalman_cases as pk

F64 = np.float64
B, TMAX = 6, 1000
MODELS = ["1x1", "2x2", "3x1", "4x2", "4x4", "bias", "5x2", "6x3"]
# (T, block): 76 blocks -- across a wave, ragged last block of 1; 16 blocks, ragged; three blocks, one of them a middle block;
# two blocks (a scan over a single span, no middle block); one block; one step
SHAPES = [(301, 4), (1000, 64), (12, 4), (8, 4), (37, 64), (1, 64)]
STREAMS = kc.STREAMS + ("loglik",)
LONG_GAP = (4, 40, 140)   # trajectory 4 is unobserved over steps 40 ... 139: 25 whole blocks at block = 4
TOL = 1e-5                # the project's standing fp32 tolerance


def pattern_element(a, obs):
    """(A_e, C_e, J_e, K, W) of a step that observes the components ``obs`` (bool, m): K and W are n x m with zero columns for
    the missing components; nothing observed gives (A, Qb, 0, 0, 0).  No jitter."""
    A, H, Qb, Rb, u, d = pk.terms(a)
    n, m = A.shape[0], H.shape[0]
    obs = np.asarray(obs, bool)
    K, W = np.zeros((n, m)), np.zeros((n, m))
    if obs.any():
        Ho = H[obs]
        Si = np.linalg.inv(Ho @ Qb @ Ho.T + Rb[np.ix_(obs, obs)])
        K[:, obs] = Qb @ Ho.T @ Si
        W[:, obs] = A.T @ Ho.T @ Si
    IKH = np.eye(n) - K @ H
    return IKH @ A, IKH @ Qb, W @ H @ A, K, W


def element(a, y):
    """The filtering element (A_e, b_e, C_e, eta_e, J_e) of one step with observation ``y`` (m,), NaN = not observed."""
    A, H, Qb, Rb, u, d = pk.terms(a)
    y = np.asarray(y, F64)
    obs = ~np.isnan(y)
    Ae, Ce, Je, K, W = pattern_element(a, obs)
    v = np.where(obs, y - H @ u - d, 0.0)
    return Ae, u + K @ v, Ce, W @ v, Je


def fold(a, ys):
    """The elements of the steps ``ys`` (L, m) combined left to right: the aggregate of one block."""
    s = element(a, ys[0])
    for y in ys[1:]:
        s = pk.combine(s, element(a, y))
    return s


def gapped_filter_f64(a, ys, m_init, P_init):
    """The jitter-free gapped filter of one trajectory, step by step: filtered means (T, n) and covariances (T, n, n)."""
    A, H, Qb, Rb, u, d = pk.terms(a)
    mp, Pp = np.asarray(m_init, F64), np.asarray(P_init, F64)
    ms, Ps = [], []
    for y in np.asarray(ys, F64):
        o = ~np.isnan(y)
        m, P = mp, Pp
        if o.any():
            Ho = H[o]
            K = np.linalg.solve(Ho @ Pp @ Ho.T + Rb[np.ix_(o, o)], Ho @ Pp).T
            m, P = mp + K @ (y[o] - Ho @ mp - d[o]), Pp - K @ Ho @ Pp
        ms.append(m)
        Ps.append(P)
        mp, Pp = A @ m + u, A @ P @ A.T + Qb
    return np.stack(ms), np.stack(Ps)


def scheme_f64(a, ys, m_init, P_init, block):
    """Yardstick 2 for ONE trajectory ys (T, m): the dict of :func:`tests.kalman_missing_cases.kalman_missing_f64`."""
    A, H, Qb, Rb, u, d = pk.terms(a)
    T = ys.shape[0]
    first = kc.kalman_missing_f64(a, ys[:block], m_init, P_init)
    if T <= block:
        return first
    parts = [first]
    m, P = first["means"][-1], first["covariances"][-1]       # filtered at the end of block 0
    NB = -(-T // block)
    for k in range(1, NB):
        if k > 1:
            m, P = pk.apply_span(fold(a, ys[(k - 1) * block:k * block]), m, P)
        parts.append(kc.kalman_missing_f64(a, ys[k * block:(k + 1) * block], A @ m + u, A @ P @ A.T + Qb))
    out = {key: np.concatenate([p[key] for p in parts]) for key in STREAMS}
    out["carry"] = parts[-1]["carry"]
    return out


def mask_for(T, m):
    """The gap pattern of the GPU cases: tests.kalman_missing_cases.observed_mask (30 % of the entries missing, step 0 and one
    whole step missing, a forecast tail, trajectories FULL / NONE / NO_COMP1) plus LONG_GAP where the series is long enough."""
    mask = kc.observed_mask(B, T, m, wholly_missing_at=150 if T > 150 else None)
    b, t0, t1 = LONG_GAP
    if T > t1:
        mask[b, t0:t1] = False
    return mask


def _batched(per):
    out = {key: np.stack([p[key] for p in per])[:, None] for key in STREAMS}
    out["carry"] = tuple(np.stack([np.asarray(p["carry"][i], F64) for p in per])[:, None] for i in range(3))
    return kc._frozen(out)


@functools.lru_cache(maxsize=None)
def case(name, T, block):
    """One GPU case, computed once and shared (no test writes into it): the model, the complete float32 emissions (B, T, m),
    the mask, the gapped emissions, the initial means, and both yardsticks shaped (B, 1, T, ...) like the product's."""
    a, ys, init, _ = pk.case(name, B, TMAX)
    ys = np.array(ys[:, :T])
    mask = mask_for(T, ys.shape[2])
    yg = kc.gapped(ys, mask)
    contract = _batched([kc.kalman_missing_f64(a, yg[b], init[b], a["P0"]) for b in range(B)])
    scheme = _batched([scheme_f64(a, yg[b], init[b], a["P0"], block) for b in range(B)])
    # (the yardsticks are frozen; the inputs are handed to torch as they are, which wants writable arrays)
    return dict(a=a, ys=ys, mask=mask, gapped=yg, init=init, contract=contract, scheme=scheme)


def errors(got, ref, key):
    """{"rel": rel_err, and on the covariance streams "elem": elem_err(ev=2)} of one stream."""
    out = {"rel": cm.rel_err(got, ref)}
    if "covariances" in key:
        out["elem"] = cm.elem_err(got, ref, ev=2)
    return out


def jitter_gap(name, T, block):
    """Per stream, the distance of the scheme from the contract in float64: what the jitter of the folded steps is worth."""
    c = case(name, T, block)
    return {key: errors(c["scheme"][key], c["contract"][key], key) for key in STREAMS if key != "weights"}


def backward_samples_f64(a, streams, noise):
    """Float64 backward sampling over the streams of one trajectory (the dict of kalman_missing_f64) with the standard normals
    ``noise`` (S, T, n): x_T = m_T + chol(P_T) z_T, x_t = m_t + G_t (x_{t+1} - m-_{t+1}) + chol(P_t - G_t P-_{t+1} G_t^T) z_t with
    G_t = P_t A^T (P-_{t+1})^-1.  Used on both yardsticks with the same noise: the distance between the two sets of samples is
    what the jitter of the folded steps is worth downstream."""
    A = np.asarray(a["A"], F64)
    m, P, pm, pP = (streams[k] for k in ("means", "covariances", "predicted_means", "predicted_covariances"))
    S, T, n = noise.shape
    xs = np.empty((S, T, n))
    xs[:, -1] = m[-1] + noise[:, -1] @ np.linalg.cholesky(P[-1]).T
    for t in range(T - 2, -1, -1):
        G = np.linalg.solve(pP[t], A @ P[t]).T
        V = P[t] - G @ pP[t] @ G.T
        xs[:, t] = m[t] + (xs[:, t + 1] - pm[t]) @ G.T + noise[:, t] @ np.linalg.cholesky(0.5 * (V + V.T)).T
    return xs

