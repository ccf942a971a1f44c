"""Cases for missing observations on the one-wave matrix-core Kalman kernel (``bf_kalman_filter_missing_tiles_f32`` /
``bf_gsf_ekf_missing_tiles_f32``, include/bayesfilt_ext2.h; DESIGN.md 4a'''): the shapes, the Gaussian-sum models that kernel
serves, and a float64 restatement of the kernel's own step -- the 32 x 32 embedding with unit rows for what is missing.  Shared
by tests/test_matrix_missing_cpu.py and tests/test_matrix_missing_gpu.py.  The references are those of
tests/kalman_missing_cases.py (float64, from the contract: the REDUCED model) and tests/gsf_missing_cases.py (the oracle's own
steps on the really compacted model, and its float64 copy)."""
import functools

import numpy as np

from oracle import models as om
from tests import common as cm
from tests import generic_missing_cases as xc
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc

F32, F64 = np.float32, np.float64
TILE = 32
T = 19
BATCHES = (1, 5)          # 1: a lone wave in a two-wave workgroup; 5: an odd chain count, and the fixed patterns exist
# (n, m), each the smallest at which a piece can go wrong: the lower edge of the route in n; in m (with n = 9); 29 permanently
# padded rows next to the missing ones; no padding, every tile row can go missing; m > n; the README's shape
KALMAN_SHAPES = [(16, 8), (9, 9), (17, 3), (32, 32), (12, 30), (32, 16)]


def kalman_case(n, m, B, T=T, tv=False):
    """``generic_missing_cases.kalman_case``: the models, emissions, initial means and frozen float64 reference of
    tests/kalman_missing_cases.py on a mask whose trajectory 0 holds a fully observed step at t = 2, next to its partly observed
    ones, the wholly missing step at T // 2 and the forecast tail."""
    return xc.kalman_case(n, m, B, T, tv)


# ---- the kernel's step, restated in float64 ------------------------------------------------------------------------------------
def embedded_f64(a, ys, m_init, P_init):
    """ONE trajectory ys (T, m), NaN = missing, the way kf_scan_bf32_kernel<..., MISSING = true> computes it, in float64: every
    step is a 32 x 32 system in which a row that is padded (a >= m) or missing has a zero row of H, a unit diagonal entry of
    D R D^T and nothing else in its row and column, and innovation 0; the +1e-6 sits on EVERY entry of that system; with
    L L^T = S + 1e-6, W = L^-1 H P, g = L^-1 1, z = L^-1 v:  m+ = m- + W^T z,  P+ = P- - W^T W + 1e-6 (W^T g)(W^T g)^T, the
    log-likelihood of the un-jittered S by the determinant lemma, plus 1/2 log 2 pi (32 - |o|) for the unit rows.  A step with
    nothing observed is skipped.  Returns what ``kalman_missing_cases.kalman_missing_f64`` returns."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    ys = np.asarray(ys, F64)
    m, n = H.shape
    mp, Pp, w = np.asarray(m_init, F64).copy(), np.asarray(P_init, F64).copy(), 1.0
    out = {k: [] for k in kc.STREAMS + ("loglik",)}
    eps = 1e-6
    for t in range(ys.shape[0]):
        Qt = Q[t] if Q.ndim == 3 else Q
        Rt = R[t] if R.ndim == 3 else R
        o = np.flatnonzero(~np.isnan(ys[t]))
        if o.size:
            H32, DRD, v = np.zeros((TILE, n)), np.eye(TILE), np.zeros(TILE)
            H32[o] = H[o]
            DRD[np.ix_(o, o)] = (D @ Rt @ D.T)[np.ix_(o, o)]
            v[o] = ys[t, o] - (H[o] @ mp + (D @ r0)[o])
            S = DRD + H32 @ Pp @ H32.T
            L = np.linalg.cholesky(S + eps)
            W, g, z = np.linalg.solve(L, H32 @ Pp), np.linalg.solve(L, np.ones(TILE)), np.linalg.solve(L, v)
            c = W.T @ g
            mf = mp + W.T @ z
            Pf = Pp - W.T @ W + eps * np.outer(c, c)
            one_m = 1.0 - eps * float(g @ g)
            quad = float(z @ z) + eps * float(g @ z) ** 2 / one_m
            ll = (-0.5 * quad - 0.5 * TILE * kc.LOG2PI - float(np.sum(np.log(np.diag(L)))) - 0.5 * np.log(one_m)
                  + 0.5 * kc.LOG2PI * (TILE - o.size))
        else:
            mf, Pf, ll = mp.copy(), Pp.copy(), 0.0
        w = 1.0 if (np.isfinite(ll) and np.isfinite(w) and w != 0.0) else np.nan
        mp = A @ mf + G @ q0
        Pp = A @ Pf @ A.T + G @ Qt @ G.T
        for k, x in zip(kc.STREAMS + ("loglik",), (w, mf, Pf, mp, Pp, ll)):
            out[k].append(np.array(x, F64))
    res = {k: np.stack(x) for k, x in out.items()}
    res["carry"] = (w, mp, Pp)
    return res


def embedded_batch(c):
    """:func:`embedded_f64` over the trajectories of a case, shaped like ``kalman_missing_cases.batch_reference``."""
    a = c["a"]
    per = [embedded_f64(a, c["gapped"][b], c["init"][b], a["P0"]) for b in range(c["gapped"].shape[0])]
    ref = {k: np.stack([p[k] for p in per])[:, None] for k in kc.STREAMS + ("loglik",)}
    ref["carry"] = tuple(np.stack([np.asarray(p["carry"][i], F64) for p in per])[:, None] for i in range(3))
    return ref


# ---- Gaussian sums the one-wave kernel serves ----------------------------------------------------------------------------------
GSF_CASES = ("lin", "lintv", "l96", "sine")
LINEAR_GSF = ("lin", "lintv")       # held to the standard bounds; the nonlinear ones to gsf_missing_cases.bounds


def gsf_model(name, T=T):
    """``name``: lin -- a linear model (16, 8), K = 3; lintv -- a linear model (24, 12) with per-step Q_t / R_t tables, K = 2;
    l96 -- Lorenz-96 at n = 16 through the even-state emission (m = 8), K = 3; sine -- the sine map at n = 16, the same
    emission, K = 2.  Returns (po, pp, K): oracle parameters, product parameters, components."""
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    eye = lambda d, s=1.0: (s * np.eye(d)).astype(F32)
    if name in LINEAR_GSF:
        a = kc.model(16, 8) if name == "lin" else kc.model(24, 12, True, T)
        return cm.oracle_params(a), cm.product_params(a), 3 if name == "lin" else 2
    n = 16
    if name == "l96":
        fo, fp, K = om.Lorenz96(n), nl.lorenz96(n), 3
    elif name == "sine":
        fo, fp, K = om.Sine(n, 1.5), nl.sine(n, 1.5), 2
    else:
        raise KeyError(name)
    po, pp = gc._pair(np.zeros(n), eye(n), fo, fp, np.zeros(n), eye(n, 1e-2), om.PickEven(n), nl.pick_even(n), np.zeros(n // 2),
                      eye(n // 2, 1e-1))
    return po, pp, K


@functools.lru_cache(maxsize=None)
def gsf_case(name, B=4, T=T):
    """One Gaussian-sum case, computed once and shared (no test writes into it), laid out like ``gsf_missing_cases.case``.  The
    emissions are drawn from the model with constant covariances (lintv: the filter's tables need not match them)."""
    po, pp, K = gsf_model(name, T)
    if name in LINEAR_GSF:
        n, m = (16, 8) if name == "lin" else (24, 12)
        ys = cm.simulate_batch(kc.model(n, m), B, T, seed=3)
    else:
        ys = gc.simulate(po, B, T)
    mask = gc.observed_mask(B, T, ys.shape[-1])
    n = np.asarray(po.initial_mean).size
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(5).normal(size=(B, K, n))).astype(F32)
    yg = gc.gapped(ys, mask)
    ref = gc._frozen(gc.batch(gc.reference, po, yg, K, init, None, None))
    return dict(po=po, pp=pp, inputs=None, ys=ys, mask=mask, gapped=yg, init=init, ref=ref, nref=B, uparams=None, K=K)


@functools.lru_cache(maxsize=None)
def gsf_bounds(name, B=4, T=T):
    """(bound, headroom) per stream.  Linear models: the standard 1e-5 (weights and log-likelihood 2e-5), the bounds of the
    matrix-core Gaussian-sum test on complete data.  Nonlinear ones: ``gsf_missing_cases.bounds``, from the reference's own
    error alone, as ``generic_missing_cases.gsf_bounds`` does."""
    c = gsf_case(name, B, T)
    with np.errstate(all="ignore"):
        b, h = gc.bounds(c, c["K"])
    if name in LINEAR_GSF:
        b = {k: (gc.WTOL if k in ("weights", "loglik") else gc.TOL) for k in b}
    return b, h
