"""Every compiled instance of the register Kalman kernel (csrc/kf_scan_group.hpp, the tables of csrc/kf_group_{a,b,c,d}.hip in
their plain build) on its LDS-staged emitter: the cases shared by test_kalman_staged_cpu.py (which pins the geometry below to the header's
formulas and checks that the references have headroom, without a GPU) and test_kalman_staged_gpu.py (which runs them).

One case per instance: the 26 (n, m) pairs at their default lanes per trajectory plus (4, 2) at kf_lanes 1 and 4 -- 28.

    model          cm.random_stable_lgssm(n, m, seed=300 n + m, bias=True)
    observations   cm.simulate_batch(a, B, T_max, seed=n + 7 m)
    priors         heterogeneous_cases.priors(a, B): a mean and a covariance of its own per trajectory, so that a kernel that
                   stages or stores a neighbour's row cannot pass
    batch          B = 5 CPW + 3: the staged launch gets five whole waves (two workgroups, the second partly filled), the
                   strided launch a tail of three

Geometry the cases rely on (GroupCfg in the header; CPW = 64 / lanes trajectories per wave; depth = steps per LDS tile row,
TP::TS / TM::TS / TW::TS for the covariance, mean and scalar streams):

    n            lanes  CPW  depth P  depth m  depth w
    1            1      64   32       16       16
    2            1      64   8        8        16
    3            2      32   4        12       32
    4            2      32   2        8        32
    4 (lanes 1)  1      64   2        4        16
    4 (lanes 4)  4      16   2        8        32
    5            4      16   4        4        16
    6            4      16   1        4        16
    7            4      16   4        4        16
    8            4      16   1        2        16

An observation block is YS = 8 / m steps (8, 4, 2, 2).  A horizon T is eligible for the staged emitter when T n and T n^2 are
multiples of 4 (launch_nml: rows_aligned): T % 4 == 0 for odd n, T even for n = 2, 6, any T for n = 4, 8.  With T % 4 != 0 the
weight and log-likelihood rows leave as dword stores (wscalar).  With D the largest of an instance's three depths, T_max is the
smallest eligible T >= 2 D + YS + 1 (at most 76): two whole rows of the deepest tile, a whole observation block and a ragged
end.  No case needed another seed or a shorter horizon for headroom (test_kalman_staged_cpu.py).

References: the float64 Kalman recursion of heterogeneous_cases.kalman_f64 (reference jitter included) vectorised over the
batch, and the NumPy fp32 oracle looped per trajectory; both also take per-step (T, d, d) Q and R.  Computed once per process,
handed out read-only."""
import functools

import numpy as np

from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import heterogeneous_cases as hc

F32, F64 = np.float32, np.float64
STREAMS = hc.STREAMS
FULL5 = ("weights",) + STREAMS
TOL, TOL_LL = 1e-5, 2e-5          # tests/test_kalman_gpu.py
HEADROOM_B = 16                   # trajectories 0-15 carry the headroom condition

# (n, m, kf_lanes option): 0 = the default lanes per trajectory of launch_kf_group
INSTANCES = [(n, m, 0) for n in range(1, 9) for m in range(1, 5) if m <= n and (n, m) != (1, 2)] + [(4, 2, 1), (4, 2, 4)]
# the table above, restated as data: key (n, lanes actually run) -> (depth P, depth m, depth w)
DEPTHS = {(1, 1): (32, 16, 16), (2, 1): (8, 8, 16), (3, 2): (4, 12, 32), (4, 2): (2, 8, 32), (4, 1): (2, 4, 16),
          (4, 4): (2, 8, 32), (5, 4): (4, 4, 16), (6, 4): (1, 4, 16), (7, 4): (4, 4, 16), (8, 4): (1, 2, 16)}


def case_id(inst):
    n, m, lanes = inst
    return f"{n}x{m}" + (f"-lanes{lanes}" if lanes else "")


def default_lanes(n):
    """csrc/kf_scan_group.hip, default_lanes: n <= 2 ? 1 : (n <= 4 ? 2 : 4)."""
    return 1 if n <= 2 else (2 if n <= 4 else 4)


def eligible(n, T):
    """launch_nml's rows_aligned with all streams enabled: rows of T n and T n^2 floats stay 16-byte aligned."""
    return (T * n) % 4 == 0 and (T * n * n) % 4 == 0


def geometry(inst):
    """dict(lanes, cpw, depths (P, m, w), ys, B, t_max, t_min, horizons, subset_horizons, cut) of an instance.
    subset_horizons: where the stream subsets run -- T_max and, where T_max % 4 != 0 (the scalar streams then leave as dwords
    and their two tiles are never carved), also the largest eligible T % 4 == 0 below it, so that every instance runs its
    subsets with the weight and log-likelihood tiles staged."""
    n, m, opt = inst
    lanes = opt or default_lanes(n)
    depths = DEPTHS[(n, lanes)]
    ys = 8 // m
    t_max = next(T for T in range(2 * max(depths) + ys + 1, 200) if eligible(n, T))
    horizons = [T for T in range(1, t_max + 1) if eligible(n, T)]
    subset_horizons = [t_max] + ([max(T for T in horizons if T % 4 == 0)] if t_max % 4 else [])
    return dict(lanes=lanes, cpw=64 // lanes, depths=depths, ys=ys, B=5 * (64 // lanes) + 3, t_max=t_max, t_min=horizons[0],
                horizons=horizons, subset_horizons=subset_horizons, cut=chunk_cut(n, depths, ys, t_max))


def chunk_cut(n, depths, ys, t_max):
    """Where the unaligned-chunk test cuts T_max: a step in the second half that is a multiple of neither YS nor any tile
    depth (a depth of one step divides every T and is left out).  Where such a step exists with both chunks eligible for the
    staged emitter the first of those is taken, so that both chunks run staged under the default emit mode; at n = 3, 5, 7 an
    eligible length is a multiple of 4 and hence of the depth-4 tile, and at n = 6 with m = 3, 4 it is even and hence a multiple
    of YS = 2: there both chunks leave through the strided emitter."""
    periods = [d for d in depths + (ys,) if d > 1]
    free = [c for c in range(t_max // 2, t_max) if all(c % d for d in periods)]
    staged = [c for c in free if eligible(n, c) and eligible(n, t_max - c)]
    return (staged or free)[0]


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def model(inst):
    n, m, _ = inst
    return _frozen(cm.random_stable_lgssm(n, m, seed=300 * n + m, bias=True))


@functools.lru_cache(maxsize=None)
def data(inst):
    """(emissions (B, T_max, m), prior means (B, n), prior covariances (B, n, n)), read-only."""
    n, m, _ = inst
    g = geometry(inst)
    a = model(inst)
    ys = cm.simulate_batch(a, g["B"], g["t_max"], seed=n + 7 * m)
    m0s, P0s = hc.priors(a, g["B"])
    for v in (ys, m0s, P0s):
        v.setflags(write=False)
    return ys, m0s, P0s


@functools.lru_cache(maxsize=None)
def tables(inst):
    """Per-step (Q_t (T_max, dq, dq), R_t (T_max, dr, dr)): Q_t = (1 + 0.5 u_t) Q with u_t uniform on [0, 1), R_t likewise, as
    tests/test_generic_gpu.py::test_time_varying_covariances_any_dimension draws them."""
    a, T = model(inst), geometry(inst)["t_max"]
    rng = np.random.default_rng(5)
    Qt = np.stack([(1 + 0.5 * rng.random()) * a["Q"] for _ in range(T)]).astype(F32)
    Rt = np.stack([(1 + 0.5 * rng.random()) * a["R"] for _ in range(T)]).astype(F32)
    Qt.setflags(write=False)
    Rt.setflags(write=False)
    return Qt, Rt


TABLE_VARIANTS = ("QR", "Q", "R")      # which of Q / R is a per-step table


def variant_tables(inst, variant):
    """(Q_t or None, R_t or None) of "const", "QR", "Q", "R"."""
    Qt, Rt = tables(inst)
    return (Qt if "Q" in variant else None), (Rt if "R" in variant else None)


# ---- references ---------------------------------------------------------------------------------------------------------
def kalman_f64_batched(a, ys, m0s, P0s, Qt=None, Rt=None):
    """heterogeneous_cases.kalman_f64 for all trajectories at once: the float64 recursion with the reference's + 1e-6 on every
    entry of S in the gain's solve and the log-likelihood log N(y; H m- + D r0, S).  Qt / Rt: per-step (T, d, d) covariances in
    place of a["Q"] / a["R"] (step t predicts with Q_t and updates with R_t: _get_params(x, 2, t), inference.py:337-340).
    Dict of (B, 1, T, ...) float64 arrays."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    B, T, m = ys.shape
    n = A.shape[0]
    out = dict(weights=np.ones((B, 1, T)), means=np.empty((B, 1, T, n)), covariances=np.empty((B, 1, T, n, n)),
               predicted_means=np.empty((B, 1, T, n)), predicted_covariances=np.empty((B, 1, T, n, n)), loglik=np.empty((B, 1, T)))
    mp, Pp = np.asarray(m0s, F64).reshape(B, n), np.asarray(P0s, F64).reshape(B, n, n)
    for t in range(T):
        GQG = G @ (Q if Qt is None else np.asarray(Qt[t], F64)) @ G.T
        DRD = D @ (R if Rt is None else np.asarray(Rt[t], F64)) @ D.T
        HP = H @ Pp                                              # (B, m, n)
        S = DRD + HP @ H.T
        K = np.swapaxes(np.linalg.solve(S + 1e-6, HP), 1, 2)     # (B, n, m)
        d = ys[:, t].astype(F64) - mp @ H.T - D @ r0
        mf = mp + (K @ d[:, :, None])[:, :, 0]
        Pf = Pp - K @ S @ np.swapaxes(K, 1, 2)
        Lc = np.linalg.cholesky(S)
        z = np.linalg.solve(Lc, d[:, :, None])[:, :, 0]
        out["loglik"][:, 0, t] = (-0.5 * np.sum(z * z, axis=1) - 0.5 * m * np.log(2 * np.pi)
                                  - np.sum(np.log(np.diagonal(Lc, axis1=1, axis2=2)), axis=1))
        mp, Pp = mf @ A.T + G @ q0, A @ Pf @ A.T + GQG
        out["means"][:, 0, t], out["covariances"][:, 0, t] = mf, Pf
        out["predicted_means"][:, 0, t], out["predicted_covariances"][:, 0, t] = mp, Pp
    return out


def kalman_numpy(a, ys, m0s, P0s, Qt=None, Rt=None):
    """The fp32 NumPy oracle per trajectory: heterogeneous_cases.kalman_numpy, and with per-step tables the same loop over
    the oracle's _condition_on / _predict with R_t / Q_t handed to step t."""
    if Qt is None and Rt is None:
        return hc.kalman_numpy(a, ys, m0s, P0s)
    p = cm.oracle_params(a)
    fn, hn = p.dynamics_function, p.emission_function
    Q, R, q0, r0 = (np.asarray(a[k], F32) for k in ("Q", "R", "q0", "r0"))
    u = np.zeros(1, F32)
    B, T = ys.shape[:2]
    n = a["A"].shape[0]
    out = dict(weights=np.ones((B, 1, T), F32), means=np.empty((B, 1, T, n), F32), covariances=np.empty((B, 1, T, n, n), F32),
               predicted_means=np.empty((B, 1, T, n), F32), predicted_covariances=np.empty((B, 1, T, n, n), F32),
               loglik=np.empty((B, 1, T), F32))
    for b in range(B):
        pm, pP = np.asarray(m0s[b], F32), np.asarray(P0s[b], F32)
        for t in range(T):
            ll, fm, fP, _, _ = go._condition_on(pm, pP, hn, R if Rt is None else np.asarray(Rt[t], F32), r0, u, ys[b, t])
            pm, pP, _ = go._predict(fm, fP, fn, Q if Qt is None else np.asarray(Qt[t], F32), q0, u)
            out["loglik"][b, 0, t] = ll
            out["means"][b, 0, t], out["covariances"][b, 0, t] = fm, fP
            out["predicted_means"][b, 0, t], out["predicted_covariances"][b, 0, t] = pm, pP
    return out


@functools.lru_cache(maxsize=None)
def reference_f64(inst, variant="const"):
    """The float64 reference of the whole batch over T_max steps; variant "const", or which of Q / R is a per-step table."""
    ys, m0s, P0s = data(inst)
    Qt, Rt = variant_tables(inst, variant) if variant != "const" else (None, None)
    return _frozen(kalman_f64_batched(model(inst), ys, m0s, P0s, Qt, Rt))


def headroom(inst, variant="const"):
    """{stream: cm.rel_err of the fp32 oracle against float64} on trajectories 0 .. HEADROOM_B - 1 over T_max steps: the four
    streams, the log-likelihood and the carry (the prediction after the last step, on its own scale).  The CPU test holds every
    one of them, the log-likelihood included, to TOL / 5 = 2e-6."""
    ys, m0s, P0s = (v[:HEADROOM_B] for v in data(inst))
    Qt, Rt = variant_tables(inst, variant) if variant != "const" else (None, None)
    r32 = kalman_numpy(dict(model(inst)), ys, m0s, P0s, Qt, Rt)
    r64 = reference_f64(inst, variant)
    out = {k: cm.rel_err(r32[k], r64[k][:HEADROOM_B]) for k in STREAMS + ("loglik",)}
    out["carry_means"] = cm.rel_err(r32["predicted_means"][:, :, -1], r64["predicted_means"][:HEADROOM_B, :, -1])
    out["carry_covariances"] = cm.rel_err(r32["predicted_covariances"][:, :, -1], r64["predicted_covariances"][:HEADROOM_B, :, -1])
    return out
