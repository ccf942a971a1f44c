"""Every compiled instance of the missing-observation routes (``missing="nan"``): the 26 (n, m) pairs of the
-DBF_MISSING=true build of csrc/kf_group_{a,b,c,d}.hip, the (n, m, lanes) rows of csrc/gsf_group_{a..e}.hip that
bf_gsf_ekf_missing_f32 can reach, and the ahead-of-time unscented shapes of csrc/ugsf_group_{u,v}.hip that no other
test launches.  Cases and references shared by tests/test_missing_instances_cpu.py (which validates them without a GPU) and
tests/test_missing_instances_gpu.py (which runs them).

Model of a row (n, m), all three parts: cm.random_stable_lgssm with the non-square noise maps of tests/test_all_instances_gpu.py,
dq = max(1, n - (n + m) % 3), dr = max(1, m - n % 2), biases on.  With dr < m the reduced (D R D^T)[o, o] is singular and S_oo
is positive definite only through H P H^T.  Seeds: 300 n + m (Kalman, extended Gaussian-sum), 400 n + m (unscented).

Kalman.  Geometry of kalman_staged_cases.geometry((n, m, 0)): B = 5 CPW + 3 (five whole waves staged, a tail of three
strided), T_max, t_min and cut as defined there; priors of heterogeneous_cases.priors (a mean and a covariance of its own per
trajectory); gaps of kalman_missing_cases.observed_mask with the wholly missing step at ``cut``, so that the second chunk of the
chunk test opens inside a gap.  Reference: the float64 recursion of the contract in kalman_missing_cases.py, vectorised over
the batch by grouping the trajectories of a step by their pattern.

Extended Gaussian-sum.  ``GSF_REACHABLE`` / ``GSF_UNREACHABLE`` (bf_gsf_ekf_missing_f32 refuses any kf_lanes but
gsf_default_lanes(n)).  Runs of a row, ``GSF_RUNS``: strided K = 3 + (n + m) % 3, B = 37, T = 19; staged K = 4, B = 64, T = 20
(K == KP, B % tpb == 0, (B K) % CPW == 0 and aligned rows at every n), reference on the first 8 trajectories; per-step Q_t / R_t
at the sizes of the strided run (whose inputs the collapsed-stream run shares).  Initial means m0 + 0.5 N(0, I).  Reference
gsf_missing_cases.reference, bounds gsf_missing_cases.bounds.  No row needed another seed to stay within the standard bounds
(test_missing_instances_cpu.py on the first trajectories; the GPU test asserts it on all).  The structured rows run
Lorenz-96(n) with the pick-even emission, built like gsf_missing_cases.model("l96"), initial means 0.05 N(0, I) as there.

Unscented.  ``UKF_SHAPES`` (n, dq, m, dr): linear registry models, K in {1, 3}, B = 37, T = 19, ParamsUKF(1, 0, 0), constant
and per-step covariances."""
import functools

import numpy as np

from oracle import gaussfilt_oracle as go, models as om
from tests import common as cm
from tests import gsf_missing_cases as gc
from tests import heterogeneous_cases as hc
from tests import kalman_missing_cases as kc
from tests import kalman_staged_cases as ks

F32, F64 = np.float32, np.float64
STREAMS = kc.STREAMS
LOG2PI = kc.LOG2PI
TOL, TOL_LL = ks.TOL, ks.TOL_LL      # tests/test_kalman_gpu.py: 1e-5 norm-wise, 2e-5 for the log-likelihood
HEADROOM_B = ks.HEADROOM_B           # trajectories 0-15 carry the headroom condition and every pattern


def noise_dims(n, m):
    return max(1, n - (n + m) % 3), max(1, m - n % 2)


def _frozen(d):
    for v in d.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def model(n, m, seed=None):
    dq, dr = noise_dims(n, m)
    return _frozen(cm.random_stable_lgssm(n, m, seed=300 * n + m if seed is None else seed, dq=dq, dr=dr, bias=True))


# ==== 1. Kalman ==========================================================================================================
KALMAN = [(n, m) for n in range(1, 9) for m in range(1, 5) if m <= n]                      # 26 pairs, four kernels each


def pair_id(p):
    return "x".join(str(v) for v in p)


def geometry(n, m):
    """kalman_staged_cases.geometry at the default lanes, with the causality horizons: t_min and the largest eligible T
    below T_max that is no multiple of the observation block 8 / m.  Where every eligible T is such a multiple (an odd n
    wants T % 4 == 0 and n = 6 an even T, which a block of two steps divides) it is the largest eligible T below T_max."""
    g = dict(ks.geometry((n, m, 0)))
    below = [T for T in g["horizons"] if T < g["t_max"]]
    ragged = [T for T in below if T % g["ys"]]
    g["causal"] = sorted({g["t_min"], (ragged or below)[-1]})
    return g


@functools.lru_cache(maxsize=None)
def kalman_data(n, m):
    """dict(a, ys complete, mask, gapped (B, T_max, m), m0s (B, n), P0s (B, n, n)), read-only."""
    g, a = geometry(n, m), model(n, m)
    ys = cm.simulate_batch(a, g["B"], g["t_max"], seed=n + 7 * m)
    mask = kc.observed_mask(g["B"], g["t_max"], m, wholly_missing_at=g["cut"])
    m0s, P0s = hc.priors(a, g["B"])
    return _frozen(dict(ys=ys, mask=mask, gapped=kc.gapped(ys, mask), m0s=m0s, P0s=P0s))


@functools.lru_cache(maxsize=None)
def kalman_tables(n, m):
    """Per-step (Q_t (T_max, dq, dq), R_t (T_max, dr, dr)), drawn as kalman_staged_cases.tables draws them (which holds the
    square noise maps of its own model): Q_t = (1 + 0.5 u_t) Q with u_t uniform on [0, 1), R_t likewise."""
    a, T = model(n, m), geometry(n, m)["t_max"]
    rng = np.random.default_rng(5)
    Qt = np.stack([(1 + 0.5 * rng.random()) * a["Q"] for _ in range(T)]).astype(F32)
    Rt = np.stack([(1 + 0.5 * rng.random()) * a["R"] for _ in range(T)]).astype(F32)
    Qt.setflags(write=False)
    Rt.setflags(write=False)
    return Qt, Rt


def kalman_missing_f64_batched(a, ys, m0s, P0s, Qt=None, Rt=None):
    """The contract of kalman_missing_cases.py in float64 for a batch ``ys`` (B, T, m), NaN = missing, from per-trajectory
    priors: at every step the trajectories are grouped by their pattern o (at most 2^m groups) and each group runs the update
    of the row-selected model H[o], (D r0)[o], (D R D^T)[o, o] -- the + 1e-6 on every entry of the reduced S_oo in the gain's
    solve, the log-likelihood log N(v_o; 0, S_oo) without it --; o empty passes.  Qt / Rt: per-step tables (step t predicts with
    Q_t and updates with R_t).  Dict of (B, 1, T, ...) float64 arrays."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    B, T, m = ys.shape
    n = A.shape[0]
    obs = ~np.isnan(ys)
    y64 = np.asarray(ys, F64)
    codes = obs @ (1 << np.arange(m))                            # (B, T): the pattern as an integer
    out = dict(weights=np.ones((B, 1, T)), means=np.empty((B, 1, T, n)), covariances=np.empty((B, 1, T, n, n)),
               predicted_means=np.empty((B, 1, T, n)), predicted_covariances=np.empty((B, 1, T, n, n)), loglik=np.zeros((B, 1, T)))
    mp, Pp = np.array(m0s, F64).reshape(B, n), np.array(P0s, F64).reshape(B, n, n)
    Dr0 = D @ r0
    for t in range(T):
        GQG = G @ (Q if Qt is None else np.asarray(Qt[t], F64)) @ G.T
        DRD = D @ (R if Rt is None else np.asarray(Rt[t], F64)) @ D.T
        mf, Pf = mp.copy(), Pp.copy()
        for code in np.unique(codes[:, t]):
            if code == 0:
                continue
            idx = np.flatnonzero(codes[:, t] == code)
            o = obs[idx[0], t]
            Ho = H[o]
            HP = Ho @ Pp[idx]                                    # (g, |o|, n)
            S = DRD[np.ix_(o, o)] + HP @ Ho.T
            K = np.swapaxes(np.linalg.solve(S + 1e-6, HP), 1, 2)
            v = y64[idx, t][:, o] - mp[idx] @ Ho.T - Dr0[o]
            mf[idx] = mp[idx] + (K @ v[:, :, None])[:, :, 0]
            Pf[idx] = Pp[idx] - K @ S @ np.swapaxes(K, 1, 2)
            Lc = np.linalg.cholesky(S)
            z = np.linalg.solve(Lc, v[:, :, None])[:, :, 0]
            out["loglik"][idx, 0, t] = (-0.5 * np.sum(z * z, axis=1) - 0.5 * int(o.sum()) * LOG2PI
                                        - np.sum(np.log(np.diagonal(Lc, axis1=1, axis2=2)), axis=1))
        mp, Pp = mf @ A.T + G @ q0, A @ Pf @ A.T + GQG
        out["means"][:, 0, t], out["covariances"][:, 0, t] = mf, Pf
        out["predicted_means"][:, 0, t], out["predicted_covariances"][:, 0, t] = mp, Pp
    return out


def variant_tables(n, m, variant):
    return kalman_tables(n, m) if variant == "QR" else (None, None)


@functools.lru_cache(maxsize=None)
def kalman_reference(n, m, variant="const"):
    """The float64 reference of the whole gapped batch over T_max steps; variant "const" or "QR"."""
    d = kalman_data(n, m)
    return _frozen(kalman_missing_f64_batched(model(n, m), d["gapped"], d["m0s"], d["P0s"], *variant_tables(n, m, variant)))


def kalman_headroom(n, m, variant="const"):
    """{stream: cm.rel_err of the float32 oracle on the row-compacted model (gsf_missing_cases.reference, K = 1) against
    float64} on trajectories 0 .. HEADROOM_B - 1 over T_max steps: the four streams, the log-likelihood and the carry."""
    d, a = kalman_data(n, m), dict(model(n, m))
    Qt, Rt = variant_tables(n, m, variant)
    po = cm.oracle_params(a)
    if Qt is not None:
        po = po._replace(dynamics_noise_covariance=Qt, emission_noise_covariance=Rt)
    per = [gc.reference(po, d["gapped"][b], 1, d["m0s"][b][None], init_covs=d["P0s"][b][None]) for b in range(HEADROOM_B)]
    r64 = kalman_reference(n, m, variant)
    out = {k: cm.rel_err(np.stack([p[k] for p in per]), r64[k][:HEADROOM_B]) for k in STREAMS[1:] + ("loglik",)}
    out["carry_means"] = cm.rel_err(np.stack([p["carry"][1] for p in per]), r64["predicted_means"][:HEADROOM_B, :, -1])
    out["carry_covariances"] = cm.rel_err(np.stack([p["carry"][2] for p in per]), r64["predicted_covariances"][:HEADROOM_B, :, -1])
    return out


# ==== 2. extended Gaussian-sum ==============================================================================================
GSF_DEFAULT_LANES = (0, 1, 1, 1, 2, 1, 2, 1, 2)      # kGsfDefaultLanes of csrc/gsf_scan.hip
GENERIC, L96 = "generic", "l96"                      # SPEC_GENERIC (groups a-d), SPEC_L96_PICK (group e)
# (spec, n, m, lanes per chain)
GSF_REACHABLE = ([(GENERIC, n, m, GSF_DEFAULT_LANES[n]) for n, m in KALMAN] + [(L96, 8, 4, 2), (L96, 4, 2, 2), (L96, 6, 3, 2)])
GSF_UNREACHABLE = [(GENERIC, 8, 4, 4), (L96, 8, 4, 1), (L96, 8, 4, 4), (L96, 4, 2, 1)]    # compiled, refused by the entry point
# rows without staged tiles (GsfCfg::STAGED_OK false): a covariance row of max(n^2, 32) floats holds a whole number of
# matrices and of 16-byte chunks, a power of two of them, at n = 1, 2, 4, 8 only
GSF_NO_STAGED_N = (3, 5, 6, 7)
GSF_RUNS = {"strided": dict(B=37, T=19, nref=None), "staged": dict(B=64, T=20, nref=8), "tv": dict(B=37, T=19, nref=None)}


def gsf_id(row):
    spec, n, m, lanes = row
    return f"{spec}-{n}x{m}-lanes{lanes}"


def gsf_K(row, run):
    return 4 if run == "staged" else 3 + (row[1] + row[2]) % 3


def _l96_pair(n):
    _, nl = gc._bfa()
    m = n // 2
    eye = lambda d, s=1.0: (s * np.eye(d)).astype(F32)
    return gc._pair(np.zeros(n), eye(n), om.Lorenz96(n), nl.lorenz96(n), np.zeros(n), eye(n, 1e-2), om.PickEven(n), nl.pick_even(n),
                    np.zeros(m), eye(m, 1e-1))


def _with_tables(po, pp, T):
    """Per-step Q_t / R_t drawn as gsf_missing_cases.model(tv=True) draws them."""
    rng = np.random.default_rng(7)
    Qt = (np.asarray(po.dynamics_noise_covariance, F32)[None] * (1 + rng.random((T, 1, 1)))).astype(F32)
    Rt = (np.asarray(po.emission_noise_covariance, F32)[None] * (1 + rng.random((T, 1, 1)))).astype(F32)
    kw = dict(dynamics_noise_covariance=Qt, emission_noise_covariance=Rt)
    return po._replace(**kw), pp._replace(**kw)


def _linear_case(a, B, T, K, tv, yseed, iseed, uparams):
    a = {k: np.array(v) for k, v in a.items()}                # (writable copies: the product hands its arrays to torch)
    po, pp = cm.oracle_params(a), cm.product_params(a)
    if tv:
        po, pp = _with_tables(po, pp, T)
    ys = cm.simulate_batch(a, B, T, seed=yseed)               # (drawn from the constant model)
    n, m = a["A"].shape[0], a["H"].shape[0]
    mask = kc.observed_mask(B, T, m)
    init = (a["m0"] + 0.5 * np.random.default_rng(iseed).normal(size=(B, K, n))).astype(F32)
    return dict(po=po, pp=pp, inputs=None, ys=ys, mask=mask, gapped=kc.gapped(ys, mask), init=init, uparams=uparams, K=K)


@functools.lru_cache(maxsize=None)
def gsf_case(row, run):
    """The inputs of one run of a row, in the layout of gsf_missing_cases.case (without the reference)."""
    spec, n, m, _ = row
    r, K = GSF_RUNS[run], gsf_K(row, run)
    if spec == GENERIC:
        return _linear_case(dict(model(n, m)), r["B"], r["T"], K, run == "tv", 2 * n + m, 10 * n + m, None)
    assert run != "tv"                                        # structure-aware instances take constant covariances
    po, pp = _l96_pair(n)
    ys = gc.simulate(po, r["B"], r["T"])
    mask = kc.observed_mask(r["B"], r["T"], m)
    init = (0.05 * np.random.default_rng(5).normal(size=(r["B"], K, n))).astype(F32)
    return dict(po=po, pp=pp, inputs=None, ys=ys, mask=mask, gapped=kc.gapped(ys, mask), init=init, uparams=None, K=K)


def _referenced(c, nref):
    nr = c["gapped"].shape[0] if nref is None else nref
    ref = gc._frozen(gc.batch(gc.reference, c["po"], c["gapped"][:nr], c["K"], c["init"][:nr], None, c["uparams"]))
    return dict(c, ref=ref, nref=nr)


@functools.lru_cache(maxsize=None)
def gsf_referenced(row, run, nref=None):
    """:func:`gsf_case` with the float32 reference of its first ``nref`` trajectories (default: those of ``GSF_RUNS``)."""
    return _referenced(gsf_case(row, run), GSF_RUNS[run]["nref"] if nref is None else nref)


@functools.lru_cache(maxsize=None)
def gsf_bounds(row, run, nref=None):
    """(bounds, headroom) of gsf_missing_cases.bounds on the referenced trajectories."""
    c = gsf_referenced(row, run, nref)
    return gc.bounds(c, c["K"])


STANDARD = dict({k: gc.TOL for k in STREAMS[1:] + ("loglik",)}, weights=gc.WTOL)


# ==== 3. unscented ===========================================================================================================
# (n, dq, m, dr) of csrc/ugsf_group_{u,v}.hip: those no other test launches, and the three that
# tests/test_gsf_missing_gpu.py runs on nonlinear models
UKF_SHAPES = [(2, 2, 1, 1), (2, 2, 2, 2), (3, 3, 1, 1), (3, 3, 3, 3), (4, 2, 1, 1), (4, 4, 2, 2)]
UKF_COVERED_ELSEWHERE = [(1, 1, 1, 1), (4, 2, 2, 2), (8, 8, 4, 4)]
UKF_K = (1, 3)
UKF_B, UKF_T = 37, 19


def ukf_id(shape):
    return "x".join(str(v) for v in shape)


@functools.lru_cache(maxsize=None)
def ukf_case(shape, K, tv):
    n, dq, m, dr = shape
    a = cm.random_stable_lgssm(n, m, seed=400 * n + m, dq=dq, dr=dr, bias=True)
    return _linear_case(a, UKF_B, UKF_T, K, tv, 2 * n + m, 10 * n + m, go.ParamsUKF(1.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def ukf_referenced(shape, K, tv, nref=None):
    return _referenced(ukf_case(shape, K, tv), nref)


@functools.lru_cache(maxsize=None)
def ukf_bounds(shape, K, tv, nref=None):
    c = ukf_referenced(shape, K, tv, nref)
    return gc.bounds(c, K, unscented=True)
