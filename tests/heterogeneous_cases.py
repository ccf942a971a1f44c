"""Linear-model batches in which every trajectory (and every Gaussian-sum component) starts from its OWN covariance, shared
by test_heterogeneous_batch_cpu.py (which checks, without a GPU, that each case is a meaningful comparison and that its
reference has headroom) and test_heterogeneous_batch_gpu.py (which runs them on the device).

For a linear model the covariance recursion does not read the data, so a batch that starts from one P0 carries identical
covariance streams and gains in every slot: a kernel that reads, stages or stores another trajectory's covariance, or reuses
a neighbour's gain, passes any test on such a batch.  Here chain c (trajectory b, or trajectory b / component k with
c = b K + k) starts from

    P0_c = L_c L_c^T + 0.5 I,  L_c = 0.5 N(0, 1)   and   m0_c = m0 + 0.3 N(0, I),   both from default_rng(1000 + c)

-- the recipe cm.random_stable_lgssm uses for its own P0, so the conditioning stays in the regime the tolerances were set for.

A case is a dict: name, family, n, m, K, B, T, seed (model), yseed (observations), tol / tol_ll (what the GPU test asserts:
the family's existing oracle test's tolerances, tests/test_kalman_gpu.py and tests/test_generic_gpu.py), tol_w (weights,
absolute, Gaussian sums), carry_T (the length of the run whose returned carry is held against the reference: T, except on
kf-cv), witness (whether ``not torch.equal`` against the run-time-dimension kernel is asserted).  Every reference is computed
once per process and handed out read-only."""
import functools

import numpy as np

from oracle import gaussfilt_oracle as go, c_oracle
from tests import common as cm

F32, F64 = np.float32, np.float64
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")
FIELDS = ("weights",) + STREAMS
TOL_C_PORT = 3e-6        # tests/test_oracle_filters.py::test_c_port_matches_numpy_oracle


def _case(name, family, n, m, B, T, seed, yseed, tol_ll, K=1, model="random", carry_T=None, witness=True):
    return dict(name=name, family=family, n=n, m=m, K=K, B=B, T=T, seed=seed, yseed=yseed, tol=1e-5, tol_ll=tol_ll, tol_w=2e-5,
                model=model, carry_T=T if carry_T is None else carry_T, witness=witness)


# A. the Kalman entry point, one group per kernel family (family "register": csrc/kf_scan_group.hpp; "runtime":
# csrc/generic_scan.hip, forced for n <= 8 and chosen by the entry point at (9, 2), (12, 4); "bf32": the one-wave matrix-core
# kernel csrc/kf_scan_bf32.hip, two waves per workgroup, so an odd B leaves a half-filled last workgroup; "mfma": the (64, 32)
# kernel csrc/kf_scan_mfma.hip).  kf-24-12 and kf-48-20 are the inputs of the smoother and sampler at n = 24, 48; kf-4-2-b130
# is a second n = 4, B = 130 input of the smoother, one on which fp32 has headroom (SMOOTHER_CASES).
# kf-cv, carry_T = 2: the returned carry is compared with the reference on the scale of its own step (cm.rel_err of the carry,
# as everywhere in the suite), and on that scale the constant-velocity recursion is sensitive -- the fp32 oracle's predicted
# covariance is 1.5e-6 from float64 after step 1, 2.4e-6 after step 2 and 6.0e-6 after step 23 (every other case: <= 4.2e-7
# after its last step).  Under the headroom rule (the reference within tol / 5 = 2e-6 of float64, else T changes, never the
# tolerance) the carry of THIS case is held against the reference after a 2-step run; the carry of the 24-step run must equal
# the last entries of its own predicted streams bit for bit, and those streams are held against the reference as whole arrays.
# witness = False on kf-cv and gsf-3-3-K5: there the register kernel and the run-time-dimension kernel produce the same bits
# (measured on the MI355X; A and H of the constant-velocity model hold only 0, 0.5 and 1, and the (3, 3) instance runs one
# lane per chain like that kernel), so equal bits say nothing about the routing; every other register case asserts it.
KALMAN_CASES = {c["name"]: c for c in [
    _case("kf-cv", "register", 4, 2, 130, 24, None, 1, 2e-5, model="cv", carry_T=2, witness=False),
    _case("kf-4-2-b130", "register", 4, 2, 130, 24, 422, 2, 2e-5),
    _case("kf-3-2", "register", 3, 2, 70, 16, 32, 3, 2e-5),
    _case("kf-7-4", "register", 7, 4, 70, 16, 74, 3, 2e-5),
    _case("kf-8-4", "register", 8, 4, 70, 16, 84, 3, 2e-5),
    _case("kf-4-2", "runtime", 4, 2, 5, 16, 42, 4, 5e-5),
    _case("kf-8-4-forced", "runtime", 8, 4, 5, 16, 85, 4, 5e-5),
    _case("kf-9-2", "runtime", 9, 2, 5, 16, 92, 4, 5e-5),
    _case("kf-12-4", "runtime", 12, 4, 5, 16, 124, 4, 5e-5),
    _case("kf-16-8", "bf32", 16, 8, 5, 14, 168, 5, 5e-5),
    _case("kf-17-3", "bf32", 17, 3, 5, 14, 173, 5, 5e-5),
    _case("kf-32-32", "bf32", 32, 32, 5, 14, 3232, 5, 5e-5),
    _case("kf-24-12", "bf32", 24, 12, 5, 14, 2412, 5, 5e-5),
    _case("kf-64-32", "mfma", 64, 32, 3, 10, 6432, 6, 5e-5),
    _case("kf-40-24", "mfma", 40, 24, 3, 10, 4024, 6, 5e-5),
    _case("kf-48-20", "mfma", 48, 20, 5, 14, 4820, 6, 5e-5),
]}

# B. Gaussian sums of a linear model, every (b, k) with its own prior ("register": csrc/gsf_scan.hpp; "bf32" / "mfma": the K
# components take turns on the matrix-core kernels as chains b K + k; "runtime": forced)
GSF_CASES = {c["name"]: c for c in [
    _case("gsf-4-2-K4", "register", 4, 2, 33, 10, 424, 7, 2e-5, K=4),
    _case("gsf-3-3-K5", "register", 3, 3, 3, 10, 335, 7, 2e-5, K=5, witness=False),
    _case("gsf-16-8-K4", "bf32", 16, 8, 3, 10, 1684, 8, 2e-5, K=4),
    _case("gsf-33-7-K2", "mfma", 33, 7, 3, 10, 3372, 8, 2e-5, K=2),
    _case("gsf-64-32-K3", "mfma", 64, 32, 3, 10, 64323, 8, 2e-5, K=3),
    _case("gsf-12-4-K3", "runtime", 12, 4, 3, 10, 1243, 8, 2e-5, K=3),
]}

CASES = {**KALMAN_CASES, **GSF_CASES}

# D. where the scan is cut in two: the carry handed over after step cut - 1 must still tell the chains apart (the differences
# decay geometrically: by the LAST step of kf-cv two trajectories' covariances agree to 1.5e-7, which is why a carry in the wrong
# slot has to be looked for at an early cut and not at the end of the scan)

# E. the smoother's inputs are the posteriors of these cases; fp32_headroom: whether a plain fp32 evaluation of the RTS
# recursion is within tol / 5 of float64 on them (``smoother_fp32_error``, asserted either way on the CPU).  kf-cv is the
# issue's n = 4, B = 130 input and has none: its large early covariances put ANY fp32 evaluation 1.6e-5 from float64, more
# than the 1e-5 the GPU test asserts (the engine measures 9.1e-6), so a change of rounding in the kernel can fail that case
# without a defect -- kf-4-2-b130 is the same shape with headroom.
SMOOTHER_CASES = {"kf-cv": False, "kf-4-2-b130": True, "kf-8-4": True, "kf-12-4": True, "kf-24-12": True, "kf-48-20": True}
TOL_SMOOTHER = 1e-5      # tests/test_smoother_gpu.py::_check

CHUNK_CUTS = {"kf-cv": 6, "kf-7-4": 5, "kf-9-2": 7, "kf-16-8": 5, "kf-64-32": 4, "gsf-4-2-K4": 6, "gsf-16-8-K4": 4, "gsf-33-7-K2": 3}


@functools.lru_cache(maxsize=None)
def _model_cached(name):
    c = CASES[name]
    a = cm.cv_model_arrays() if c["model"] == "cv" else cm.random_stable_lgssm(c["n"], c["m"], c["seed"], bias=True)
    for v in a.values():
        v.setflags(write=False)
    return a


def model(name):
    return dict(_model_cached(name))


def priors(a, count):
    """(m0_c (count, n), P0_c (count, n, n)) of the module docstring, fp32."""
    n = a["A"].shape[0]
    m0s, P0s = np.empty((count, n), F32), np.empty((count, n, n), F32)
    for c in range(count):
        rng = np.random.default_rng(1000 + c)
        L = 0.5 * rng.normal(size=(n, n))
        P0s[c] = (L @ L.T + 0.5 * np.eye(n)).astype(F32)
        m0s[c] = (a["m0"] + 0.3 * rng.normal(size=n)).astype(F32)
    return m0s, P0s


@functools.lru_cache(maxsize=None)
def data(name, B=None):
    """(emissions (B, T, m), initial means (B, K, n), initial covariances (B, K, n, n)), read-only; ``B``: another batch size
    than the case's (the placement tests take one without a ragged tail)."""
    c = CASES[name]
    B = c["B"] if B is None else B
    a = model(name)
    ys = cm.simulate_batch(a, B, c["T"], seed=c["yseed"])
    m0s, P0s = priors(a, B * c["K"])
    out = (ys, m0s.reshape(B, c["K"], c["n"]), P0s.reshape(B, c["K"], c["n"], c["n"]))
    for v in out:
        v.setflags(write=False)
    return out


# ---- references of one chain each -------------------------------------------------------------------------------------
def kalman_numpy(a, ys, m0s, P0s):
    """The NumPy oracle's _condition_on / _predict (gaussfiltax/inference.py:72-105, :51-70) looped over trajectories, each
    from its own prior: dict of (B, 1, T, ...) arrays like cm.oracle_kalman_batch."""
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
            ll, fm, fP, _, _ = go._condition_on(pm, pP, hn, R, r0, u, ys[b, t])
            pm, pP, _ = go._predict(fm, fP, fn, Q, q0, u)
            out["loglik"][b, 0, t] = ll
            out["means"][b, 0, t], out["covariances"][b, 0, t] = fm, fP
            out["predicted_means"][b, 0, t], out["predicted_covariances"][b, 0, t] = pm, pP
    return out


def kalman_fp32(a, ys, m0s, P0s):
    """The fp32 checker: the NumPy oracle below n = 16, its C port (pinned to it at 3e-6 by test_oracle_filters.py and, with
    init_covs, by test_heterogeneous_batch_cpu.py) from there."""
    if a["A"].shape[0] >= 16:
        return c_oracle.kalman_filter(a, ys, m0s, init_covs=P0s)
    return kalman_numpy(a, ys, m0s, P0s)


def kalman_f64(a, ys, m0s, P0s):
    """The same recursion in float64, trajectory by trajectory: tests/test_smoother_cpu.py::kalman_f64 with the two things
    the operation under test has and that one leaves out -- the reference's + 1e-6 on every entry of S in the gain's solve
    (gaussfiltax/utils.py:256-259; a 1e-5 relative perturbation at R = 0.1, an input of the operation and no rounding error)
    and the log-likelihood log N(y; H m- + D r0, S)."""
    A, G, H, D = (np.asarray(a[k], F64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], F64) for k in ("Q", "R", "q0", "r0"))
    GQG, DRD = G @ Q @ G.T, D @ R @ D.T
    B, T, m = ys.shape
    n = A.shape[0]
    out = dict(weights=np.ones((B, 1, T)), means=np.empty((B, 1, T, n)), covariances=np.empty((B, 1, T, n, n)),
               predicted_means=np.empty((B, 1, T, n)), predicted_covariances=np.empty((B, 1, T, n, n)), loglik=np.empty((B, 1, T)))
    for b in range(B):
        mp, Pp = np.asarray(m0s[b], F64), np.asarray(P0s[b], F64)
        for t in range(T):
            S = DRD + H @ Pp @ H.T
            K = np.linalg.solve(S + 1e-6, H @ Pp).T
            d = ys[b, t].astype(F64) - H @ mp - D @ r0
            mf = mp + K @ d
            Pf = Pp - K @ S @ K.T
            Lc = np.linalg.cholesky(S)
            z = np.linalg.solve(Lc, d)
            out["loglik"][b, 0, t] = -0.5 * z @ z - 0.5 * m * np.log(2 * np.pi) - np.sum(np.log(np.diag(Lc)))
            mp, Pp = A @ mf + G @ q0, A @ Pf @ A.T + GQG
            out["means"][b, 0, t], out["covariances"][b, 0, t] = mf, Pf
            out["predicted_means"][b, 0, t], out["predicted_covariances"][b, 0, t] = mp, Pp
    return out


def _weights(lls, reweight, dtype):
    """(B, K, T) weights from (B, K, T) per-component log-likelihoods, from 1 / K (inference.py:347-350)."""
    B, K, T = lls.shape
    w = np.empty((B, K, T), dtype)
    for b in range(B):
        cur = (np.ones(K, dtype) / dtype(K)).astype(dtype)
        for t in range(T):
            cur = reweight(lls[b, :, t], cur)
            w[b, :, t] = cur
    return w


def _reweight_f64(lls, w):
    x = np.exp(lls - np.max(lls)) * w
    return x / np.sum(x)


def _run(name, kalman, reweight, dtype, same_prior):
    c = CASES[name]
    a = model(name)
    ys, m0s, P0s = data(name)
    B, K, T, n = c["B"], c["K"], c["T"], c["n"]
    P = np.broadcast_to(P0s[0, 0], (B * K, n, n)) if same_prior else P0s.reshape(B * K, n, n)
    r = kalman(a, np.repeat(ys, K, axis=0), m0s.reshape(B * K, n), P)      # chain b K + k filters trajectory b
    out = {k: np.asarray(v).reshape((B, K) + v.shape[2:]) for k, v in r.items()}
    out["weights"] = _weights(out["loglik"], reweight, dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, same_prior=False):
    """The free-running fp32 reference of a case: dict of (B, K, T, ...) arrays, the five streams and "loglik" (per component).
    A linear model's component recursions do not read the weights, so each (b, k) is a Kalman chain of its own and the weights
    follow from the chains' log-likelihoods by go.reweight.  ``same_prior``: THE MUTATION the GPU tests are for -- every chain
    starts from chain 0's covariance, as a kernel that reads the wrong P_in would compute."""
    return _run(name, kalman_fp32, go.reweight, F32, same_prior)


@functools.lru_cache(maxsize=None)
def reference_f64(name):
    return _run(name, kalman_f64, _reweight_f64, F64, False)


def gsf_first_step(name, b):
    """Step 0 of trajectory b of a Gaussian-sum case as the oracle's scan body computes it from the GIVEN priors
    (inference.py:345-353: _condition_on per component, reweight from 1 / K, _predict): dict of (K, ...) arrays."""
    c = CASES[name]
    a = model(name)
    ys, m0s, P0s = data(name)
    p = cm.oracle_params(a)
    fn, hn = p.dynamics_function, p.emission_function
    Q, R, q0, r0 = (np.asarray(a[k], F32) for k in ("Q", "R", "q0", "r0"))
    u = np.zeros(1, F32)
    K, n = c["K"], c["n"]
    lls, fm, fP = np.empty(K, F32), np.empty((K, n), F32), np.empty((K, n, n), F32)
    pm, pP = np.empty((K, n), F32), np.empty((K, n, n), F32)
    for k in range(K):
        lls[k], fm[k], fP[k], _, _ = go._condition_on(m0s[b, k], P0s[b, k], hn, R, r0, u, ys[b, 0])
    w = go.reweight(lls, (np.ones(K, F32) / F32(K)).astype(F32))
    for k in range(K):
        pm[k], pP[k], _ = go._predict(fm[k], fP[k], fn, Q, q0, u)
    return dict(weights=w, means=fm, covariances=fP, predicted_means=pm, predicted_covariances=pP, loglik=lls)


# ---- the figures the CPU test asserts and the summary quotes -----------------------------------------------------------
def pairwise_min_rel_err(C):
    """min over ordered pairs i != j of cm.rel_err(C[i], C[j]) = max|C_i - C_j| / max|C_j| for C (chains, n, n)."""
    C = np.asarray(C, F64)
    num = np.max(np.abs(C[:, None] - C[None]), axis=(2, 3))
    den = np.maximum(np.max(np.abs(C), axis=(1, 2)), 1e-30)
    r = num / den[None, :]
    np.fill_diagonal(r, np.inf)
    return float(np.min(r))


def discrimination(name):
    """{t: (smallest rel_err between the filtered covariances of two distinct chains, rel_err of the mutated reference's
    filtered covariances against the true reference's)} at t = 0 and t = min(3, T - 1).  The second figure is taken over all
    chains at once, as the GPU test compares whole arrays: it is the worst chain's (chain 0 is unchanged by construction); that
    EVERY other chain moves is what the first figure says, since the mutation gives each of them chain 0's covariances."""
    c = CASES[name]
    ref, mut = reference(name), reference(name, True)
    n = c["n"]
    out = {}
    for t in (0, min(3, c["T"] - 1)):
        P = ref["covariances"][:, :, t].reshape(-1, n, n)
        out[t] = (pairwise_min_rel_err(P), cm.rel_err(mut["covariances"][:, :, t], ref["covariances"][:, :, t]))
    return out


def carry_discrimination(name):
    """Smallest rel_err between the predicted covariances (= the carry) of two distinct chains after step CHUNK_CUTS[name] - 1."""
    c = CASES[name]
    P = reference(name)["predicted_covariances"][:, :, CHUNK_CUTS[name] - 1]
    return pairwise_min_rel_err(P.reshape(-1, c["n"], c["n"]))


def headroom(name):
    """{stream: error of the fp32 reference against the float64 recursion} as the GPU test measures it (rel_err; weights:
    largest absolute difference; loglik of a Gaussian sum: per component; carry_*: the prediction after step carry_T - 1 on its
    own scale).  For a Gaussian sum this is the FREE-RUNNING chain-wise reference over all T steps, while the GPU test asserts
    step 0 and teacher-forced single steps, which compound nothing: the condition is stricter than that test needs."""
    ref, r64 = reference(name), reference_f64(name)
    out = {k: cm.rel_err(ref[k], r64[k]) for k in STREAMS + ("loglik",)}
    out["weights"] = float(np.max(np.abs(ref["weights"].astype(F64) - r64["weights"])))
    t = CASES[name]["carry_T"] - 1
    out["carry_means"] = cm.rel_err(ref["predicted_means"][:, :, t], r64["predicted_means"][:, :, t])
    out["carry_covariances"] = cm.rel_err(ref["predicted_covariances"][:, :, t], r64["predicted_covariances"][:, :, t])
    return out


def _rts_covariances_fp32(P, pP, F):
    """Smoothed covariances of ONE trajectory by the RTS recursion of tests/test_smoother_cpu.py::rts_f64 with every
    intermediate rounded to fp32: what a plain fp32 evaluation gives, no kernel involved."""
    P, pP, F = (np.asarray(x, F32) for x in (P, pP, F))
    T = P.shape[0]
    Ps = np.empty_like(P)
    b = Ps[T - 1] = P[T - 1]
    for t in range(T - 2, -1, -1):
        L = np.linalg.cholesky(pP[t]).astype(F32)
        G = np.linalg.solve(L.T, np.linalg.solve(L, np.matmul(F, P[t], dtype=F32)).astype(F32)).astype(F32).T
        b = (P[t] + np.matmul(np.matmul(G, (b - pP[t]).astype(F32), dtype=F32), G.T, dtype=F32)).astype(F32)
        Ps[t] = b
    return Ps


@functools.lru_cache(maxsize=None)
def smoother_fp32_error(name):
    """rel_err of the fp32 RTS recursion against the float64 one, smoothed covariances of the whole batch, both run on the
    fp32 reference's filtered streams of the case (the GPU test runs the float64 one on the engine's own streams)."""
    from tests.test_smoother_cpu import rts_f64
    r, A = reference(name), model(name)["A"]
    P32, P64 = [], []
    for b in range(CASES[name]["B"]):
        m, P, pm, pP = (r[k][b, 0] for k in STREAMS)
        P64.append(rts_f64(m, P, pm, pP, A)[1])
        P32.append(_rts_covariances_fp32(P, pP, A))
    return cm.rel_err(np.stack(P32), np.stack(P64))
