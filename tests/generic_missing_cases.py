"""Cases for missing observations on the run-time-dimension kernel (``bf_kalman_filter_missing_anydim_f32`` /
``bf_gsf_ekf_missing_anydim_f32``, include/bayesfilt_ext.h; DESIGN.md 4a''): the shapes, the Gaussian-sum models above the register
limits, and the sources of the same Lorenz-96 model.  Shared by tests/test_generic_missing_cpu.py and
tests/test_generic_missing_gpu.py.  The references are the dimension-generic ones of tests/kalman_missing_cases.py (float64, from
the contract) and tests/gsf_missing_cases.py (the oracle's own steps on the really compacted model, and its float64 copy)."""
import functools

import numpy as np

from oracle import models as om
from tests import common as cm
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc
from tests import source_smoother_cases as sc

F32 = np.float32

# Kalman, K = 1 -- the smallest shapes at which each piece can go wrong: n just over the register limit; m over it; m > n;
# (12, 4); (33, 6): above gen_nt64_max = 32, the 256-thread workgroup whose barriers are real
KALMAN_SHAPES = [(9, 2), (6, 5), (3, 6), (12, 4), (33, 6)]
BATCHES = (1, 5)          # 5: the fixed patterns FULL, NONE and NO_COMP1 exist
T = 19


@functools.lru_cache(maxsize=None)
def kalman_case(n, m, B, T=T, tv=False):
    """``kalman_missing_cases.case`` (same models, emissions, initial means and float64 reference, computed once and frozen) on
    a mask whose trajectory 0 -- the only one at B = 1 -- holds a fully observed step at t = 2 whatever m is, next to its partly
    observed ones, the wholly missing step at T // 2 and the forecast tail."""
    a = kc.model(n, m, tv, T)
    ys = cm.simulate_batch(kc.model(n, m), B, T, seed=3)
    mask = kc.observed_mask(B, T, m)
    mask[0, 2] = True
    init = (np.tile(a["m0"], (B, 1)) + 0.3 * np.random.default_rng(5).normal(size=(B, n))).astype(F32)
    yg = kc.gapped(ys, mask)
    return dict(a=a, ys=ys, mask=mask, gapped=yg, init=init, ref=kc._frozen(kc.batch_reference(a, yg, init)))


PICK_EVEN_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  for (int a = 0; a < BF_M; ++a) out[a] = x[2 * a] + r[a];
}
"""


def _sv_matrices(n):
    """A stable banded Phi and a banded, diagonally dominant R for the stochastic-volatility model at dimension n."""
    Phi = (0.75 * np.eye(n) + 0.08 * np.eye(n, k=1) - 0.05 * np.eye(n, k=-1)).astype(F32)
    R = (0.12 * np.eye(n) + 0.02 * (np.eye(n, k=1) + np.eye(n, k=-1))).astype(F32)
    r0 = np.where(np.arange(n) % 2 == 0, 0.1, -0.2).astype(F32)
    return Phi, R, r0


def gsf_model(name, T=T):
    """``name``: l96 -- Lorenz-96 at n = 12 observed through pick_even (m = 6); l96src -- the same model with both functions
    given as source; sv -- linear dynamics with the stochastic-volatility emission at n = m = 9 (state-dependent noise Jacobian,
    the alternating input of the ``sv`` case of tests/gsf_missing_cases.py); svleak -- ``sv`` with its last component decoupled
    from the others (in Phi and in R) for the test of what a missing row may hold.  Returns (po, pp, inputs, K)."""
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    eye = lambda d, s=1.0: (s * np.eye(d)).astype(F32)
    if name in ("l96", "l96src"):
        n = 12
        f, h = nl.lorenz96(n), nl.pick_even(n)
        if name == "l96src":
            f = nl.user_dynamics(sc.L96_SRC, n, theta=sc.L96_THETA)
            h = nl.user_emission(PICK_EVEN_SRC, n, n // 2)
        po, pp = gc._pair(np.zeros(n), eye(n), om.Lorenz96(n), f, np.zeros(n), eye(n, 1e-2), om.PickEven(n), h, np.zeros(n // 2),
                          eye(n // 2, 1e-1))
        return po, pp, None, 3
    if name in ("sv", "svleak"):
        n = 9
        Phi, R, r0 = _sv_matrices(n)
        if name == "svleak":
            Phi[n - 1, :], Phi[:, n - 1], Phi[n - 1, n - 1] = 0.0, 0.0, 1.0
            R[n - 1, :n - 1], R[:n - 1, n - 1] = 0.0, 0.0
        u = np.array([t % 2 for t in range(T)], F32)
        po, pp = gc._pair(np.zeros(n), eye(n), om.Linear(Phi), nl.linear_dynamics(Phi), np.zeros(n), eye(n, 0.5), om.StochVol(n),
                          nl.stoch_vol(n), r0, R)
        return po, pp, u, 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def gsf_case(name, B=4, T=T):
    """One Gaussian-sum case, computed once and shared (no test writes into it), laid out like ``gsf_missing_cases.case``: the
    model, complete and gapped emissions, the mask, the initial means (B, K, n), the float32 reference of the gapped run."""
    po, pp, u, K = gsf_model(name, T)
    ys = gc.simulate(gsf_model("l96" if name == "l96src" else name, T)[0], B, T, u)
    mask = gc.observed_mask(B, T, ys.shape[-1])
    n = np.asarray(po.initial_mean).size
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(5).normal(size=(B, K, n))).astype(F32)
    yg = gc.gapped(ys, mask)
    iu = None if u is None else u.reshape(T, 1)
    ref = gc._frozen(gc.batch(gc.reference, po, yg, K, init, iu, None))
    return dict(po=po, pp=pp, inputs=u, ys=ys, mask=mask, gapped=yg, init=init, ref=ref, nref=B, uparams=None, K=K)


@functools.lru_cache(maxsize=None)
def gsf_bounds(name, B=4, T=T):
    """(bound, headroom) per stream of ``gsf_case(name)``: ``gsf_missing_cases.bounds``, from the reference's own error alone."""
    c = gsf_case(name, B, T)
    with np.errstate(all="ignore"):
        return gc.bounds(c, c["K"])


def mask_has_every_kind_of_step(mask):
    """Per trajectory-independent requirement on a case's (B, T, m) mask: somewhere a fully observed step, a wholly missing step
    after t = 0 that is not part of the forecast tail, a partly observed step, and the forecast tail itself."""
    count = mask.sum(axis=2)
    m, T_ = mask.shape[2], mask.shape[1]
    inner = count[:, 1:T_ - kc.FORECAST]
    return bool((count == m).any() and (inner == 0).any() and (m == 1 or ((count > 0) & (count < m)).any())
                and (count[:, T_ - kc.FORECAST:] == 0).all(axis=1).any())
