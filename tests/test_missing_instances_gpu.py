"""Every compiled instance of the missing-observation routes on the MI355X (``missing="nan"``): the 26 (n, m) pairs of
bf_kalman_filter_missing_f32 on both emitters with constant and per-step tables (104 kernels), every (n, m, lanes) row that
bf_gsf_ekf_missing_f32 can reach on its strided, staged, EXT and collapsed-only kernels, and the six ahead-of-time unscented
shapes of bf_ugsf_ukf_missing_f32 that no other test launches.  What depends on the instance -- the lane-group mapping under the
gap selects (padding lanes at n = 3, 5, 6, 7), an observation block of 8 / m steps that holds NaNs, the tile geometry of each
(n, lanes), the EXT variants, register allocation -- is not covered by the host program of the masked arithmetic.  Cases,
geometry and references: tests/missing_instance_cases.py (validated without a GPU by tests/test_missing_instances_cpu.py).

Every option goes through ``options=`` on the call.  kf_emit_mode = 2 is refused when the launch is not eligible for the staged
emitter, so a forced call that returns is the witness that the staged kernel ran; kf_emit_mode = 0 is the strided emitter.

Kalman, per pair (B = 5 CPW + 3: five whole waves staged, a tail of three strided; a prior of its own per trajectory):
  1. float64           the staged T_max run against the float64 recursion: streams and carry 1e-5 norm-wise, log-likelihood 2e-5
                       (tests/test_kalman_gpu.py), weights exactly 1, the gap identities and the carry bit for bit
  2. routes            the strided run and the batch-inner run == run 1 bit for bit, six outputs and the carry
  3. per-step tables   Q_t and R_t: staged == strided bit for bit and against float64, at T_max and the smallest T
  4. causality         shorter staged runs == the first steps of run 1 bit for bit: later gaps do not reach back
  5. chunks            two chunks through the carry, the second opening inside the wholly missing step, == run 1 bit for bit
Gaussian-sum, per row: a. strided, b. staged (or its refusal where the row has no staged tiles), c. per-step tables and
collapsed streams (EXT kernels; EMIT_NONE with ``fields=()``), against gsf_missing_cases.reference under the standard bounds.
Unscented, per shape: K = 1 and 3, constant and per-step covariances."""
import functools

import numpy as np
import pytest
import torch

from bayesianfiltering_amd._lib import BayesFiltError
from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import gsf_missing_cases as gc
from tests import missing_instance_cases as mi
from tests.test_gsf_missing_gpu import _bits, _compare, _filter, _np

pytestmark = pytest.mark.gpu
FULL5, STREAMS = mi.STREAMS, mi.STREAMS[1:]
KIDS = [mi.pair_id(p) for p in mi.KALMAN]
GIDS = [mi.gsf_id(r) for r in mi.GSF_REACHABLE]
STAGED, STRIDED = 2, 0


# ==== 1. Kalman ==========================================================================================================
class Case:
    """One (n, m) pair with its inputs on the device (uploaded once) and its runs."""

    def __init__(self, pair):
        self.pair, (self.n, self.m) = pair, pair
        self.g, self.d = mi.geometry(*pair), mi.kalman_data(*pair)
        self.pp = cm.product_params({k: np.array(v) for k, v in mi.model(*pair).items()})
        self.y = torch.as_tensor(self.d["gapped"].copy(), device="cuda")      # (the cases are read-only arrays)
        self.m0 = torch.as_tensor(self.d["m0s"].copy(), device="cuda")
        self.P0 = torch.as_tensor(self.d["P0s"].copy(), device="cuda")

    def params(self, variant, T):
        if variant == "const":
            return self.pp
        Qt, Rt = mi.kalman_tables(*self.pair)
        return self.pp._replace(dynamics_noise_covariance=Qt[:T], emission_noise_covariance=Rt[:T])

    def run(self, T, mode, variant="const", t0=0, carry=None, layout="reference"):
        """(posterior, log-likelihood, carry) of steps t0 .. t0 + T - 1 from the priors (or ``carry``)."""
        import bayesianfiltering_amd as bfa
        opts = {} if mode is None else {"kf_emit_mode": mode}
        start = dict(carry=carry, initial_means=None) if carry is not None else dict(initial_means=self.m0, initial_covariances=self.P0)
        return bfa.kalman_filter(self.params(variant, T), self.y[:, t0:t0 + T], missing="nan", layout=layout, return_loglik=True,
                                 return_carry=True, options=opts, **start)

    @functools.cached_property
    def full(self):
        """Run 1: the staged T_max run, never modified."""
        return self.run(self.g["t_max"], STAGED)


@functools.lru_cache(maxsize=None)
def case(pair):
    return Case(pair)


def _assert_same_bits(got, want, what, T=None):
    """Posterior, log-likelihood and (T = None) carry of two runs bit for bit; with T, ``want`` is cut to its first T steps."""
    for k in FULL5:
        w = getattr(want[0], k)
        assert torch.equal(getattr(got[0], k), w if T is None else w[:, :, :T]), (what, k)
    assert torch.equal(got[1], want[1] if T is None else want[1][:, :, :T]), (what, "loglik")
    if T is None:
        for x, y_, nm in zip(got[2], want[2], ("weights", "means", "covariances")):
            assert torch.equal(x, y_), (what, "carry." + nm)


def _assert_meets_float64(c, res, variant, T, what):
    ref = mi.kalman_reference(*c.pair, variant)
    post, ll, carry = res
    e = {k: cm.rel_err(_np(getattr(post, k)), ref[k][:, :, :T]) for k in STREAMS}
    e["loglik"] = cm.rel_err(_np(ll), ref["loglik"][:, :, :T])
    e["carry_means"] = cm.rel_err(_np(carry.means), ref["predicted_means"][:, :, T - 1])
    e["carry_covariances"] = cm.rel_err(_np(carry.covariances), ref["predicted_covariances"][:, :, T - 1])
    print(f"  {mi.pair_id(c.pair)} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    cm.record(f"kalman_missing_instance_vs_float64[{mi.pair_id(c.pair)}-{what}]", **e)
    for k, v in e.items():
        assert v < (mi.TOL_LL if k == "loglik" else mi.TOL), (what, k, v)
    assert bool((post.weights == 1.0).all()) and bool((carry.weights == 1.0).all()), what
    shape = (c.g["B"], 1, T)
    assert tuple(post.means.shape) == shape + (c.n,) and tuple(post.covariances.shape) == shape + (c.n, c.n)
    assert tuple(ll.shape) == shape


def _assert_gap_identities(c, res, T):
    """A step with nothing observed is predict-only, exactly: m+ = m-, P+ = P- bit for bit and log-likelihood 0; the
    log-likelihood is non-zero everywhere else; the carry is the last prediction."""
    post, ll, carry = res
    m_f, P_f, m_p, P_p, lls = (_np(v)[:, 0] for v in (post.means, post.covariances, post.predicted_means,
                                                     post.predicted_covariances, ll))
    empty = ~c.d["mask"][:, :T].any(axis=2)                      # (B, T)
    bs, ts = np.nonzero(empty[:, 1:])
    if T > c.g["cut"]:
        assert len(ts) >= c.g["B"] - 2                           # the wholly missing step of every gapped trajectory at least
    assert np.array_equal(m_f[bs, ts + 1].view(np.uint32), m_p[bs, ts].view(np.uint32))
    assert np.array_equal(P_f[bs, ts + 1].view(np.uint32), P_p[bs, ts].view(np.uint32))
    assert (lls[empty] == 0.0).all() and (lls[~empty] != 0.0).all()
    assert torch.equal(carry.means, post.predicted_means[:, :, -1]) and torch.equal(carry.covariances, post.predicted_covariances[:, :, -1])


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_float64(pair):
    c = case(pair)
    T = c.g["t_max"]
    _assert_meets_float64(c, c.full, "const", T, "const")
    _assert_gap_identities(c, c.full, T)


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_routes(pair):
    c = case(pair)
    T = c.g["t_max"]
    _assert_same_bits(c.run(T, STRIDED), c.full, "strided vs staged")
    _assert_same_bits(c.run(T, None, layout="batch_inner"), c.full, "batch_inner vs staged")


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_per_step_tables(pair):
    """kf_scan_group_kernel<..., TV = true, MISSING = true> on both emitters: step t predicts with Q_t and updates with R_t."""
    c = case(pair)
    for T in (c.g["t_max"], c.g["t_min"]):
        staged = c.run(T, STAGED, variant="QR")
        _assert_same_bits(staged, c.run(T, STRIDED, variant="QR"), f"QR T={T} staged vs strided")
        _assert_meets_float64(c, staged, "QR", T, f"QR-T{T}")
        _assert_gap_identities(c, staged, T)
        assert not torch.equal(staged[0].predicted_covariances, c.full[0].predicted_covariances[:, :, :T]), T


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_causality(pair):
    c = case(pair)
    for T in c.g["causal"]:
        _assert_same_bits(c.run(T, STAGED), c.full, f"T={T} vs the first steps of T_max={c.g['t_max']}", T=T)


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_chunks(pair):
    c = case(pair)
    T, cut = c.g["t_max"], c.g["cut"]
    assert not c.d["mask"][0, cut].any()                         # the second chunk opens inside a gap
    first = c.run(cut, None)
    second = c.run(T - cut, None, t0=cut, carry=first[2])
    for k in FULL5:
        parts = torch.cat([getattr(first[0], k), getattr(second[0], k)], dim=2)
        assert torch.equal(parts, getattr(c.full[0], k)), (cut, k)
    assert torch.equal(torch.cat([first[1], second[1]], dim=2), c.full[1]), (cut, "loglik")
    for x, y_, nm in zip(second[2], c.full[2], ("weights", "means", "covariances")):
        assert torch.equal(x, y_), (cut, "carry." + nm)


# ==== 2. extended Gaussian-sum ==============================================================================================
def _standard_bounds(bounds_and_headroom, what):
    """gsf_missing_cases.bounds of the case, which must be the standard ones: a case whose float32 reference is further than a
    quarter of them from float64 gets another seed, not a wider bound."""
    bound, h = bounds_and_headroom
    assert bound == mi.STANDARD, (what, h)
    return bound


def _assert_streams_same_bits(x, y, what):
    for k in FULL5:
        assert np.array_equal(_bits(getattr(x[0], k)), _bits(getattr(y[0], k))), (what, k)
    assert np.array_equal(_bits(x[1]), _bits(y[1])), (what, "loglik")
    for a, b in zip(x[2], y[2]):
        assert np.array_equal(_bits(a), _bits(b)), (what, "carry")


def _strided(row, what, **options):
    c = mi.gsf_referenced(row, "strided")
    bound = _standard_bounds(mi.gsf_bounds(row, "strided"), what)
    worst = _compare(_filter(c, c["K"], options=dict(options, kf_emit_mode=STRIDED)), c["ref"], bound, label=what)
    cm.record(f"gsf_missing_instance[{what}]", **worst)


@pytest.mark.parametrize("row", mi.GSF_REACHABLE, ids=GIDS)
def test_gsf_strided(row):
    _strided(row, f"{mi.gsf_id(row)} strided")


@pytest.mark.parametrize("row", [r for r in mi.GSF_REACHABLE if r[0] == mi.L96 and r[1] != 8], ids=mi.gsf_id)
def test_gsf_structured_model_on_the_dense_instance(row):
    """The Lorenz-96 model of a structured row on the generic instance of its (n, m) (tests/test_gsf_missing_gpu.py has (8, 4))."""
    _strided(row, f"{mi.gsf_id(row)} dense", gsf_structured=0)


@pytest.mark.parametrize("row", mi.GSF_REACHABLE, ids=GIDS)
def test_gsf_staged(row):
    """K = 4, B = 64, T = 20: the LDS-staged emitter, forced, against the reference on the first trajectories (the fixed
    patterns among them) and bit for bit against the strided emitter on all; a row without staged tiles refuses the force."""
    what = f"{mi.gsf_id(row)} staged"
    if row[1] in mi.GSF_NO_STAGED_N:
        c = mi.gsf_case(row, "staged")
        with pytest.raises(BayesFiltError, match="staged emitter needs"):
            _filter(c, c["K"], options={"kf_emit_mode": STAGED})
        return
    c = mi.gsf_referenced(row, "staged")
    bound = _standard_bounds(mi.gsf_bounds(row, "staged"), what)
    staged = _filter(c, c["K"], options={"kf_emit_mode": STAGED})
    worst = _compare(staged, c["ref"], bound, nr=c["nref"], label=what)
    cm.record(f"gsf_missing_instance[{what}]", **worst)
    _assert_streams_same_bits(staged, _filter(c, c["K"], options={"kf_emit_mode": STRIDED}), what)


@pytest.mark.parametrize("row", mi.GSF_REACHABLE, ids=GIDS)
def test_gsf_ext(row):
    """The EXT kernels: per-step Q_t / R_t (generic rows; the structure-aware instances take constant covariances), the
    collapsed streams beside the five, and alone (``fields=()``: the EMIT_NONE kernel)."""
    rid = mi.gsf_id(row)
    if row[0] == mi.GENERIC:
        c = mi.gsf_referenced(row, "tv")
        bound = _standard_bounds(mi.gsf_bounds(row, "tv"), rid + " tv")
        worst = _compare(_filter(c, c["K"]), c["ref"], bound, label=rid + " per-step Q/R")
        cm.record(f"gsf_missing_instance[{rid} tv]", **worst)
    c = mi.gsf_referenced(row, "strided")
    K = c["K"]
    bound = _standard_bounds(mi.gsf_bounds(row, "strided"), rid + " collapsed")
    post, ll, carry, (cmean, ccov) = _filter(c, K, return_collapsed=True)
    worst = _compare((post, ll, carry), c["ref"], bound, label=rid + " collapsed")
    cm.record(f"gsf_missing_instance[{rid} collapsed]", **worst)
    w, mu, P = (_np(x).astype(np.float64) for x in (post.weights, post.means, post.covariances))
    B, T = w.shape[0], w.shape[2]
    want = [[go.collapse(mu[b, :, t], P[b, :, t], w[b, :, t]) for t in range(T)] for b in range(B)]
    wm, wP = np.array([[x[0] for x in r] for r in want]), np.array([[x[1] for x in r] for r in want])
    assert _np(cmean).shape == wm.shape and _np(ccov).shape == wP.shape
    for b in range(B):
        for t in range(T):
            assert gc.rel_err(_np(cmean)[b, t], wm[b, t]) < 1e-5 and gc.rel_err(_np(ccov)[b, t], wP[b, t]) < 1e-5, (b, t)
    only = _filter(c, K, fields=(), return_collapsed=True, return_loglik=False, return_carry=False)
    assert np.array_equal(_bits(only[1][0]), _bits(cmean)) and np.array_equal(_bits(only[1][1]), _bits(ccov))


# ==== 3. unscented ===========================================================================================================
@pytest.mark.parametrize("tv", [False, True], ids=["const", "tv"])
@pytest.mark.parametrize("K", mi.UKF_K)
@pytest.mark.parametrize("shape", mi.UKF_SHAPES, ids=mi.ukf_id)
def test_unscented(shape, K, tv):
    what = f"unscented {mi.ukf_id(shape)} K={K} {'tv' if tv else 'const'}"
    c = mi.ukf_referenced(shape, K, tv)
    bound = _standard_bounds(mi.ukf_bounds(shape, K, tv), what)
    worst = _compare(_filter(c, K, unscented=True), c["ref"], bound, label=what)
    cm.record(f"gsf_missing_instance[{what}]", **worst)
