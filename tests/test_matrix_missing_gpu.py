"""Missing observations on the one-wave matrix-core Kalman kernel on the MI355X (``kalman_filter(..., missing="nan")`` and
``gaussian_sum_filter(..., missing="nan")`` where the plain call runs that kernel: 9 <= n <= 32, m <= 32 and (n >= 16 or m > 8);
``bf_kalman_filter_missing_tiles_f32`` / ``bf_gsf_ekf_missing_tiles_f32``): against the float64 contract of
tests/kalman_missing_cases.py and the compacted float32 reference of tests/gsf_missing_cases.py, at the shapes and models of
tests/matrix_missing_cases.py.

Tolerances are the project's: norm-wise 1e-5 for the streams and the carry (this kernel's bound and every gapped route's), 5e-5
for the log-likelihood (the bound of test_models_padded_into_the_matrix_core_kernel for this kernel), 1e-5 for the smoothed
streams; the linear Gaussian sums are held to 1e-5 with 2e-5 for weights and log-likelihood
(test_gaussian_sum_of_a_linear_model_on_the_matrix_cores), the nonlinear ones to ``gsf_missing_cases.bounds``."""
import ctypes as C

import numpy as np
import pytest

from tests import common as cm
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc
from tests import matrix_missing_cases as mc

pytestmark = pytest.mark.gpu
TOL, TOL_LL, TOL_SMOOTHED = 1e-5, 5e-5, 1e-5
F32 = np.float32
T = mc.T
GENERIC = {"force_generic": 1}


def _np(x):
    return x.detach().cpu().numpy()


def _kf(c, ys=None, **kw):
    """The gapped Kalman call of a case (any of ``kalman_filter``'s keywords may replace the defaults)."""
    import bayesianfiltering_amd as bfa
    kw.setdefault("initial_means", c["init"])
    if "observed" not in kw:
        kw.setdefault("missing", "nan")
    return bfa.kalman_filter(cm.product_params(c["a"]), c["gapped"] if ys is None else ys, **kw)


def _gsf(c, ys=None, pp=None, **kw):
    import bayesianfiltering_amd as bfa
    kw.setdefault("initial_means", c["init"])
    kw.setdefault("missing", "nan")
    return bfa.gaussian_sum_filter(c["pp"] if pp is None else pp, c["gapped"] if ys is None else ys, c["K"], 1, None, **kw)


def _errs(post, ll, ref):
    e = {k: cm.rel_err(_np(getattr(post, k)), ref[k]) for k in kc.STREAMS}
    e["loglik"] = cm.rel_err(_np(ll), ref["loglik"])
    return e


def _assert_streams(post, ll, ref, label):
    e = _errs(post, ll, ref)
    print(label, {k: f"{v:.2e}" for k, v in e.items()})
    for k in kc.STREAMS:
        assert _np(getattr(post, k)).shape == ref[k].shape, (label, k)
        assert e[k] < TOL, (label, k, e[k])
    assert e["loglik"] < TOL_LL, (label, e["loglik"])


def _assert_same_bits(x, y, label, carry=False):
    """Streams and log-likelihood of two (post, ll[, carry]) results, bit for bit."""
    for k in kc.STREAMS:
        assert np.array_equal(_np(getattr(x[0], k)), _np(getattr(y[0], k)), equal_nan=True), (label, k)
    assert np.array_equal(_np(x[1]), _np(y[1]), equal_nan=True), (label, "loglik")
    if carry:
        for a, b in zip(x[2], y[2]):
            assert np.array_equal(_np(a), _np(b), equal_nan=True), (label, "carry")


def _differs(x, y):
    return any(not np.array_equal(_np(getattr(x[0], k)), _np(getattr(y[0], k))) for k in kc.STREAMS[1:])


def _assert_gap_identities(post, ll, mask, K=1):
    """A step with nothing observed: m+ = m-, P+ = P- and ll = 0 exactly; elsewhere ll != 0; with one component the weights are 1."""
    m_f, P_f, m_p, P_p, lls = (_np(v) for v in (post.means, post.covariances, post.predicted_means, post.predicted_covariances, ll))
    empty = ~mask.any(axis=2)                                      # (B, T)
    bs, ts = np.nonzero(empty[:, 1:])
    assert len(ts) >= kc.FORECAST
    assert np.array_equal(m_f[bs, :, ts + 1], m_p[bs, :, ts]) and np.array_equal(P_f[bs, :, ts + 1], P_p[bs, :, ts])
    for k in range(K):
        assert (lls[:, k][empty] == 0.0).all() and (lls[:, k][~empty] != 0.0).all()
    if K == 1:
        assert (_np(post.weights) == 1.0).all()


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("n,m", mc.KALMAN_SHAPES)
def test_kalman_shapes_match_the_float64_contract(n, m, B):
    """Every shape and batch size against the contract, the gap identities exactly -- and on the matrix-core kernel: the
    streams are not the run-time-dimension kernel's, which served these calls before and rounds differently."""
    c = mc.kalman_case(n, m, B)
    post, ll, carry = _kf(c, return_loglik=True, return_carry=True)
    assert _differs((post, ll), _kf(c, return_loglik=True, options=GENERIC)), (n, m, B)
    _assert_streams(post, ll, c["ref"], (n, m, B))
    for got, want, name in zip(carry, c["ref"]["carry"], ("w", "m", "P")):
        assert _np(got).shape == want.shape and cm.rel_err(_np(got), want) < TOL, ("carry", name)
    _assert_gap_identities(post, ll, c["mask"])
    if B > kc.NONE:
        assert (_np(ll)[kc.NONE] == 0.0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(32, 16), (16, 8)])
def test_complete_data_is_the_plain_matrix_core_call_bit_for_bit(n, m):
    """Which kernel ran: on complete data the gapped call equals the plain call -- streams, carry and log-likelihood -- and not
    the run-time-dimension kernel's gapped call, which rounds differently."""
    import bayesianfiltering_amd as bfa
    c = mc.kalman_case(n, m, 5)
    plain = bfa.kalman_filter(cm.product_params(c["a"]), c["ys"], initial_means=c["init"], return_loglik=True, return_carry=True)
    new = _kf(c, ys=c["ys"], return_loglik=True, return_carry=True)
    _assert_same_bits(new, plain, (n, m), carry=True)
    generic = _kf(c, ys=c["ys"], return_loglik=True, options=GENERIC)
    assert _differs(new, generic), (n, m)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", mc.KALMAN_SHAPES)
def test_a_never_observed_component_is_the_row_reduced_model_on_the_plain_kernel(n, m):
    import bayesianfiltering_amd as bfa
    c = mc.kalman_case(n, m, 5)
    b = kc.NO_COMP1
    assert not c["mask"][b, :, 1].any() and np.delete(c["mask"][b], 1, axis=1).all()
    keep = [i for i in range(m) if i != 1]
    reduced = cm.product_params(kc.row_reduced(c["a"], keep))
    want, ll0 = bfa.kalman_filter(reduced, c["ys"][b:b + 1][:, :, keep], initial_means=c["init"][b:b + 1], return_loglik=True)
    post, ll = _kf(c, return_loglik=True)
    e = {k: cm.rel_err(_np(getattr(post, k))[b:b + 1], _np(getattr(want, k))) for k in kc.STREAMS}
    e["loglik"] = cm.rel_err(_np(ll)[b:b + 1], _np(ll0))
    print((n, m), "largest difference from the row-reduced model:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e[k] for k in kc.STREAMS) < TOL and e["loglik"] < TOL_LL, e


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _chunked(run, ys, init, cuts, Tn):
    parts, carry, t0 = [], None, 0
    for t1 in cuts + (Tn,):
        kw = dict(initial_means=init) if carry is None else dict(carry=carry, initial_means=None)
        post, ll, carry = run(ys[:, t0:t1], **kw)
        parts.append((post, ll))
        t0 = t1
    return parts, carry


def _assert_chunks_equal(parts, carry, whole, label):
    for k in kc.STREAMS:
        assert np.array_equal(np.concatenate([_np(getattr(p, k)) for p, _ in parts], axis=2), _np(getattr(whole[0], k))), (label, k)
    assert np.array_equal(np.concatenate([_np(l) for _, l in parts], axis=2), _np(whole[1])), label
    for x, y in zip(carry, whole[2]):
        assert np.array_equal(_np(x), _np(y)), (label, "carry")


@pytest.mark.parametrize("n,m", [(32, 16), (17, 3)])
def test_chunks_through_the_carry_inside_a_gap_are_bit_exact(n, m):
    c = mc.kalman_case(n, m, 5)
    cut = T // 2                                                   # the wholly missing step: the second chunk starts in the gap
    assert not c["mask"][0, cut].any()
    whole = _kf(c, return_loglik=True, return_carry=True)
    run = lambda ys, **kw: _kf(c, ys=ys, return_loglik=True, return_carry=True, **kw)
    for cuts in ((cut,), (cut + 1,), (T - 3,)):                    # ... ends in it, inside the forecast tail
        parts, carry = _chunked(run, c["gapped"], c["init"], cuts, T)
        _assert_chunks_equal(parts, carry, whole, cuts)


@pytest.mark.parametrize("n,m", [(32, 16), (9, 9)])
def test_a_trajectorys_bits_do_not_depend_on_its_neighbours_gaps_or_its_position(n, m):
    """Positions 0 and 4 are the first waves of two different workgroups; at position 1 the trajectory is a second wave."""
    c = mc.kalman_case(n, m, 5)
    base = _kf(c, return_loglik=True)
    probe = 0                                                      # a trajectory with the random pattern
    for fill, position in ((c["ys"], probe), (np.full_like(c["ys"], np.nan), probe), (c["ys"], 4), (c["gapped"], 1)):
        ys = np.array(fill)
        ys[position] = c["gapped"][probe]
        init = np.array(c["init"])
        init[position] = c["init"][probe]
        post, ll = _kf(c, ys=ys, initial_means=init, return_loglik=True)
        for k in kc.STREAMS:
            assert np.array_equal(_np(getattr(post, k))[position], _np(getattr(base[0], k))[probe]), (position, k)
        assert np.array_equal(_np(ll)[position], _np(base[1])[probe]), position


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_observed_mask_forms_equal_the_nan_form():
    n, m, B = 16, 8, 5
    c = mc.kalman_case(n, m, B)
    rng = np.random.default_rng(2)
    for shape in ((T,), (B, T), (T, m), (B, T, m)):
        mk = rng.random(shape) > 0.3
        full = np.broadcast_to(mk.reshape({(T,): (1, T, 1), (B, T): (B, T, 1), (T, m): (1, T, m)}.get(shape, shape)), (B, T, m))
        a = _kf(c, ys=c["ys"], observed=mk, return_loglik=True)
        b = _kf(c, ys=kc.gapped(c["ys"], full), return_loglik=True)
        _assert_same_bits(a, b, shape)


def test_inf_is_not_missing_and_nan_poisons_without_the_keyword():
    import bayesianfiltering_amd as bfa
    n, m, B, tb, bb = 16, 8, 5, 6, 3
    c = mc.kalman_case(n, m, B)
    clean = _kf(c, return_loglik=True)
    for value, comp in ((np.inf, 0), (-np.inf, m - 1)):
        ys = np.array(c["gapped"])
        ys[bb, tb, comp] = value                                   # whatever the mask said: this entry is now observed
        post, ll = _kf(c, ys=ys, return_loglik=True)
        mm, lls, w = _np(post.means), _np(ll), _np(post.weights)
        seen = ~np.isnan(ys[bb, tb:]).all(axis=1)
        assert np.isnan(w[bb, 0, tb:]).all() and (~np.isfinite(mm[bb, 0, tb:])).any(axis=1).all()
        assert seen[0] and (~np.isfinite(lls[bb, 0, tb:][seen])).all() and (lls[bb, 0, tb:][~seen] == 0.0).all()
        others = np.arange(B) != bb
        for k in kc.STREAMS:
            got, want = _np(getattr(post, k)), _np(getattr(clean[0], k))
            assert np.array_equal(got[others], want[others]) and np.array_equal(got[bb, 0, :tb], want[bb, 0, :tb]), k
        assert np.array_equal(lls[others], _np(clean[1])[others])
    # without the keyword a NaN is no gap: it poisons its trajectory from that step on, and only it
    ys = np.array(c["ys"])
    ys[bb, tb, 0] = np.nan
    plain = bfa.kalman_filter(cm.product_params(c["a"]), ys, initial_means=c["init"])
    w = _np(plain.weights)
    assert np.isnan(w[bb, 0, tb:]).all() and np.isfinite(w[np.arange(B) != bb]).all() and np.isfinite(w[bb, 0, :tb]).all()


def test_per_step_covariances():
    c = mc.kalman_case(32, 16, 5, T, True)
    post, ll = _kf(c, return_loglik=True)
    _assert_streams(post, ll, c["ref"], "tv (32, 16)")
    _assert_gap_identities(post, ll, c["mask"])
    generic = _kf(c, return_loglik=True, options=GENERIC)
    assert _differs((post, ll), generic)                           # (the per-step instance of the matrix-core kernel did run)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.GSF_CASES)
def test_gaussian_sums_match_the_compacted_reference(name):
    c = mc.gsf_case(name)
    bound, _ = mc.gsf_bounds(name)
    K = c["K"]
    post, ll, carry = _gsf(c, return_loglik=True, return_carry=True)
    e = _errs(post, ll, c["ref"])
    e["weights"] = float(np.abs(_np(post.weights).astype(np.float64) - c["ref"]["weights"]).max())
    print(name, {k: f"{v:.2e}" for k, v in e.items()}, "bounds", {k: f"{v:.1e}" for k, v in bound.items()})
    for k, v in e.items():
        assert v < bound[k], (name, k, v, bound[k])
    for got, want, k in zip(carry, c["ref"]["carry"], ("weights", "predicted_means", "predicted_covariances")):
        d = float(np.abs(_np(got) - want).max()) if k == "weights" else cm.rel_err(_np(got), want)
        assert d < bound[k], ("carry", k, d)
    # a step with nothing observed changes only the weights (renormalised), and with them nothing else
    _assert_gap_identities(post, ll, c["mask"], K)
    w = _np(post.weights)
    bs, ts = np.nonzero(~c["mask"].any(axis=2)[:, 1:])
    assert np.allclose(w[bs, :, ts + 1], w[bs, :, ts], rtol=1e-6, atol=0)
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("name", mc.GSF_CASES)
def test_gaussian_sums_on_complete_data_are_the_plain_call_bit_for_bit(name):
    c = mc.gsf_case(name)
    plain = _gsf(c, ys=c["ys"], missing=None, return_loglik=True, return_carry=True)
    new = _gsf(c, ys=c["ys"], return_loglik=True, return_carry=True)
    _assert_same_bits(new, plain, name, carry=True)
    generic = _gsf(c, ys=c["ys"], return_loglik=True, options=GENERIC)
    assert _differs(new, generic), name


def _sliced(pp, t0, t1):
    """The parameters of a chunk: per-step tables are sliced with the observations."""
    kw = {k: np.asarray(getattr(pp, k))[t0:t1] for k in ("dynamics_noise_covariance", "emission_noise_covariance")
          if np.asarray(getattr(pp, k)).ndim == 3}
    return pp._replace(**kw) if kw else pp


@pytest.mark.parametrize("name", ["lintv", "l96"])
def test_gaussian_sum_chunks_inside_a_gap_are_bit_exact(name):
    c = mc.gsf_case(name)
    cut = T // 2
    assert not c["mask"][0, cut].any()
    whole = _gsf(c, return_loglik=True, return_carry=True)
    first = _gsf(c, ys=c["gapped"][:, :cut], pp=_sliced(c["pp"], 0, cut), return_loglik=True, return_carry=True)
    second = _gsf(c, ys=c["gapped"][:, cut:], pp=_sliced(c["pp"], cut, T), carry=first[2], initial_means=None, return_loglik=True,
                  return_carry=True)
    _assert_chunks_equal([first[:2], second[:2]], second[2], whole, name)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def _anydim_call(c):
    """bf_kalman_filter_missing_anydim_f32 itself, through ctypes, on the gapped emissions of a Kalman case: the five streams and
    the log-likelihood as (B, 1, T, ...) arrays."""
    import torch
    from bayesianfiltering_amd import _lib
    lib = _lib.require_gpu()
    a = c["a"]
    B, Tn, m = c["gapped"].shape
    n = a["A"].shape[0]
    keep = []

    def fp(x):
        keep.append(np.ascontiguousarray(x, F32))
        return keep[-1].ctypes.data_as(_lib._FP)

    p = _lib.bf_lgssm()
    p.n, p.dq, p.m, p.dr = n, a["G"].shape[1], m, a["D"].shape[1]
    p.A, p.G, p.H, p.D, p.Q, p.R, p.q0, p.r0 = (fp(a[k]) for k in ("A", "G", "H", "D", "Q", "R", "q0", "r0"))
    p.Q_steps, p.R_steps = 1, 1
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, F32), device="cuda")
    y, m_in, P_in = dev(c["gapped"]), dev(c["init"]), dev(np.tile(a["P0"], (B, 1, 1)))
    ys = _lib.bf_cstream()
    ys.ptr, ys.sB, ys.sT, ys.sE = y.data_ptr(), Tn * m, m, 1
    carry = _lib.bf_carry()
    carry.m_in, carry.P_in = m_in.data_ptr(), P_in.data_ptr()
    od = _lib.bf_out_desc()
    sizes = {"weights": 1, "means": n, "covs": n * n, "pred_means": n, "pred_covs": n * n, "loglik": 1}
    bufs = {k: torch.empty((B, 1, Tn, e), dtype=torch.float32, device="cuda") for k, e in sizes.items()}
    for k, e in sizes.items():
        s = getattr(od, k)
        s.ptr, s.sB, s.sK, s.sT, s.sE = bufs[k].data_ptr(), Tn * e, 0, e, 1
    _lib.check(lib.bf_kalman_filter_missing_anydim_f32(C.byref(p), C.byref(ys), B, Tn, C.byref(carry), C.byref(od), None))
    torch.cuda.synchronize()
    shaped = {"weights": (B, 1, Tn), "means": (B, 1, Tn, n), "covs": (B, 1, Tn, n, n), "pred_means": (B, 1, Tn, n),
              "pred_covs": (B, 1, Tn, n, n), "loglik": (B, 1, Tn)}
    return {k: _np(v).reshape(shaped[k]) for k, v in bufs.items()}


_C_NAMES = dict(zip(kc.STREAMS, ("weights", "means", "covs", "pred_means", "pred_covs")))


def test_force_generic_and_small_mode_off_are_the_anydim_entry_point_bit_for_bit():
    from bayesianfiltering_amd import _lib
    c = mc.kalman_case(32, 16, 5)
    want = _anydim_call(c)
    lib = _lib.require_gpu()
    forced = _kf(c, return_loglik=True, options=GENERIC)
    _lib.check(lib.bf_set_option(b"kf_small_mode", 0))
    try:
        off = _kf(c, return_loglik=True)
    finally:
        _lib.check(lib.bf_set_option(b"kf_small_mode", 1))
    for label, got in (("force_generic", forced), ("kf_small_mode = 0", off)):
        for k in kc.STREAMS:
            assert np.array_equal(_np(getattr(got[0], k)), want[_C_NAMES[k]], equal_nan=True), (label, k)
        assert np.array_equal(_np(got[1]), want["loglik"]), (label, "loglik")
    assert _differs(_kf(c, return_loglik=True), forced)


def test_33_6_stays_on_the_run_time_dimension_kernel():
    """Outside the one-wave kernel nothing moves: the default gapped (33, 6) call on complete data is the plain force_generic
    kernel bit for bit (streams and carry), as tests/test_generic_missing_gpu.py pins it."""
    import bayesianfiltering_amd as bfa
    c = mc.kalman_case(33, 6, 5)
    plain = bfa.kalman_filter(cm.product_params(c["a"]), c["ys"], initial_means=c["init"], options=GENERIC, return_carry=True)
    new = _kf(c, ys=c["ys"], return_carry=True)
    for k in kc.STREAMS:
        assert np.array_equal(_np(getattr(new[0], k)), _np(getattr(plain[0], k))), k
    for x, y in zip(new[1], plain[1]):
        assert np.array_equal(_np(x), _np(y)), "carry"


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_passes_on_the_gapped_posterior():
    import torch
    import bayesianfiltering_amd as bfa
    n, m, B, S = 16, 8, 5, 3
    c = mc.kalman_case(n, m, B)
    p = cm.product_params(c["a"])
    ref = c["ref"]
    via_kw = bfa.kalman_smoother(p, c["gapped"], initial_means=c["init"], missing="nan")
    via_post = bfa.rts_smoother(p, _kf(c))
    for label, s in (("kalman_smoother", via_kw), ("rts_smoother", via_post)):
        e = (cm.rel_err(_np(s.smoothed_means), ref["smoothed_means"]), cm.rel_err(_np(s.smoothed_covariances), ref["smoothed_covariances"]))
        print(label, (n, m), [f"{v:.2e}" for v in e])
        assert max(e) < TOL_SMOOTHED, (label, e)
    noise = torch.randn((B, S, T, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    xs = bfa.kalman_posterior_sample(p, c["gapped"], S, None, noise=noise, initial_means=c["init"], missing="nan")
    assert tuple(xs.shape) == (B, S, T, n) and bool(torch.isfinite(xs).all())
    want = bfa.posterior_sample(p, _kf(c, fields=("means", "covariances")), S, noise=noise)
    assert torch.equal(xs, want)
