"""Missing observations on the run-time-dimension kernel on the MI355X (``kalman_filter(..., missing="nan")`` and
``gaussian_sum_filter(..., missing="nan")`` beyond the register kernels, or with ``options={"force_generic": 1}``;
``bf_kalman_filter_missing_anydim_f32`` / ``bf_gsf_ekf_missing_anydim_f32``): against the float64 contract of
tests/kalman_missing_cases.py and the compacted float32 reference of tests/gsf_missing_cases.py, at the shapes of
tests/generic_missing_cases.py -- n, m and m > n past the register limits, the 256-thread workgroup, K > 1, the state-dependent
noise Jacobian, models from source.

Tolerances are the project's: norm-wise 1e-5 for the streams, 2e-5 for the log-likelihood, 1e-5 for the smoothed streams
(tests/test_kalman_missing_gpu.py); the Gaussian-sum cases are held to ``gsf_missing_cases.bounds``, which
tests/test_generic_missing_cpu.py shows to be the standard 1e-5 / 2e-5 (weights) at these cases."""
import numpy as np
import pytest

from tests import common as cm
from tests import generic_missing_cases as xc
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc

pytestmark = pytest.mark.gpu
TOL, TOL_LL, TOL_SMOOTHED = 1e-5, 2e-5, 1e-5
F32 = np.float32
T = xc.T
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
    return bfa.gaussian_sum_filter(c["pp"] if pp is None else pp, c["gapped"] if ys is None else ys, c["K"], 1, c["inputs"], **kw)


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


def _assert_same_bits(x, y, label, loglik=True):
    for k in kc.STREAMS:
        assert np.array_equal(_np(getattr(x[0], k)), _np(getattr(y[0], k)), equal_nan=True), (label, k)
    if loglik:
        assert np.array_equal(_np(x[1]), _np(y[1]), equal_nan=True), (label, "loglik")


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
@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("n,m", xc.KALMAN_SHAPES)
def test_kalman_shapes_match_the_float64_contract(n, m, B):
    """The test that fails without the feature: these calls used to be refused (n > 8, m > 4 or m > n)."""
    c = xc.kalman_case(n, m, B, T)
    post, ll, carry = _kf(c, return_loglik=True, return_carry=True)
    _assert_streams(post, ll, c["ref"], (n, m, B))
    for got, want, name in zip(carry, c["ref"]["carry"], ("w", "m", "P")):
        assert _np(got).shape == want.shape and cm.rel_err(_np(got), want) < TOL, ("carry", name)
    _assert_gap_identities(post, ll, c["mask"])
    if B > kc.NONE:
        assert (_np(ll)[kc.NONE] == 0.0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(9, 2), (33, 6)])
def test_complete_data_is_the_plain_generic_kernel_bit_for_bit(n, m):
    import bayesianfiltering_amd as bfa
    c = xc.kalman_case(n, m, 5, T)
    plain = bfa.kalman_filter(cm.product_params(c["a"]), c["ys"], initial_means=c["init"], options=GENERIC, return_loglik=True,
                              return_carry=True)
    new = _kf(c, ys=c["ys"], return_loglik=True, return_carry=True)
    _assert_same_bits(new, plain, (n, m), loglik=False)
    for x, y in zip(new[2], plain[2]):
        assert np.array_equal(_np(x), _np(y)), "carry"
    print((n, m), "log-likelihood bit-equal to the plain kernel:", np.array_equal(_np(new[1]), _np(plain[1])))
    assert cm.rel_err(_np(new[1]), _np(plain[1])) < TOL_LL


def test_complete_data_is_the_plain_generic_kernel_bit_for_bit_gaussian_sum():
    c = xc.gsf_case("l96")
    plain = _gsf(c, ys=c["ys"], missing=None, options=GENERIC, return_loglik=True, return_carry=True)
    new = _gsf(c, ys=c["ys"], return_loglik=True, return_carry=True)
    _assert_same_bits(new, plain, "l96", loglik=False)
    for x, y in zip(new[2], plain[2]):
        assert np.array_equal(_np(x), _np(y)), "carry"
    print("l96: log-likelihood bit-equal to the plain kernel:", np.array_equal(_np(new[1]), _np(plain[1])))
    assert cm.rel_err(_np(new[1]), _np(plain[1])) < TOL_LL


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", xc.KALMAN_SHAPES)
def test_a_never_observed_component_is_the_row_reduced_model_on_the_plain_kernel(n, m):
    import bayesianfiltering_amd as bfa
    c = xc.kalman_case(n, m, 5, T)
    b = kc.NO_COMP1
    assert not c["mask"][b, :, 1].any() and np.delete(c["mask"][b], 1, axis=1).all()
    keep = [i for i in range(m) if i != 1]
    reduced = cm.product_params(kc.row_reduced(c["a"], keep))
    want, ll0 = bfa.kalman_filter(reduced, c["ys"][b:b + 1][:, :, keep], initial_means=c["init"][b:b + 1], options=GENERIC,
                                  return_loglik=True)
    post, ll = _kf(c, return_loglik=True)
    e = {k: cm.rel_err(_np(getattr(post, k))[b:b + 1], _np(getattr(want, k))) for k in kc.STREAMS}
    e["loglik"] = cm.rel_err(_np(ll)[b:b + 1], _np(ll0))
    print((n, m), "largest difference from the row-reduced model:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e[k] for k in kc.STREAMS) < TOL and e["loglik"] < TOL_LL, e


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_small_model_agrees_with_the_register_route():
    c = kc.case(4, 2, 5, T)
    reg = _kf(c, return_loglik=True)
    gen = _kf(c, return_loglik=True, options=GENERIC)
    _assert_streams(gen[0], gen[1], c["ref"], "(4, 2) force_generic")
    for k in kc.STREAMS:
        assert cm.rel_err(_np(getattr(gen[0], k)), _np(getattr(reg[0], k))) < TOL, k
    assert cm.rel_err(_np(gen[1]), _np(reg[1])) < TOL_LL
    _assert_gap_identities(gen[0], gen[1], c["mask"])


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def _chunked(run, ys, init, cuts, Tn):
    parts, carry, t0 = [], None, 0
    for t1 in cuts + (Tn,):
        kw = dict(initial_means=init) if carry is None else dict(carry=carry, initial_means=None)
        post, ll, carry = run(ys[:, t0:t1], **kw)
        parts.append((post, ll))
        t0 = t1
    return parts, carry


@pytest.mark.parametrize("n,m", [(9, 2), (33, 6)])
def test_chunks_through_the_carry_inside_a_gap_are_bit_exact(n, m):
    c = xc.kalman_case(n, m, 5, T)
    cut = T // 2                                                   # the wholly missing step: the second chunk starts in the gap
    assert not c["mask"][0, cut].any()
    whole = _kf(c, return_loglik=True, return_carry=True)
    run = lambda ys, **kw: _kf(c, ys=ys, return_loglik=True, return_carry=True, **kw)
    for cuts in ((cut,), (cut + 1,), (T - 3,)):                    # ... ends in it, inside the forecast tail
        parts, carry = _chunked(run, c["gapped"], c["init"], cuts, T)
        for k in kc.STREAMS:
            assert np.array_equal(np.concatenate([_np(getattr(p, k)) for p, _ in parts], axis=2), _np(getattr(whole[0], k))), (cuts, k)
        assert np.array_equal(np.concatenate([_np(l) for _, l in parts], axis=2), _np(whole[1])), cuts
        for x, y in zip(carry, whole[2]):
            assert np.array_equal(_np(x), _np(y)), (cuts, "carry")


def test_chunks_through_the_carry_inside_a_gap_are_bit_exact_gaussian_sum():
    c = xc.gsf_case("l96")
    cut = T // 2
    assert not c["mask"][0, cut].any()
    whole = _gsf(c, return_loglik=True, return_carry=True)
    run = lambda ys, **kw: _gsf(c, ys=ys, return_loglik=True, return_carry=True, **kw)
    parts, carry = _chunked(run, c["gapped"], c["init"], (cut,), T)
    for k in kc.STREAMS:
        assert np.array_equal(np.concatenate([_np(getattr(p, k)) for p, _ in parts], axis=2), _np(getattr(whole[0], k))), k
    assert np.array_equal(np.concatenate([_np(l) for _, l in parts], axis=2), _np(whole[1]))
    for x, y in zip(carry, whole[2]):
        assert np.array_equal(_np(x), _np(y)), "carry"


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(9, 2), (33, 6)])
def test_a_trajectorys_bits_do_not_depend_on_its_neighbours_gaps(n, m):
    c = xc.kalman_case(n, m, 5, T)
    base = _kf(c, return_loglik=True)
    probe = 0                                                      # a trajectory with the random pattern
    for fill, position in ((c["ys"], probe), (np.full_like(c["ys"], np.nan), probe), (c["ys"], 4)):
        ys = np.array(fill)
        ys[position] = c["gapped"][probe]
        init = np.array(c["init"])
        init[position] = c["init"][probe]
        post, ll = _kf(c, ys=ys, initial_means=init, return_loglik=True)
        for k in kc.STREAMS:
            assert np.array_equal(_np(getattr(post, k))[position], _np(getattr(base[0], k))[probe]), k
        assert np.array_equal(_np(ll)[position], _np(base[1])[probe])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_observed_mask_forms_equal_the_nan_form():
    n, m, B = 9, 2, 5
    c = xc.kalman_case(n, m, B, T)
    rng = np.random.default_rng(2)
    for shape in ((T,), (B, T), (T, m), (B, T, m)):
        mk = rng.random(shape) > 0.3
        full = np.broadcast_to(mk.reshape({(T,): (1, T, 1), (B, T): (B, T, 1), (T, m): (1, T, m)}.get(shape, shape)), (B, T, m))
        a = _kf(c, ys=c["ys"], observed=mk, return_loglik=True)
        b = _kf(c, ys=kc.gapped(c["ys"], full), return_loglik=True)
        _assert_same_bits(a, b, shape)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_per_step_covariances():
    c = xc.kalman_case(9, 2, 5, T, True)
    post, ll = _kf(c, return_loglik=True)
    _assert_streams(post, ll, c["ref"], "tv (9, 2)")


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_inf_is_not_missing_and_nan_poisons_without_the_keyword():
    import bayesianfiltering_amd as bfa
    n, m, B, tb, bb = 9, 2, 5, 6, 3
    c = xc.kalman_case(n, m, B, T)
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


# 10 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l96", "sv"])
def test_gaussian_sum_cases_match_the_compacted_reference(name):
    c = xc.gsf_case(name)
    bound, _ = xc.gsf_bounds(name)
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


def test_what_the_model_computes_for_a_missing_row_does_not_leak():
    """svleak: the last state starts at 1e3, where exp(x / sigma) overflows, so the last row of h, H_x and H_r R H_r^T is not
    finite (tests/test_generic_missing_cpu.py shows it); that row is never observed and that state is coupled to nothing.
    Everything the other states produce is finite and equals, bit for bit, the run in which the last state starts at 0.3."""
    c = xc.gsf_case("svleak")
    n = 9
    yg = np.array(c["gapped"])
    yg[:, :, n - 1] = np.nan
    runs = []
    for x_last in (1e3, 0.3):
        init = np.array(c["init"])
        init[:, :, n - 1] = x_last
        runs.append(_gsf(c, ys=yg, initial_means=init, return_loglik=True))
    (hot, ll_hot), (cool, ll_cool) = runs
    assert np.isfinite(_np(ll_hot)).all() and np.array_equal(_np(ll_hot), _np(ll_cool))
    assert np.array_equal(_np(hot.weights), _np(cool.weights)) and np.isfinite(_np(hot.weights)).all()
    for k in ("means", "predicted_means"):
        a, b = _np(getattr(hot, k)), _np(getattr(cool, k))
        assert np.isfinite(a).all() and np.array_equal(a[..., :n - 1], b[..., :n - 1]), k
    for k in ("covariances", "predicted_covariances"):
        a, b = _np(getattr(hot, k)), _np(getattr(cool, k))
        assert np.isfinite(a).all() and np.array_equal(a[..., :n - 1, :n - 1], b[..., :n - 1, :n - 1]), k
    assert (_np(ll_hot)[:, :, 1:T - kc.FORECAST] != 0).any()         # the other rows were conditioned on


# 11 --------------------------------------------------------------------------------------------------------------------------------
def test_from_source_matches_the_reference_and_its_plain_route():
    c = xc.gsf_case("l96src")
    bound, _ = xc.gsf_bounds("l96src")
    post, ll = _gsf(c, return_loglik=True)
    e = _errs(post, ll, c["ref"])
    e["weights"] = float(np.abs(_np(post.weights).astype(np.float64) - c["ref"]["weights"]).max())
    print("l96 from source", {k: f"{v:.2e}" for k, v in e.items()})
    for k, v in e.items():
        assert v < bound[k], (k, v, bound[k])
    _assert_gap_identities(post, ll, c["mask"], c["K"])
    # complete data: the twin built at run time equals the handle's plain kernel bit for bit
    plain = _gsf(c, ys=c["ys"], missing=None, return_loglik=True, return_carry=True)
    new = _gsf(c, ys=c["ys"], return_loglik=True, return_carry=True)
    _assert_same_bits(new, plain, "l96 from source", loglik=False)
    for x, y in zip(new[2], plain[2]):
        assert np.array_equal(_np(x), _np(y)), "carry"
    assert cm.rel_err(_np(new[1]), _np(plain[1])) < TOL_LL


def test_a_recorded_python_function_at_n_9():
    """The linear (9, 2) model written as plain Python functions of NumPy operations: recorded, compiled at run time with the
    gapped twin, and held to the float64 contract of the Kalman case."""
    import bayesianfiltering_amd as bfa
    n, m, B = 9, 2, 5
    c = xc.kalman_case(n, m, B, T)
    a = c["a"]
    A, G, H, D = (np.asarray(a[k], F32) for k in ("A", "G", "H", "D"))
    f = lambda x, q, u: A @ x + G @ q
    h = lambda x, r, u: H @ x + D @ r
    p = bfa.ParamsNLSSM(a["m0"], a["P0"], f, a["q0"], a["Q"], h, a["r0"], a["R"])
    post, ll = bfa.gaussian_sum_filter(p, c["gapped"], 1, initial_means=c["init"].reshape(B, 1, n), missing="nan", return_loglik=True)
    _assert_streams(post, ll, c["ref"], "recorded (9, 2)")
    _assert_gap_identities(post, ll, c["mask"])


# 12 --------------------------------------------------------------------------------------------------------------------------------
def test_backward_passes_on_the_gapped_posterior():
    import torch
    import bayesianfiltering_amd as bfa
    n, m, B, S = 9, 2, 5, 3
    c = xc.kalman_case(n, m, B, T)
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


def test_nonlinear_backward_passes_at_n_12():
    """The extended smoother and the Gaussian-sum smoother / sampler wrappers pass the keywords on: finite results of the right
    shape on the gapped Lorenz-96 posterior (their arithmetic is covered by their own tests; a backward pass reads no observation)."""
    import bayesianfiltering_amd as bfa
    c = xc.gsf_case("l96")
    B, K, n = c["init"].shape
    s1 = bfa.extended_kalman_smoother(c["pp"], c["gapped"], initial_means=c["init"][:, :1], missing="nan")
    assert tuple(s1.smoothed_means.shape) == (B, 1, T, n) and np.isfinite(_np(s1.smoothed_means)).all()
    sK = bfa.extended_gaussian_sum_smoother(c["pp"], c["gapped"], K, initial_means=c["init"], missing="nan")
    assert np.isfinite(_np(sK.smoothed_means)).all() and tuple(sK.smoothed_means.shape) == (B, K, T, n)
    xs = bfa.extended_gaussian_sum_posterior_sample(c["pp"], c["gapped"], K, 2, bfa.PRNGKey(1), initial_means=c["init"], missing="nan")
    assert np.isfinite(_np(xs)).all() and tuple(xs.shape)[-2:] == (T, n)
