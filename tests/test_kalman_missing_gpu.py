"""The Kalman filter with missing observations on the MI355X (``kalman_filter(..., missing="nan")`` /
``bf_kalman_filter_missing_f32``) against the float64 reference of tests/kalman_missing_cases.py, on every data path of the
register kernel: both emitters and the tail launch, the batch-inner layout, per-step Q / R, the carry, and the backward passes
that run on the gapped posterior.

Tolerances are those of tests/test_kalman_gpu.py for the same streams (norm-wise 1e-5, 2e-5 for the log-likelihood) and of
tests/test_smoother_gpu.py for the smoothed ones (1e-5)."""
import numpy as np
import pytest

from tests import common as cm
from tests import kalman_missing_cases as kc

pytestmark = pytest.mark.gpu
TOL, TOL_LL, TOL_SMOOTHED = 1e-5, 2e-5, 1e-5
F32 = np.float32


def _np(x):
    return x.detach().cpu().numpy()


def _staged_eligible(n, T):
    """The staged emitter takes the reference layout when the rows of the vector and matrix streams are 16-byte aligned
    (launch_nml: rows_aligned); elsewhere kf_emit_mode = 2 is refused and the default route is the strided kernel."""
    return (T * n) % 4 == 0 and (T * n * n) % 4 == 0


def _run(c, ys=None, mode=-1, layout="reference", **kw):
    import bayesianfiltering_amd as bfa
    kw.setdefault("initial_means", c["init"])
    kw.setdefault("missing", "nan")
    return bfa.kalman_filter(cm.product_params(c["a"]), c["gapped"] if ys is None else ys, layout=layout,
                             options={"kf_emit_mode": mode}, **kw)


def _assert_streams(post, ll, ref, label):
    errs = {k: cm.rel_err(_np(getattr(post, k)), ref[k]) for k in kc.STREAMS}
    errs["loglik"] = cm.rel_err(_np(ll), ref["loglik"])
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k in kc.STREAMS:
        assert _np(getattr(post, k)).shape == ref[k].shape, (label, k)
        assert errs[k] < TOL, (label, k, errs[k])
    assert errs["loglik"] < TOL_LL, (label, errs["loglik"])


def _assert_same_bits(x, y, label):
    for k in kc.STREAMS:
        assert np.array_equal(_np(getattr(x[0], k)), _np(getattr(y[0], k)), equal_nan=True), (label, k)
    assert np.array_equal(_np(x[1]), _np(y[1]), equal_nan=True), (label, "loglik")


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", kc.HORIZONS)
@pytest.mark.parametrize("B", kc.BATCHES)
@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_streams_loglik_and_carry_match_the_reference_on_every_route(n, m, B, T):
    c = kc.case(n, m, B, T)
    ref = c["ref"]
    staged = _staged_eligible(n, T)
    runs = {"staged" if staged else "default": _run(c, mode=2 if staged else -1, return_loglik=True, return_carry=True),
            "strided": _run(c, mode=0, return_loglik=True, return_carry=True),
            "batch_inner": _run(c, layout="batch_inner", return_loglik=True, return_carry=True)}
    for label, (post, ll, carry) in runs.items():
        _assert_streams(post, ll, ref, (n, m, B, T, label))
        for got, want, name in zip(carry, ref["carry"], ("w", "m", "P")):
            assert _np(got).shape == want.shape and cm.rel_err(_np(got), want) < TOL, (label, "carry", name)
    first = next(iter(runs.values()))
    for label in ("strided", "batch_inner"):
        _assert_same_bits(first, runs[label], (n, m, B, T, label))
        for x, y in zip(first[2], runs[label][2]):
            assert np.array_equal(_np(x), _np(y)), (label, "carry")
    # the gaps themselves: a step with nothing observed is predict-only, exactly
    post, ll, _ = first
    m_f, P_f, m_p, P_p, lls = (_np(v)[:, 0] for v in (post.means, post.covariances, post.predicted_means,
                                                     post.predicted_covariances, ll))
    empty = ~c["mask"].any(axis=2)                                 # (B, T)
    bs, ts = np.nonzero(empty[:, 1:])
    assert len(ts) >= kc.FORECAST                                  # the forecast tail at least
    assert np.array_equal(m_f[bs, ts + 1], m_p[bs, ts]) and np.array_equal(P_f[bs, ts + 1], P_p[bs, ts])
    assert (lls[empty] == 0.0).all() and (lls[~empty] != 0.0).all()
    if B > kc.NONE:
        assert (lls[kc.NONE] == 0.0).all() and (_np(post.weights)[kc.NONE] == 1.0).all()
    assert (_np(post.weights) == 1.0).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,mode", [(5, -1), (37, 2)])
def test_per_step_covariances(B, mode):
    """Q_t and R_t tables at (4, 2): B = 5 is less than a wave (the strided kernel), B = 37 one whole wave on the staged
    kernel and a tail of 5."""
    c = kc.case(4, 2, B, 64, True)
    post, ll = _run(c, mode=mode, return_loglik=True)
    _assert_streams(post, ll, c["ref"], ("tv", B, mode))
    _assert_same_bits((post, ll), _run(c, mode=0, return_loglik=True), ("tv", B, "strided"))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(4, 2), (8, 4)])
def test_chunks_through_the_carry_inside_a_gap_are_bit_exact(n, m):
    B, T = 37, 64
    c = kc.case(n, m, B, T)
    cut = T // 2                                                   # the wholly missing step: the second chunk starts in the gap
    assert not c["mask"][0, cut].any() and not c["mask"][0, T - 1].any()
    whole = _run(c, return_loglik=True, return_carry=True)
    for cuts in ((cut,), (cut + 1,), (T - 3,), (7, cut)):          # ... ends in it, inside the forecast tail, three chunks
        parts, carry, t0 = [], None, 0
        for t1 in cuts + (T,):
            kw = dict(initial_means=c["init"]) if carry is None else dict(carry=carry, initial_means=None)
            post, ll, carry = _run(c, ys=c["gapped"][:, t0:t1], return_loglik=True, return_carry=True, **kw)
            parts.append((post, ll))
            t0 = t1
        for k in kc.STREAMS:
            glued = np.concatenate([_np(getattr(p, k)) for p, _ in parts], axis=2)
            assert np.array_equal(glued, _np(getattr(whole[0], k))), (cuts, k)
        assert np.array_equal(np.concatenate([_np(l) for _, l in parts], axis=2), _np(whole[1])), cuts
        for x, y in zip(carry, whole[2]):
            assert np.array_equal(_np(x), _np(y)), (cuts, "carry")


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_a_trajectorys_bits_do_not_depend_on_its_neighbours_gaps(n, m):
    """Lanes with different patterns share a wave (and, at m >= 2, the selects of one instruction stream): the same
    trajectory next to fully observed neighbours, next to unobserved ones, and in another position of the batch."""
    B, T = 37, 19
    c = kc.case(n, m, B, T)
    base = _run(c, return_loglik=True)
    probe = 5                                                      # a trajectory with the random pattern
    for fill, position in ((c["ys"], probe), (np.full_like(c["ys"], np.nan), probe), (c["ys"], 20)):
        ys = np.array(fill)
        ys[position] = c["gapped"][probe]
        init = np.array(c["init"])
        init[position] = c["init"][probe]
        post, ll = _run(c, ys=ys, initial_means=init, return_loglik=True)
        for k in kc.STREAMS:
            assert np.array_equal(_np(getattr(post, k))[position], _np(getattr(base[0], k))[probe]), k
        assert np.array_equal(_np(ll)[position], _np(base[1])[probe])


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_complete_data_through_the_missing_route_is_the_plain_filter(n, m):
    """Same tolerance as against the reference.  Whether the bits agree too is reported, not required: the run-time |o| of
    the log 2 pi term may be contracted differently from the plain kernel's constant."""
    import bayesianfiltering_amd as bfa
    B, T = 37, 64
    c = kc.case(n, m, B, T)
    p = cm.product_params(c["a"])
    plain, ll0 = bfa.kalman_filter(p, c["ys"], initial_means=c["init"], return_loglik=True)
    post, ll = _run(c, ys=c["ys"], return_loglik=True)
    same = all(np.array_equal(_np(getattr(post, k)), _np(getattr(plain, k))) for k in kc.STREAMS)
    print(f"(n, m) = ({n}, {m}): streams bit-equal to the plain filter: {same}; log-likelihood: {np.array_equal(_np(ll), _np(ll0))}")
    for k in kc.STREAMS:
        assert cm.rel_err(_np(getattr(post, k)), _np(getattr(plain, k))) < TOL, k
    assert cm.rel_err(_np(ll), _np(ll0)) < TOL_LL


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [s for s in kc.SHAPES if s[1] >= 2])
def test_a_never_observed_component_is_the_row_reduced_model(n, m):
    import bayesianfiltering_amd as bfa
    B, T = 37, 64
    c = kc.case(n, m, B, T)
    b = kc.NO_COMP1
    assert not c["mask"][b, :, 1].any() and np.delete(c["mask"][b], 1, axis=1).all()
    keep = [i for i in range(m) if i != 1]
    reduced = cm.product_params(kc.row_reduced(c["a"], keep))
    want, ll0 = bfa.kalman_filter(reduced, c["ys"][b:b + 1][:, :, keep], initial_means=c["init"][b:b + 1], return_loglik=True)
    post, ll = _run(c, return_loglik=True)
    for k in kc.STREAMS:
        assert cm.rel_err(_np(getattr(post, k))[b:b + 1], _np(getattr(want, k))) < TOL, k
    assert cm.rel_err(_np(ll)[b:b + 1], _np(ll0)) < TOL_LL


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(4, 2), (3, 3)])
def test_inf_is_not_missing(n, m):
    """+-Inf in an observed component poisons that trajectory from that step on, as in the plain filter, and only it: the
    weight is NaN and the mean is not finite at every later step, the log-likelihood is not finite wherever the step observes
    something (a wholly missing step keeps its contractual 0), the covariances read no data and stay finite."""
    B, T, tb, bb = 37, 19, 6, 7
    c = kc.case(n, m, B, T)
    clean = _run(c, return_loglik=True)
    for value, comp in ((np.inf, 0), (-np.inf, m - 1)):
        ys = np.array(c["gapped"])
        ys[bb, tb, comp] = value                                   # whatever the mask said: this entry is now observed
        post, ll = _run(c, ys=ys, return_loglik=True)
        mm, lls, w = _np(post.means), _np(ll), _np(post.weights)
        seen = ~np.isnan(ys[bb, tb:]).all(axis=1)
        assert np.isnan(w[bb, 0, tb:]).all() and (~np.isfinite(mm[bb, 0, tb:])).any(axis=1).all()
        assert seen[0] and (~np.isfinite(lls[bb, 0, tb:][seen])).all() and (lls[bb, 0, tb:][~seen] == 0.0).all()
        assert np.isfinite(_np(post.covariances)).all()
        others = np.arange(B) != bb
        for k in kc.STREAMS:
            got, want = _np(getattr(post, k)), _np(getattr(clean[0], k))
            assert np.array_equal(got[others], want[others]) and np.array_equal(got[bb, 0, :tb], want[bb, 0, :tb]), k
        assert np.array_equal(lls[others], _np(clean[1])[others])


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(4, 2), (8, 4)])
def test_smoothers_on_the_gapped_posterior(n, m):
    import bayesianfiltering_amd as bfa
    B, T = 37, 64
    c = kc.case(n, m, B, T)
    p = cm.product_params(c["a"])
    ref = c["ref"]
    sm = bfa.rts_smoother(p, _run(c))
    via_kw = bfa.kalman_smoother(p, c["gapped"], initial_means=c["init"], missing="nan")
    via_mask = bfa.kalman_smoother(p, c["ys"], initial_means=c["init"], observed=c["mask"])
    for label, s in (("rts_smoother", sm), ("kalman_smoother", via_kw), ("observed=", via_mask)):
        e = (cm.rel_err(_np(s.smoothed_means), ref["smoothed_means"]),
             cm.rel_err(_np(s.smoothed_covariances), ref["smoothed_covariances"]))
        print(label, (n, m), [f"{v:.2e}" for v in e])
        assert max(e) < TOL_SMOOTHED, (label, e)
    assert np.array_equal(_np(via_kw.smoothed_means), _np(via_mask.smoothed_means))
    assert np.array_equal(_np(via_kw.smoothed_covariances), _np(via_mask.smoothed_covariances))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_posterior_samples_on_the_gapped_posterior():
    import torch
    import bayesianfiltering_amd as bfa
    n, m, B, T, S = 4, 2, 37, 64, 3
    c = kc.case(n, m, B, T)
    p = cm.product_params(c["a"])
    ys = torch.as_tensor(c["ys"], device="cuda")
    before = ys.clone()
    noise = torch.randn((B, S, T, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    xs = bfa.kalman_posterior_sample(p, ys, S, None, noise=noise, initial_means=c["init"], observed=c["mask"])
    assert torch.equal(ys, before)                                  # the mask went into a copy
    assert tuple(xs.shape) == (B, S, T, n) and bool(torch.isfinite(xs).all())
    post = _run(c, fields=("means", "covariances"))
    want = bfa.posterior_sample(p, post, S, noise=noise)
    assert torch.equal(xs, want)


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_observed_mask_forms_and_single_trajectory():
    """``observed=`` in its four shapes equals ``missing="nan"`` on the NaN-filled copy bit for bit; one trajectory (T, m)
    comes back without the batch axis; ``fields`` and ``out=`` behave as in the plain filter."""
    import bayesianfiltering_amd as bfa
    n, m, B, T = 4, 2, 37, 19
    c = kc.case(n, m, B, T)
    p = cm.product_params(c["a"])
    rng = np.random.default_rng(2)
    for shape in ((T,), (B, T), (T, m), (B, T, m)):
        mk = rng.random(shape) > 0.3
        full = np.broadcast_to(mk.reshape({(T,): (1, T, 1), (B, T): (B, T, 1), (T, m): (1, T, m)}.get(shape, shape)), (B, T, m))
        a = bfa.kalman_filter(p, c["ys"], initial_means=c["init"], observed=mk, return_loglik=True)
        b = bfa.kalman_filter(p, kc.gapped(c["ys"], full), initial_means=c["init"], missing="nan", return_loglik=True)
        _assert_same_bits(a, b, shape)
    one = bfa.kalman_filter(p, c["gapped"][0], initial_means=c["init"][:1], missing="nan", fields=("means", "covariances"))
    assert tuple(one.means.shape) == (1, T, n) and one.weights is None and one.predicted_means is None
    whole = _run(c)
    assert np.array_equal(_np(one.means), _np(whole.means)[0]) and np.array_equal(_np(one.covariances), _np(whole.covariances)[0])
    again = _run(c, out=whole)
    assert again.means.data_ptr() == whole.means.data_ptr()
    with pytest.raises(ValueError, match="observed must have shape"):
        bfa.kalman_filter(p, c["ys"], observed=np.ones((T + 1,), bool))
