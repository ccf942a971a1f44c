"""RTS smoother on the MI355X: parity with the float64 oracle of tests/test_smoother_cpu.py (itself pinned to the dense
joint Gaussian), bit-for-bit agreement of the data paths, chunking through the carry, every dimension, extended
dynamics."""
import os

import numpy as np
import pytest

from tests import common as cm
from tests.test_smoother_cpu import kalman_f64, rts_f64, dense_posterior

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np(x):
    return x.detach().cpu().numpy()


def _oracle(post, F, inputs_F=None):
    """float64 RTS over the GPU's own fp32 filtered streams, trajectory by trajectory (posterior arrays (B, 1, T, ...))."""
    m, P, pm, pP = (_np(getattr(post, k))[:, 0] for k in ("means", "covariances", "predicted_means", "predicted_covariances"))
    out = [rts_f64(m[b], P[b], pm[b], pP[b], F if inputs_F is None else inputs_F(b, m[b])) for b in range(m.shape[0])]
    return tuple(np.stack([o[i] for o in out])[:, None] for i in range(3))


def _check(sm, ref, tol=1e-5, name=""):
    ms, Ps, Cs = ref
    e = (cm.rel_err(_np(sm.smoothed_means), ms), cm.rel_err(_np(sm.smoothed_covariances), Ps))
    if sm.smoothed_cross_covariances is not None:
        e += (cm.rel_err(_np(sm.smoothed_cross_covariances), Cs[:, :, :-1]),)
    cm.record("smoother" + name, errs=list(e))
    assert max(e) < tol, (name, e)


def _filter(a, B, T, seed, layout="reference", fields=None):
    import bayesianfiltering_amd as bfa
    ys = cm.simulate_batch(a, B, T, seed=seed)
    post = bfa.kalman_filter(cm.product_params(a), ys, initial_means=np.tile(a["m0"], (B, 1)), layout=layout,
                             **({"fields": fields} if fields else {}))
    return ys, post


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kalman_cv_n4_m2_T64", "kalman_random_n3_m3_T40"])
def test_fixture_streams_parity(name):
    import torch
    import bayesianfiltering_amd as bfa
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    a = {k: d[k] for k in ("A", "G", "H", "D", "Q", "R", "m0", "P0", "q0", "r0")}
    dev = lambda k: torch.as_tensor(d["out_" + k], device="cuda")
    post = bfa.PosteriorGaussianSumFiltered(None, dev("means"), dev("covariances"), dev("predicted_means"),
                                            dev("predicted_covariances"))
    sm = bfa.rts_smoother(cm.product_params(a), post, cross_covariances=True)
    torch.cuda.synchronize()
    _check(sm, _oracle(post, a["A"]), name=name)


# 2 -----------------------------------------------------------------------------------------------------------------
def test_kalman_smoother_vs_exact_posterior():
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=21, bias=True)
    B, T = 6, 16
    ys = cm.simulate_batch(a, B, T, seed=5)
    sm = bfa.kalman_smoother(cm.product_params(a), ys, initial_means=np.tile(a["m0"], (B, 1)), cross_covariances=True)
    for b in range(B):
        dm, dP, dC = dense_posterior(a, ys[b].astype(np.float64), a["m0"], a["P0"])
        e = (cm.rel_err(_np(sm.smoothed_means[b, 0]), dm), cm.rel_err(_np(sm.smoothed_covariances[b, 0]), dP),
             cm.rel_err(_np(sm.smoothed_cross_covariances[b, 0]), dC))
        # the filter's gain carries the reference's +1e-6 on every entry of S (gaussfiltax/utils.py:258)
        assert max(e) < 1e-4, (b, e)


# 3 -----------------------------------------------------------------------------------------------------------------
def test_last_step_and_chunks_bit_for_bit():
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    B, T, s = 128, 72, 40
    _, post = _filter(a, B, T, seed=3)
    p = cm.product_params(a)
    full = bfa.rts_smoother(p, post, cross_covariances=True)
    assert np.array_equal(_np(full.smoothed_means[:, :, -1]), _np(post.means[:, :, -1]))
    assert np.array_equal(_np(full.smoothed_covariances[:, :, -1]), _np(post.covariances[:, :, -1]))
    cut = lambda lo, hi: post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in
                                          ("means", "covariances", "predicted_means", "predicted_covariances")})
    late, carry = bfa.rts_smoother(p, cut(s, T), cross_covariances=True, return_carry=True)
    early = bfa.rts_smoother(p, cut(0, s), carry=carry, cross_covariances=True)
    for k in ("smoothed_means", "smoothed_covariances"):
        joined = np.concatenate([_np(getattr(early, k)), _np(getattr(late, k))], axis=2)
        assert np.array_equal(joined, _np(getattr(full, k))), k
    C = np.concatenate([_np(early.smoothed_cross_covariances), _np(late.smoothed_cross_covariances)], axis=2)
    assert np.array_equal(C, _np(full.smoothed_cross_covariances))
    assert np.array_equal(_np(carry.means), _np(late.smoothed_means[:, 0, 0]))


# 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,B", [(4, 2, 128), (4, 2, 130), (2, 1, 192), (3, 2, 70), (1, 1, 64)])
def test_layouts_and_paths_bit_for_bit(n, m, B):
    import torch
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays() if n == 4 else cm.random_stable_lgssm(n, m, seed=n)
    T = 24
    ys, post = _filter(a, B, T, seed=9)
    p = cm.product_params(a)
    staged = bfa.rts_smoother(p, post, cross_covariances=True, options={"rts_load_mode": 2})
    ref = [_np(x) for x in staged[2:]]
    runs = {"strided": bfa.rts_smoother(p, post, cross_covariances=True, options={"rts_load_mode": 0})}
    _, post_bi = _filter(a, B, T, seed=9, layout="batch_inner")
    runs["batch_inner"] = bfa.rts_smoother(p, post_bi, cross_covariances=True, layout="batch_inner")
    # a stride set neither layout has: every stream a slice of a longer buffer
    wide = {k: torch.zeros((B, 1, T + 3) + tuple(getattr(post, k).shape[3:]), device="cuda")[:, :, 1:T + 1]
            for k in ("means", "covariances", "predicted_means", "predicted_covariances")}
    for k, v in wide.items():
        v.copy_(getattr(post, k))
    runs["odd_strides"] = bfa.rts_smoother(p, post._replace(**wide), cross_covariances=True)
    for name, r in runs.items():
        for x, y in zip(ref, r[2:]):
            assert np.array_equal(x, _np(y)), name
    _check(staged, _oracle(post, a["A"]), name=f"layouts_n{n}_B{B}")


# 5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tv", [False, True])
def test_recompute_path(tv):
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=33, dq=3, bias=True)
    B, T = 96, 32
    if tv:
        rng = np.random.default_rng(1)
        a["Q"] = np.stack([a["Q"] * F32(0.5 + rng.random()) for _ in range(T)]).astype(F32)
    ys = cm.simulate_batch(dict(a, Q=a["Q"][0] if tv else a["Q"]), B, T, seed=2)
    p = cm.product_params(a)
    post = bfa.kalman_filter(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
    with_pred = bfa.rts_smoother(p, post, cross_covariances=True)
    without = bfa.rts_smoother(p, post._replace(predicted_means=None, predicted_covariances=None), cross_covariances=True)
    for x, y in zip(with_pred[2:], without[2:]):
        assert cm.rel_err(_np(y), _np(x)) <= 1e-6
    ks = bfa.kalman_smoother(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
    assert np.array_equal(_np(ks.smoothed_means), _np(without.smoothed_means))


# 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 12, 24, 48])
def test_every_dimension(n):
    import bayesianfiltering_amd as bfa
    m = min(n, 2)
    a = cm.random_stable_lgssm(n, m, seed=40 + n)
    B, T = 70, 20
    _, post = _filter(a, B, T, seed=n)
    p = cm.product_params(a)
    ref = _oracle(post, a["A"])
    _check(bfa.rts_smoother(p, post, cross_covariances=True), ref, name=f"n{n}")
    if n <= 8:
        _check(bfa.rts_smoother(p, post, cross_covariances=True, options={"force_generic": 1}), ref, name=f"n{n}_generic")


# 7 -----------------------------------------------------------------------------------------------------------------
def _ext_case(kind):
    import bayesianfiltering_amd as bfa
    from oracle import models as om
    nl = bfa.nonlinearities
    rng = np.random.default_rng(17)
    B, T = 66, 24
    u = None
    if kind == "lorenz63":
        n, f, fo = 3, nl.lorenz63(), om.Lorenz63()
        m0, Q, R = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32), 0.5 * np.eye(3, dtype=F32)
    elif kind == "sine":
        n, f, fo = 2, nl.sine(2, w0=1.0), om.Sine(2, w0=1.0)
        m0, Q, R = np.array([0.3, -0.2], F32), 1e-1 * np.eye(2, dtype=F32), 0.2 * np.eye(2, dtype=F32)
    else:
        n, f, fo = 1, nl.growth(), om.Growth()
        m0, Q, R = np.array([0.1], F32), np.eye(1, dtype=F32), np.eye(1, dtype=F32)
        u = (8 * np.cos(1.2 * np.arange(T))).astype(F32)
    H = np.eye(n, dtype=F32)
    p = bfa.ParamsNLSSM(m0, np.eye(n, dtype=F32), f, np.zeros(n, F32), Q, nl.linear_emission(H), np.zeros(n, F32), R)
    xs = np.empty((B, T, n), F32)
    x = m0 + rng.normal(size=(B, n)).astype(F32)
    for t in range(T):
        ut = 0.0 if u is None else u[t]
        x = np.stack([f(x[b], rng.normal(size=n).astype(F32) * np.sqrt(np.diag(Q)), ut) for b in range(B)])
        xs[:, t] = x
    ys = (xs + rng.normal(size=xs.shape) * np.sqrt(np.diag(R))).astype(F32)
    return p, fo, ys, u, B, T, n


@pytest.mark.parametrize("kind", ["lorenz63", "sine", "growth"])
def test_extended_smoother(kind):
    import bayesianfiltering_amd as bfa
    p, fo, ys, u, B, T, n = _ext_case(kind)
    post = bfa.gaussian_sum_filter(p, ys, 1, inputs=u, initial_means=np.tile(p.initial_mean, (B, 1)).reshape(B, 1, n))
    sm = bfa.rts_smoother(p, post, inputs=u, cross_covariances=True)
    zq = np.zeros(n, F32)
    jac = lambda b, m: np.stack([fo.jac_x(m[t], zq, np.array([0.0 if u is None else u[t]], F32)) for t in range(T)])
    _check(sm, _oracle(post, None, jac), name="ext_" + kind)
    gen = bfa.rts_smoother(p, post, inputs=u, cross_covariances=True, options={"force_generic": 1})
    _check(gen, _oracle(post, None, jac), name="ext_generic_" + kind)
    es = bfa.extended_kalman_smoother(p, ys, inputs=u)
    assert np.array_equal(_np(es.smoothed_means), _np(sm.smoothed_means))


def test_linear_model_through_both_entry_points():
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=8)
    _, post = _filter(a, 64, 20, seed=8)
    p = cm.product_params(a)
    lin = bfa.rts_smoother(p, post, cross_covariances=True)
    ext = bfa.rts_smoother(p, post, cross_covariances=True, extended=True)
    for x, y in zip(lin[2:], ext[2:]):
        assert cm.rel_err(_np(y), _np(x)) <= 1e-6


# 8 -----------------------------------------------------------------------------------------------------------------
def test_errors_on_device():
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    p = cm.product_params(a)
    ys = cm.simulate_batch(a, 4, 8, seed=1)
    post = bfa.gaussian_sum_filter(p, ys, 2)
    with pytest.raises(ValueError, match="one component"):
        bfa.rts_smoother(p, post)
    nl = bfa.nonlinearities
    pe = bfa.ParamsNLSSM(np.zeros(3, F32), np.eye(3, dtype=F32), nl.lorenz63(), np.zeros(3, F32), np.eye(3, dtype=F32),
                         nl.linear_emission(np.eye(3, dtype=F32)), np.zeros(3, F32), np.eye(3, dtype=F32))
    post3 = bfa.gaussian_sum_filter(pe, np.zeros((2, 8, 3), F32), 1, fields=("means", "covariances"))
    with pytest.raises(ValueError, match="predicted"):
        bfa.rts_smoother(pe, post3)
    with pytest.raises(bfa.BayesFiltError) as e:   # staged path forced on a layout it cannot serve
        bfa.rts_smoother(p, bfa.kalman_filter(p, ys, layout="batch_inner"), options={"rts_load_mode": 2})
    assert e.value.code == -1
