"""Gaussian-sum smoother on the MI355X.  The per-component streams are the one-component smoother's, bit for bit, on every
route, layout and kernel; the fused collapsed moments are the float64 collapse of those streams; a linear model with a
mixture prior is smoothed exactly; chunks through the carry equal one pass; dead weights stay in their trajectory."""
import functools

import numpy as np
import pytest

from tests import common as cm
from tests import gaussian_sum_backward_cases as gc
from tests import source_smoother_cases as sc

pytestmark = pytest.mark.gpu

F32 = np.float32
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")
SMOOTHED = ("smoothed_means", "smoothed_covariances", "smoothed_cross_covariances")
GENERIC = {"force_generic": 1}
UP = (1.0, 0.0, 0.0)


def _np(x):
    return x.detach().cpu().numpy()


def _same(a, b):
    a, b = _np(a), _np(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Case:
    def __init__(self, p, ys, u, init, n, uparams=None):
        self.p, self.ys, self.u, self.init, self.n, self.uparams = p, ys, u, init, n, uparams
        self.B, self.T = ys.shape[:2]
        self.K = init.shape[1]

    @functools.lru_cache(maxsize=None)
    def post(self, layout="reference"):
        import bayesianfiltering_amd as bfa
        if self.uparams is not None:
            return bfa.unscented_gaussian_sum_filter(self.p, self.uparams, self.ys, self.K, inputs=self.u, initial_means=self.init,
                                                     layout=layout)
        return bfa.gaussian_sum_filter(self.p, self.ys, self.K, inputs=self.u, initial_means=self.init, layout=layout)

    def route(self):
        return {"uparams": self.uparams} if self.uparams is not None else {}


def _simulate(f, h, m0, Q, R, B, T, u, rng):
    """(B, T, m) observations of the model; u (T,), (B, T, 1) or None"""
    x = m0 + rng.normal(size=(B, m0.size)).astype(F32)
    sq, sr = np.sqrt(np.diag(Q)), np.sqrt(np.diag(R))
    ys = []
    for t in range(T):
        ut = lambda b: 0.0 if u is None else (u[t] if np.ndim(u) == 1 else u[b, t, 0])
        x = np.stack([f(x[b], rng.normal(size=sq.size).astype(F32) * sq, ut(b)) for b in range(B)])
        ys.append(np.stack([h(x[b], rng.normal(size=sr.size).astype(F32) * sr, ut(b)) for b in range(B)]))
    return np.stack(ys, axis=1).astype(F32)


@functools.lru_cache(maxsize=None)
def case(kind, K, B, T):
    """kind: 'lorenz63-quad', 'growth' (inputs that differ per trajectory), 'lorenz63-source', 'pendulum' (a recorded lambda),
    'lorenz63-unscented', 'lorenz96-8', 'lorenz96-10', 'linear4' (n = 4, linear registry functions)."""
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    rng = np.random.default_rng(1000 + 7 * K + B + T)
    u, up, spread = None, None, 0.5
    if kind == "linear4":
        a = cm.random_stable_lgssm(4, 2, seed=41, bias=True)
        p = cm.product_params(a)
        ys = cm.simulate_batch(a, B, T, seed=42)
        init = (a["m0"] + spread * rng.normal(size=(B, K, 4))).astype(F32)
        return Case(p, ys, None, init, 4)
    if kind == "pendulum":
        p = sc.pendulum_case().p
        f, h = p.dynamics_function, p.emission_function
        m0, Q, R, n, spread = np.asarray(p.initial_mean, F32), np.asarray(p.dynamics_noise_covariance), np.asarray(p.emission_noise_covariance), 2, 0.2
        ys = _simulate(lambda x, q, u_: f(x, q, u_), lambda x, r, u_: h(x, r, u_), m0, Q, R, B, T, None, rng)
        return Case(p, ys, None, (m0 + spread * rng.normal(size=(B, K, n))).astype(F32), n)
    if kind.startswith("lorenz63"):
        n, reg = 3, nl.lorenz63()
        f = nl.user_dynamics(sc.L63_SRC, 3, theta=sc.L63_THETA) if kind.endswith("source") else reg
        m0, Q = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32)
        if kind.endswith("quad"):
            h, R = nl.quadratic(3, 0.5), 0.5 * np.eye(1, dtype=F32)
        else:
            h, R = nl.linear_emission(np.eye(3, dtype=F32)), 0.5 * np.eye(3, dtype=F32)
        up = bfa.ParamsUKF(*UP) if kind.endswith("unscented") else None
    elif kind == "growth":
        n, reg = 1, nl.growth()
        f, h = reg, nl.linear_emission(np.eye(1, dtype=F32))
        m0, Q, R = np.array([0.1], F32), np.eye(1, dtype=F32), np.eye(1, dtype=F32)
        u = (8 * np.cos(1.2 * np.arange(T)[None, :, None] + 0.3 * np.arange(B)[:, None, None])).astype(F32)
    elif kind.startswith("lorenz96"):
        n = int(kind.split("-")[1])
        reg = nl.lorenz96(n)
        f, h = reg, nl.linear_emission(np.eye(n, dtype=F32))
        m0, Q, R = np.linspace(-1.0, 1.0, n).astype(F32), 1e-2 * np.eye(n, dtype=F32), 0.5 * np.eye(n, dtype=F32)
    else:
        raise ValueError(kind)
    p = bfa.ParamsNLSSM(m0, np.eye(n, dtype=F32), f, np.zeros(Q.shape[0], F32), Q, h, np.zeros(R.shape[0], F32), R)
    ys = _simulate(reg, h, m0, Q, R, B, T, u, rng)
    return Case(p, ys, u, (m0 + spread * rng.normal(size=(B, K, n))).astype(F32), n, up)


def _slice(post, k):
    return post._replace(**{s: getattr(post, s)[:, k:k + 1] for s in STREAMS + ("weights",)})


def _components_equal_one_component_smoother(c, layout, options=None):
    """every chain of the Gaussian-sum smoother against rts_smoother on its slice"""
    import bayesianfiltering_amd as bfa
    post = c.post(layout)
    gs = bfa.gaussian_sum_smoother(c.p, post, inputs=c.u, cross_covariances=True, collapsed=False, layout=layout,
                                   options=options, **c.route())
    assert gs.collapsed_means is None and tuple(gs.smoothed_means.shape) == (c.B, c.K, c.T, c.n)
    assert tuple(gs.smoothed_cross_covariances.shape) == (c.B, c.K, c.T - 1, c.n, c.n)
    assert np.isfinite(_np(gs.smoothed_covariances)).all()
    for k in range(c.K):
        one = bfa.rts_smoother(c.p, _slice(post, k), inputs=c.u, cross_covariances=True, layout=layout, options=options,
                               **(c.route() or {"extended": True}))
        for s in SMOOTHED:
            assert _same(getattr(gs, s)[:, k:k + 1], getattr(one, s)), (k, s)
    assert _same(gs.weights, post.weights[..., -1])
    return gs


# 1 ---- per-component streams, bit for bit ------------------------------------------------------------------------------------
SHAPES = [("linear4", 3, 37, 13), ("linear4", 5, 13, 24), ("linear4", 64, 3, 13), ("growth", 2, 70, 24), ("lorenz63-quad", 2, 70, 13),
          ("lorenz96-8", 2, 70, 13), ("lorenz63-source", 3, 37, 13), ("pendulum", 5, 13, 24), ("lorenz63-unscented", 3, 37, 13),
          ("lorenz63-unscented", 2, 70, 24)]


@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@pytest.mark.parametrize("kind,K,B,T", SHAPES)
def test_components_bit_for_bit(kind, K, B, T, layout):
    c = case(kind, K, B, T)
    gs = _components_equal_one_component_smoother(c, layout)
    if layout == "reference" and c.uparams is None:
        # the strided data path against the default one (staged where the rows are 16-byte aligned and B K >= 64)
        import bayesianfiltering_amd as bfa
        st = bfa.gaussian_sum_smoother(c.p, c.post(layout), inputs=c.u, cross_covariances=True, collapsed=False,
                                       options={"rts_load_mode": 0})
        for s in SMOOTHED:
            assert _same(getattr(st, s), getattr(gs, s)), s


@pytest.mark.parametrize("kind,K,B,T", [("linear4", 3, 37, 13), ("growth", 2, 70, 24), ("lorenz63-source", 3, 37, 13),
                                        ("lorenz63-unscented", 3, 37, 13)])
def test_components_bit_for_bit_force_generic(kind, K, B, T):
    _components_equal_one_component_smoother(case(kind, K, B, T), "reference", options=GENERIC)
    _components_equal_one_component_smoother(case(kind, K, B, T), "batch_inner", options=GENERIC)


@pytest.mark.parametrize("kind", ["lorenz96-10"])
def test_components_bit_for_bit_lds_kernel(kind):
    c = case(kind, 3, 5, 12)
    _components_equal_one_component_smoother(c, "reference")
    _components_equal_one_component_smoother(c, "batch_inner")


# 2 ---- collapsed moments -----------------------------------------------------------------------------------------------------
def _collapse_err(sm, name):
    """collapsed moments against the float64 collapse of the call's own fp32 per-component streams and weights"""
    w, ms, Ps = _np(sm.weights), _np(sm.smoothed_means), _np(sm.smoothed_covariances)
    ref = [gc.collapse_f64(w[b], ms[b], Ps[b]) for b in range(w.shape[0])]
    e = (cm.rel_err(_np(sm.collapsed_means), np.stack([r[0] for r in ref])),
         cm.rel_err(_np(sm.collapsed_covariances), np.stack([r[1] for r in ref])))
    cm.record("gs_smoother_collapse_" + name, errs=list(e))
    return max(e)


@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@pytest.mark.parametrize("kind,K,B,T", SHAPES)
def test_fused_collapsed_moments(kind, K, B, T, layout):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    post = c.post(layout)
    both = bfa.gaussian_sum_smoother(c.p, post, inputs=c.u, cross_covariances=True, layout=layout, **c.route())
    assert tuple(both.collapsed_means.shape) == (B, T, c.n) and tuple(both.collapsed_covariances.shape) == (B, T, c.n, c.n)
    assert _collapse_err(both, f"{kind}_K{K}_{layout}") <= 1e-5
    comp = bfa.gaussian_sum_smoother(c.p, post, inputs=c.u, cross_covariances=True, collapsed=False, layout=layout, **c.route())
    for s in SMOOTHED:  # the fused kernel's chains carry the bits of the components-only one
        assert _same(getattr(both, s), getattr(comp, s)), s
    only = bfa.gaussian_sum_smoother(c.p, post, inputs=c.u, components=False, layout=layout, **c.route())
    assert only.smoothed_means is None and only.smoothed_covariances is None
    assert _same(only.collapsed_means, both.collapsed_means) and _same(only.collapsed_covariances, both.collapsed_covariances)
    # five trajectories run alone: another place in the wave, the same bits
    lo = min(B - 5, 30) if B >= 5 else 0
    hi = min(lo + 5, B)
    sub = post._replace(**{s: getattr(post, s)[lo:hi].contiguous() for s in STREAMS + ("weights",)})
    u = c.u[lo:hi] if (c.u is not None and np.ndim(c.u) == 3) else c.u
    alone = bfa.gaussian_sum_smoother(c.p, sub, inputs=u, components=False, **c.route())
    assert _same(alone.collapsed_means, both.collapsed_means[lo:hi]) and _same(alone.collapsed_covariances, both.collapsed_covariances[lo:hi])


def test_collapsed_moments_after_the_lds_kernel():
    """n = 10 and force_generic: the moments come from the collapse kernel over the component streams"""
    import bayesianfiltering_amd as bfa
    c = case("lorenz96-10", 3, 5, 12)
    both = bfa.gaussian_sum_smoother(c.p, c.post(), **c.route())
    assert _collapse_err(both, "lorenz96-10") <= 1e-5
    only = bfa.gaussian_sum_smoother(c.p, c.post(), components=False)
    assert only.smoothed_means is None and _same(only.collapsed_means, both.collapsed_means)
    c = case("linear4", 3, 37, 13)
    gen = bfa.gaussian_sum_smoother(c.p, c.post(), options=GENERIC)
    assert _collapse_err(gen, "linear4_generic") <= 1e-5


# 3 ---- exactness on a linear model with a mixture prior -----------------------------------------------------------------------
@pytest.mark.parametrize("n,m,K,T,seed", [(4, 2, 3, 16, 300), (3, 2, 5, 24, 310)])
def test_linear_mixture_against_exact_dense_mixture(n, m, K, T, seed):
    import bayesianfiltering_amd as bfa
    a, ys, m_inits = gc.mixture_case(n, m, K, T, seed)
    p = cm.product_params(a)
    post = bfa.gaussian_sum_filter(p, ys.astype(F32)[None], K, initial_means=m_inits.astype(F32)[None])
    sm = bfa.gaussian_sum_smoother(p, post)
    w, dm, dP, dmu, dS = gc.dense_mixture(a, ys, m_inits.astype(F32).astype(np.float64), a["P0"])
    assert _same(sm.weights, post.weights[..., -1])
    # the filter's gain carries the reference's +1e-6 on every entry of S (gaussfiltax/utils.py:258): the bar of
    # test_kalman_smoother_vs_exact_posterior
    e = (cm.rel_err(_np(sm.weights[0]), w), cm.rel_err(_np(sm.smoothed_means[0]), dm), cm.rel_err(_np(sm.smoothed_covariances[0]), dP),
         cm.rel_err(_np(sm.collapsed_means[0]), dmu), cm.rel_err(_np(sm.collapsed_covariances[0]), dS))
    cm.record(f"gs_smoother_exact_n{n}_K{K}", errs=list(e))
    assert max(e) <= 1e-4, e
    assert np.ptp(w) > 1e-3
    # the wrappers: filter, then the same backward pass
    un = bfa.unscented_gaussian_sum_smoother(p, UP, ys.astype(F32)[None], K, initial_means=m_inits.astype(F32)[None])
    upost = bfa.unscented_gaussian_sum_filter(p, bfa.ParamsUKF(*UP), ys.astype(F32)[None], K, initial_means=m_inits.astype(F32)[None])
    un2 = bfa.gaussian_sum_smoother(p, upost, uparams=UP)
    assert _same(un.collapsed_means, un2.collapsed_means) and _same(un.smoothed_covariances, un2.smoothed_covariances)
    ex = bfa.extended_gaussian_sum_smoother(p, ys.astype(F32)[None], K, initial_means=m_inits.astype(F32)[None])
    assert _same(ex.collapsed_means, sm.collapsed_means) and _same(ex.smoothed_covariances, sm.smoothed_covariances)


# 4 ---- chunks, K = 1, unbatched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,B,T,options", [("linear4", 3, 37, 13, None), ("lorenz63-unscented", 3, 37, 13, None),
                                                 ("lorenz63-source", 3, 37, 13, None), ("growth", 2, 70, 24, GENERIC)])
def test_chunks_through_the_carry_bit_for_bit(kind, K, B, T, options):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    post, s = c.post(), 5
    kw = dict(cross_covariances=True, options=options, **c.route())
    full = bfa.gaussian_sum_smoother(c.p, post, inputs=c.u, **kw)
    cut = lambda lo, hi: post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in STREAMS + ("weights",)})
    ucut = lambda lo, hi: None if c.u is None else c.u[:, lo:hi]
    w = post.weights[..., -1]
    late, carry = bfa.gaussian_sum_smoother(c.p, cut(s, T), inputs=ucut(s, T), return_carry=True, **kw)
    early = bfa.gaussian_sum_smoother(c.p, cut(0, s), inputs=ucut(0, s), carry=carry, **kw)   # the weights travel in the carry
    assert _same(carry.weights, w) and _same(early.weights, w)
    assert tuple(carry.means.shape) == (B, K, c.n) and _same(carry.means, late.smoothed_means[:, :, 0])
    for k in SMOOTHED[:2] + ("collapsed_means", "collapsed_covariances"):
        ax = 1 if k.startswith("collapsed") else 2
        joined = np.concatenate([_np(getattr(early, k)), _np(getattr(late, k))], axis=ax)
        assert np.array_equal(joined, _np(getattr(full, k))), k
    C = np.concatenate([_np(early.smoothed_cross_covariances), _np(late.smoothed_cross_covariances)], axis=2)
    assert np.array_equal(C, _np(full.smoothed_cross_covariances))
    # collapsed moments alone through the carry
    l2, c2 = bfa.gaussian_sum_smoother(c.p, cut(s, T), inputs=ucut(s, T), return_carry=True, components=False, options=options, **c.route())
    e2 = bfa.gaussian_sum_smoother(c.p, cut(0, s), inputs=ucut(0, s), carry=c2, components=False, options=options, **c.route())
    assert _same(c2.means, carry.means) and _same(c2.covariances, carry.covariances)
    assert np.array_equal(np.concatenate([_np(e2.collapsed_means), _np(l2.collapsed_means)], axis=1), _np(full.collapsed_means))


@pytest.mark.parametrize("kind", ["lorenz63-quad", "lorenz63-unscented", "lorenz63-source", "lorenz96-10"])
@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
def test_one_component_equals_rts_smoother(kind, layout):
    import bayesianfiltering_amd as bfa
    c = case(kind, 1, 70 if kind != "lorenz96-10" else 5, 13)
    post = c.post(layout)
    one = bfa.rts_smoother(c.p, post, cross_covariances=True, layout=layout, **(c.route() or {"extended": True}))
    gs = bfa.gaussian_sum_smoother(c.p, post, cross_covariances=True, layout=layout, **c.route())
    for s in SMOOTHED:
        assert _same(getattr(gs, s), getattr(one, s)), s
    # one component of weight one: the collapsed moments are w (P + d d^T) with d = m - w m
    assert _collapse_err(gs, f"K1_{kind}_{layout}") <= 1e-6


def test_unbatched_posterior_squeezes():
    import bayesianfiltering_amd as bfa
    c = case("lorenz63-quad", 3, 1, 13)
    post = bfa.gaussian_sum_filter(c.p, c.ys[0], 3, initial_means=c.init[0])
    assert post.means.dim() == 3
    sm = bfa.gaussian_sum_smoother(c.p, post, cross_covariances=True)
    ref = bfa.gaussian_sum_smoother(c.p, c.post(), cross_covariances=True)
    assert tuple(sm.weights.shape) == (3,) and tuple(sm.smoothed_means.shape) == (3, 13, 3) and tuple(sm.collapsed_covariances.shape) == (13, 3, 3)
    for s in SMOOTHED + ("collapsed_means", "collapsed_covariances", "weights"):
        assert _same(getattr(sm, s), getattr(ref, s)[0]), s


# 5 ---- a trajectory whose weights died ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,B,T,options", [("linear4", 3, 37, 13, None), ("lorenz63-unscented", 3, 37, 13, None),
                                                 ("linear4", 3, 37, 13, GENERIC)])
def test_nan_weights_stay_in_their_trajectory(kind, K, B, T, options):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    post = c.post()
    good = bfa.gaussian_sum_smoother(c.p, post, options=options, **c.route())
    w = post.weights[..., -1].clone()
    dead = [1, 18, B - 1]
    w[dead] = float("nan")
    sm = bfa.gaussian_sum_smoother(c.p, post, weights=w, options=options, **c.route())
    alive = [b for b in range(B) if b not in dead]
    assert np.isnan(_np(sm.collapsed_means[dead])).all() and np.isnan(_np(sm.collapsed_covariances[dead])).all()
    assert _same(sm.collapsed_means[alive], good.collapsed_means[alive]) and _same(sm.collapsed_covariances[alive], good.collapsed_covariances[alive])
    assert _same(sm.smoothed_means, good.smoothed_means) and _same(sm.smoothed_covariances, good.smoothed_covariances)
    assert np.isfinite(_np(sm.smoothed_means)).all()


# 6 ---- more components than the fused kernel holds ---------------------------------------------------------------------------
def test_65_components():
    import ctypes as C
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import _lib
    c = case("linear4", 65, 2, 13)
    post = c.post()
    both = bfa.gaussian_sum_smoother(c.p, post)
    assert _collapse_err(both, "linear4_K65") <= 1e-5
    only = bfa.gaussian_sum_smoother(c.p, post, components=False)   # Python smooths into scratch streams and collapses them
    assert only.smoothed_means is None
    assert _same(only.collapsed_means, both.collapsed_means) and _same(only.collapsed_covariances, both.collapsed_covariances)
    # the C call itself refuses collapsed moments alone, naming the limit
    from bayesianfiltering_amd.inference import _Model, _stream_desc
    lib = _lib.load()
    fd = _lib.bf_out_desc()
    fd.means, fd.covs = _stream_desc(post.means, 1), _stream_desc(post.covariances, 2)
    fd.pred_means, fd.pred_covs = _stream_desc(post.predicted_means, 1), _stream_desc(post.predicted_covariances, 2)
    sd = _lib.bf_gs_smooth_desc()
    sd.coll_mean.ptr, sd.coll_mean.sB, sd.coll_mean.sT, sd.coll_mean.sE = only.collapsed_means.data_ptr(), 13 * 4, 4, 1
    sd.weights = both.weights.data_ptr()
    mdl = _Model(c.p)
    rc = lib.bf_gs_smoother_f32(C.byref(mdl.c), None, C.byref(_lib.bf_cstream()), C.byref(fd), 2, 13, 65, None, C.byref(sd), None)
    assert rc == _lib.BF_EUNSUPPORTED and b"K <= 64" in lib.bf_last_error() and b"K = 65" in lib.bf_last_error()


def test_single_trajectory_many_components():
    """K = 100 chains of one trajectory fill lanes (one launch), on both layouts"""
    import bayesianfiltering_amd as bfa
    c = case("lorenz63-quad", 100, 1, 13)
    for layout in ("reference", "batch_inner"):
        gs = bfa.gaussian_sum_smoother(c.p, c.post(layout), layout=layout)
        assert _collapse_err(gs, "K100_" + layout) <= 1e-5
        k = 57
        one = bfa.rts_smoother(c.p, _slice(c.post(layout), k), extended=True, layout=layout)
        assert _same(gs.smoothed_means[:, k:k + 1], one.smoothed_means) and _same(gs.smoothed_covariances[:, k:k + 1], one.smoothed_covariances)
