"""Gaussian-sum posterior sampler on the MI355X.  With the components and the noise given, sample (b, s) is the
one-component sampler's on chain (b, z[b, s]) with that noise row, bit for bit, on every route and both kernels; the drawn
components are the float32 draw restated in NumPy; keys mean what the documentation says; chunks through the carry equal
one pass; an invalid draw stays in its sample."""
import numpy as np
import pytest

from tests import common as cm
from tests import gaussian_sum_backward_cases as gc
from tests.test_gaussian_sum_smoother_gpu import case, _np, _same, _slice, STREAMS, GENERIC

pytestmark = pytest.mark.gpu

F32 = np.float32
B, T = 11, 12


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _noise(c, S, seed=5):
    return _dev(np.random.default_rng(seed).normal(size=(c.B, S, c.T, c.n)).astype(F32))


def _components(c, S, seed=6):
    return np.random.default_rng(seed).integers(0, c.K, size=(c.B, S)).astype(np.int32)


def _one_component_samples(c, post, S, noise, layout="reference", options=None):
    """posterior_sample on every slice: (K, B, S, T, n)"""
    import bayesianfiltering_amd as bfa
    kw = dict(noise=noise, inputs=c.u, layout=layout, options=options, **(c.route() or {"extended": True}))
    return np.stack([_np(bfa.posterior_sample(c.p, _slice(post, k), S, **kw)) for k in range(c.K)])


def _pick(per_k, z):
    """sample (b, s) of component z[b, s]"""
    Bn, S = z.shape
    return np.stack([np.stack([per_k[z[b, s], b, s] for s in range(S)]) for b in range(Bn)])


# 1 ---- a sample is the one-component sampler's on its chain, bit for bit ------------------------------------------------------
CASES = [("lorenz63-quad", 3, 1), ("lorenz63-quad", 5, 5), ("linear4", 3, 9), ("linear4", 5, 1), ("lorenz63-source", 3, 5),
         ("lorenz63-unscented", 5, 9), ("lorenz63-unscented", 3, 1), ("growth", 3, 5)]


@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@pytest.mark.parametrize("kind,K,S", CASES)
def test_samples_bit_for_bit(kind, K, S, layout):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    post, noise, z = c.post(layout), _noise(c, S), _components(c, S)
    x, zz = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, components=z, inputs=c.u, layout=layout,
                                              return_components=True, **c.route())
    assert tuple(x.shape) == (B, S, T, c.n) and np.array_equal(_np(zz), z)
    want = _pick(_one_component_samples(c, post, S, noise, layout), z)
    assert np.isfinite(want).all() and np.array_equal(_np(x), want)


@pytest.mark.parametrize("kind,K,S", [("lorenz63-quad", 3, 5), ("linear4", 5, 9), ("lorenz63-source", 3, 5), ("lorenz63-unscented", 3, 9),
                                      ("growth", 3, 1)])
def test_samples_bit_for_bit_force_generic(kind, K, S):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    for layout in ("reference", "batch_inner"):
        post, noise, z = c.post(layout), _noise(c, S), _components(c, S)
        z[3] = 1           # every sample of a trajectory on one component: the other workgroups serve none
        x = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, components=z, inputs=c.u, layout=layout, options=GENERIC,
                                              **c.route())
        want = _pick(_one_component_samples(c, post, S, noise, layout, options=GENERIC), z)
        assert np.array_equal(_np(x), want)


@pytest.mark.parametrize("S", [1, 9])
def test_samples_bit_for_bit_lds_kernel(S):
    import bayesianfiltering_amd as bfa
    c = case("lorenz96-10", 3, 5, 12)
    post, noise, z = c.post(), _noise(c, S), _components(c, S)
    x = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, components=z)
    assert np.array_equal(_np(x), _pick(_one_component_samples(c, post, S, noise), z))


def test_one_component_equals_posterior_sample():
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    c = case("lorenz63-quad", 1, 70, 13)
    noise = _noise(c, 5)
    x = bfa.gaussian_sum_posterior_sample(c.p, c.post(), 5, noise=noise, component_noise=np.full((70, 5), 0.5, F32))
    assert _same(x, bfa.posterior_sample(c.p, c.post(), 5, noise=noise, extended=True))
    key = bfa.PRNGKey(3)
    xk = bfa.gaussian_sum_posterior_sample(c.p, c.post(), 5, key=key)
    assert _same(xk, bfa.posterior_sample(c.p, c.post(), 5, key=bfr.split(key, 2)[0], extended=True))


# 2, 3 ---- the draw, and what a key means ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,S,options", [("lorenz63-quad", 5, 9, None), ("linear4", 3, 5, None), ("lorenz63-quad", 5, 9, GENERIC),
                                              ("lorenz96-10", 3, 9, None)])
def test_drawn_components_and_keys(kind, K, S, options):
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    c = case(kind, K, *((5, 12) if kind == "lorenz96-10" else (B, T)))
    post = c.post()
    w = _np(post.weights[..., -1])
    v = np.random.default_rng(8).random(size=(c.B, S)).astype(F32)
    v[0, 0], v[1, 0] = 0.0, np.nextafter(F32(1.0), F32(0.0))
    noise = _noise(c, S)
    x, z = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, component_noise=v, return_components=True, options=options)
    assert np.array_equal(_np(z), gc.draw_components_f32(w, v))
    assert _same(x, bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, components=z, options=options))
    # unnormalised weights given by the caller: the same draw as the restatement
    w2 = (w * np.linspace(0.5, 3.0, c.K, dtype=F32)).astype(F32)
    z2 = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, component_noise=v, weights=w2, return_components=True, options=options)[1]
    assert np.array_equal(_np(z2), gc.draw_components_f32(w2, v))
    # key = noise + component_noise formed on the host from the documented keys
    key = bfa.PRNGKey(11)
    k_x, k_z = bfr.split(key, 2)
    keys_x, keys_z = bfr.split(k_x, c.B), bfr.split(k_z, c.B)
    hn = np.stack([bfr.normal(keys_x[b], (S, c.T, c.n)) for b in range(c.B)])
    hv = np.stack([bfr.uniform(keys_z[b], (S,)) for b in range(c.B)])
    xk, zk = bfa.gaussian_sum_posterior_sample(c.p, post, S, key=key, return_components=True, options=options)
    xh, zh = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=_dev(hn), component_noise=hv, return_components=True, options=options)
    assert np.array_equal(_np(zk), _np(zh)) and np.array_equal(_np(zk), gc.draw_components_f32(w, hv))
    assert _same(xk, xh)


# 4 ---- chunks through the carry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,S,options", [("lorenz63-quad", 3, 5, None), ("lorenz63-unscented", 3, 1, None), ("linear4", 5, 9, GENERIC),
                                              ("lorenz63-source", 3, 5, None)])
def test_chunks_through_the_carry_bit_for_bit(kind, K, S, options):
    import bayesianfiltering_amd as bfa
    c = case(kind, K, B, T)
    post, noise = c.post(), _noise(c, S)
    v = np.random.default_rng(9).random(size=(B, S)).astype(F32)
    kw = dict(options=options, **c.route())
    full, z = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, component_noise=v, return_components=True, **kw)
    cut = lambda lo, hi: post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in STREAMS})
    w = post.weights[..., -1]
    s = T - 1   # the late chunk is one step long (T = 1)
    late, carry = bfa.gaussian_sum_posterior_sample(c.p, cut(s, T), S, noise=noise[:, :, s:].contiguous(), component_noise=v, weights=w,
                                                    return_carry=True, **kw)
    assert tuple(late.shape) == (B, S, 1, c.n) and np.array_equal(_np(carry.components), _np(z)) and _same(carry.states, late[:, :, 0])
    mid, carry2 = bfa.gaussian_sum_posterior_sample(c.p, cut(4, s), S, noise=noise[:, :, 4:s].contiguous(), carry=carry, return_carry=True, **kw)
    early = bfa.gaussian_sum_posterior_sample(c.p, cut(0, 4), S, noise=noise[:, :, :4].contiguous(), carry=carry2, **kw)
    assert np.array_equal(_np(carry2.components), _np(z))
    assert np.array_equal(np.concatenate([_np(early), _np(mid), _np(late)], axis=2), _np(full))


# 5 ---- invalid draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [None, GENERIC])
def test_invalid_draws_stay_in_their_sample(options):
    import bayesianfiltering_amd as bfa
    c = case("lorenz63-quad", 3, B, T)
    post, S = c.post(), 5
    noise = _noise(c, S)
    v = np.random.default_rng(10).random(size=(B, S)).astype(F32)
    good, zg = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, component_noise=v, return_components=True, options=options)
    w = post.weights[..., -1].clone()
    w[2] = float("nan")
    w[7] = 0.0
    x, z, carry = (lambda r: (r[0], r[2], r[1]))(bfa.gaussian_sum_posterior_sample(
        c.p, post, S, noise=noise, component_noise=v, weights=w, return_components=True, return_carry=True, options=options))
    dead = [2, 7]
    alive = [b for b in range(B) if b not in dead]
    assert (_np(z)[dead] == -1).all() and np.isnan(_np(x)[dead]).all() and np.isnan(_np(carry.states)[dead]).all()
    assert np.array_equal(_np(z)[alive], _np(zg)[alive]) and np.array_equal(_np(x)[alive], _np(good)[alive])
    # single samples marked invalid by the caller
    zi = _np(zg).copy()
    zi[0, 1] = zi[4, 4] = -1
    zi[5, 0] = 3      # outside [0, K): invalid too
    xi, zo = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=noise, components=zi, return_components=True, options=options)
    bad = np.zeros((B, S), bool)
    bad[0, 1] = bad[4, 4] = bad[5, 0] = True
    assert np.isnan(_np(xi)[bad]).all() and (_np(zo)[bad] == -1).all()
    assert np.array_equal(_np(xi)[~bad], _np(good)[~bad]) and np.array_equal(_np(zo)[~bad], _np(zg)[~bad])


# 6 ---- zero noise: the component's smoothed means --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,options", [("lorenz63-quad", None), ("lorenz63-unscented", None), ("linear4", GENERIC)])
def test_zero_noise_gives_the_smoothed_means_of_the_component(kind, options):
    import torch
    import bayesianfiltering_amd as bfa
    c = case(kind, 3, B, T)
    post, S = c.post(), 5
    pick = np.arange(B) % 3
    w = np.zeros((B, 3), F32)
    w[np.arange(B), pick] = 1.0       # one-hot weights
    v = np.random.default_rng(12).random(size=(B, S)).astype(F32)
    x, z = bfa.gaussian_sum_posterior_sample(c.p, post, S, noise=torch.zeros((B, S, T, c.n), device="cuda"), component_noise=v,
                                             weights=w, return_components=True, options=options, **c.route())
    assert np.array_equal(_np(z), np.repeat(pick[:, None], S, axis=1))
    sm = _np(bfa.gaussian_sum_smoother(c.p, post, collapsed=False, options=options, **c.route()).smoothed_means)
    want = np.stack([np.repeat(sm[b, pick[b]][None], S, axis=0) for b in range(B)])
    e = cm.rel_err(_np(x), want)
    cm.record(f"gs_sampler_zero_noise_{kind}", err=e)
    assert e <= 1e-6


# 7 ---- the components' frequencies --------------------------------------------------------------------------------------------
def test_component_frequencies():
    """4096 draws per trajectory from (0.2, 0.5, 0.3): each frequency within 4 standard errors, 4 sqrt(w (1 - w) / S) <= 0.031
    (the binomial's, not a measurement)"""
    import bayesianfiltering_amd as bfa
    c = case("lorenz63-quad", 3, 2, T)
    S = 4096
    w = np.tile(np.array([0.2, 0.5, 0.3], F32), (2, 1))
    x, z = bfa.gaussian_sum_posterior_sample(c.p, c.post(), S, key=bfa.PRNGKey(2024), weights=w, return_components=True)
    z = _np(z)
    assert np.isfinite(_np(x)).all() and z.min() >= 0 and z.max() <= 2
    for b in range(2):
        f = np.bincount(z[b], minlength=3) / S
        assert np.all(np.abs(f - w[b]) <= 4 * np.sqrt(w[b] * (1 - w[b]) / S)), (b, f)
    assert not np.array_equal(z[0], z[1])   # a key per trajectory
