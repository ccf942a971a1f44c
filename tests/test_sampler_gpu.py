"""Posterior sampler on the MI355X: parity with the float64 oracle of tests/test_sampler_cpu.py (itself pinned to the
dense joint Gaussian) on the GPU filter's own fp32 streams, every register instance, the run-time-dimension kernel, the
rank-deficient headline model, the exact joint law, keys, chunks, layouts, extended dynamics and the edges."""
import numpy as np
import pytest

from tests import common as cm
from tests.test_smoother_cpu import dense_posterior
from tests.test_sampler_cpu import ffbs_f64, joint_blocks, TAU

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 1e-5
SPLS = (1, 2, 4, 8)   # the samples-per-lane counts csrc/ffbs_sampler.hip compiles for every n <= 8
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")


def _np(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=F32), device="cuda")


def _filter(a, B, T, seed, layout="reference", fields=None):
    import bayesianfiltering_amd as bfa
    ys = cm.simulate_batch(a, B, T, seed=seed)
    post = bfa.kalman_filter(cm.product_params(a), ys, initial_means=np.tile(a["m0"], (B, 1)), layout=layout,
                             **({"fields": fields} if fields else {}))
    return ys, post


def _oracle(post, F, xi, inputs_F=None, pivots=None):
    """float64 backward sampling over the GPU's own fp32 filtered streams, trajectory by trajectory (posterior arrays
    (B, 1, T, ...), xi (B, S, T, n))."""
    m, P, pm, pP = (_np(getattr(post, k))[:, 0] for k in STREAMS)
    return np.stack([ffbs_f64(m[b], P[b], pm[b], pP[b], F if inputs_F is None else inputs_F(b, m[b]), xi[b], pivots=pivots)
                     for b in range(m.shape[0])])


def _err(x, ref, post):
    """e = max|x_gpu - x_f64| / max(1, max|x_f64|, sqrt(max diag P))"""
    P = _np(post.covariances)
    scale = max(1.0, float(np.max(np.abs(ref))), float(np.sqrt(np.max(np.diagonal(P, axis1=-2, axis2=-1)))))
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref)) / scale)


def _check(x, ref, post, name):
    e = _err(_np(x), ref, post)
    cm.record("sampler_" + name, err=e)
    print(f"sampler_{name}: e = {e:.3e}")
    assert e <= TOL, (name, e)


def _noise(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(F32)


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
def test_parity_every_register_instance(n):
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(n, max(1, n // 2), seed=n)
    B, S, T = 70, 5, 9
    _, post = _filter(a, B, T, seed=n)
    xi = _noise((B, S, T, n), 100 + n)
    ref = _oracle(post, a["A"], xi)
    p = cm.product_params(a)
    for spl in SPLS:
        x = bfa.posterior_sample(p, post, S, noise=_dev(xi), options={"ffbs_spl": spl})
        assert tuple(x.shape) == (B, S, T, n)
        _check(x, ref, post, f"reg_n{n}_spl{spl}")
    _check(bfa.posterior_sample(p, post, S, noise=_dev(xi)), ref, post, f"reg_n{n}_auto")


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", [(12, 5), (24, 5), (24, 100)])   # S = 100 at n = 24: two sample blocks in LDS (85 + 15)
def test_parity_runtime_dimension(n, S):
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(n, max(1, n // 2), seed=n)
    B, T = 3, 9
    _, post = _filter(a, B, T, seed=n)
    xi = _noise((B, S, T, n), 200 + n)
    ref = _oracle(post, a["A"], xi)
    x = bfa.posterior_sample(cm.product_params(a), post, S, noise=_dev(xi))
    _check(x, ref, post, f"generic_n{n}_S{S}")
    late, carry = bfa.posterior_sample(cm.product_params(a), _cut(post, 4, T), S, noise=_dev(xi[:, :, 4:]), return_carry=True)
    early = bfa.posterior_sample(cm.product_params(a), _cut(post, 0, 4), S, noise=_dev(xi[:, :, :4]), carry=carry)
    assert np.array_equal(np.concatenate([_np(early), _np(late)], axis=2), _np(x))


def test_force_generic_agrees_with_register_kernel():
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=4)
    B, S, T = 70, 5, 9
    _, post = _filter(a, B, T, seed=4)
    xi = _noise((B, S, T, 4), 204)
    ref = _oracle(post, a["A"], xi)
    p = cm.product_params(a)
    gen = bfa.posterior_sample(p, post, S, noise=_dev(xi), options={"force_generic": 1})
    reg = bfa.posterior_sample(p, post, S, noise=_dev(xi))
    _check(gen, ref, post, "generic_n4")
    _check(reg, ref, post, "reg_n4_vs_generic")
    _check(gen, _np(reg).astype(np.float64), post, "generic_n4_vs_reg")      # the two kernels against each other


@pytest.mark.parametrize("n,m", [(64, 32), (89, 2)])
def test_parity_near_the_lds_limit(n, m):
    """More than 64 KiB of dynamic LDS per workgroup (84 KiB at n = 64) and the largest n that fits 160 KiB (89).  P0 = I
    and Q = 0.1 I keep P- well conditioned (random_stable_lgssm's own P0 and Q have condition numbers of several hundred
    at these n, where ANY fp32 evaluation is 1e-5 ... 5e-5 from float64): a NumPy fp32 restatement of the recursion is
    7e-7 ... 1.4e-6 (n = 64) and 3.0e-6 ... 3.5e-6 (n = 89) from the oracle on this model, so the 1e-5 bound applies."""
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(n, m, seed=n)
    a["P0"], a["Q"] = np.eye(n, dtype=F32), (0.1 * np.eye(n)).astype(F32)
    B, S, T = 1, 2, 3
    _, post = _filter(a, B, T, seed=n)
    xi = _noise((B, S, T, n), 300 + n)
    x = bfa.posterior_sample(cm.product_params(a), post, S, noise=_dev(xi))
    _check(x, _oracle(post, a["A"], xi), post, f"generic_n{n}_lds_limit")


# 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [0, 1])
def test_rank_deficient_headline_model(generic):
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    B, S, T = 66, 3, 64
    _, post = _filter(a, B, T, seed=3)
    xi = _noise((B, S, T, 4), 303)
    piv = []
    ref = _oracle(post, a["A"], xi, pivots=piv)
    # the stated condition, on the oracle's pivots: no pivot straddles the threshold
    assert len(piv) == B * T
    ratios = np.array([r for rec in piv for r, _ in rec])
    kept = np.array([k for rec in piv for _, k in rec])
    assert np.all(ratios[kept] >= 100 * TAU), float(ratios[kept].min())
    assert np.all(np.abs(ratios[~kept]) <= TAU / 4), float(np.abs(ratios[~kept]).max())
    assert (~kept).sum() == 2 * B * (T - 1)
    cm.record("sampler_cv_pivots", smallest_kept=float(ratios[kept].min()), largest_dropped=float(np.abs(ratios[~kept]).max()))
    x = bfa.posterior_sample(cm.product_params(a), post, S, noise=_dev(xi), options={"force_generic": generic})
    assert np.all(np.isfinite(_np(x)))
    _check(x, ref, post, "cv_generic" if generic else "cv")


# 4 -----------------------------------------------------------------------------------------------------------------
def test_exact_joint_law_from_the_gpu():
    import bayesianfiltering_amd as bfa
    n, T, B = 3, 6, 2
    a = cm.random_stable_lgssm(n, 2, seed=21, bias=True)
    ys, post = _filter(a, B, T, seed=5)
    S = T * n + 1
    xi = np.zeros((B, S, T, n), F32)
    xi[:, 1:] = np.eye(T * n, dtype=F32).reshape(T * n, T, n)
    x = _np(bfa.posterior_sample(cm.product_params(a), post, S, noise=_dev(xi))).astype(np.float64).reshape(B, S, T * n)
    for b in range(B):
        dm, dP, dC = dense_posterior(a, ys[b].astype(np.float64), a["m0"], a["P0"])
        cov, cross = joint_blocks((x[b, 1:] - x[b, 0]).T, T, n)
        e = (cm.rel_err(x[b, 0].reshape(T, n), dm), cm.rel_err(cov, dP), cm.rel_err(cross, dC))
        cm.record("sampler_joint_law", errs=list(e))
        # the filter's gain carries the reference's +1e-6 on every entry of S (gaussfiltax/utils.py:258)
        assert max(e) < 1e-4, (b, e)


# 5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tv", [False, True])
def test_zero_noise_is_the_smoothed_mean(tv):
    import torch
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=33, dq=3, bias=True)
    B, T, S = 96, 32, 2
    if tv:
        rng = np.random.default_rng(1)
        a["Q"] = np.stack([a["Q"] * F32(0.5 + rng.random()) for _ in range(T)]).astype(F32)
    ys = cm.simulate_batch(dict(a, Q=a["Q"][0] if tv else a["Q"]), B, T, seed=2)
    p = cm.product_params(a)
    post = bfa.kalman_filter(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
    bare = post._replace(predicted_means=None, predicted_covariances=None)
    z = torch.zeros((B, S, T, 4), device="cuda")
    full, rec = bfa.posterior_sample(p, post, S, noise=z), bfa.posterior_sample(p, bare, S, noise=z)
    sm_full, sm_rec = bfa.rts_smoother(p, post).smoothed_means, bfa.rts_smoother(p, bare).smoothed_means
    for s in range(S):
        assert cm.rel_err(_np(full[:, s]), _np(sm_full[:, 0])) <= 1e-6
        assert cm.rel_err(_np(rec[:, s]), _np(sm_rec[:, 0])) <= 1e-6
    assert cm.rel_err(_np(rec), _np(full)) <= 1e-5
    gen = bfa.posterior_sample(p, bare, S, noise=z, options={"force_generic": 1})
    assert cm.rel_err(_np(gen), _np(full)) <= 1e-5
    if not tv:
        ks = bfa.kalman_posterior_sample(p, ys, S, bfa.PRNGKey(3), initial_means=np.tile(a["m0"], (B, 1)))
        assert np.array_equal(_np(ks), _np(bfa.posterior_sample(p, bare, S, key=bfa.PRNGKey(3))))


# 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [0, 1])
def test_key_mode(generic):
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    n, B, S, T = 3, 3, 3, 5     # 45 values per trajectory: odd, the padded Threefry block
    a = cm.random_stable_lgssm(n, 2, seed=6)
    _, post = _filter(a, B, T, seed=6)
    p = cm.product_params(a)
    opt = {"force_generic": generic}
    key = bfa.PRNGKey(7)
    keys = bfr.split(key, B)
    xi = np.stack([bfr.normal(keys[b], (S, T, n)) for b in range(B)])
    by_key = _np(bfa.posterior_sample(p, post, S, key=key, options=opt))
    by_noise = _np(bfa.posterior_sample(p, post, S, noise=_dev(xi), options=opt))
    assert np.array_equal(by_key, by_noise)
    assert np.array_equal(by_key, _np(bfa.posterior_sample(p, post, S, key=key, options=opt)))
    assert np.array_equal(by_key, _np(bfa.posterior_sample(p, post, S, key=keys, options=opt)))   # (B, 2) keys as they are
    other = _np(bfa.posterior_sample(p, post, S, key=bfa.PRNGKey(8), options=opt))
    assert not np.array_equal(by_key, other) and np.all(np.isfinite(other))
    _check(by_key, _oracle(post, a["A"], xi), post, "keys_generic" if generic else "keys")


# 7 -----------------------------------------------------------------------------------------------------------------
def _cut(post, lo, hi):
    return post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in STREAMS if getattr(post, k) is not None})


@pytest.mark.parametrize("generic", [0, 1])
def test_chunks_bit_for_bit(generic):
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    B, S, T, s = 70, 3, 20, 12
    _, post = _filter(a, B, T, seed=7)
    p = cm.product_params(a)
    opt = {"force_generic": generic}
    xi = _noise((B, S, T, 4), 707)
    full = _np(bfa.posterior_sample(p, post, S, noise=_dev(xi), options=opt))
    late, carry = bfa.posterior_sample(p, _cut(post, s, T), S, noise=_dev(xi[:, :, s:]), return_carry=True, options=opt)
    early = bfa.posterior_sample(p, _cut(post, 0, s), S, noise=_dev(xi[:, :, :s]), carry=carry, options=opt)
    assert np.array_equal(np.concatenate([_np(early), _np(late)], axis=2), full)
    assert tuple(carry.states.shape) == (B, S, 4)
    assert np.array_equal(_np(carry.states), _np(late[:, :, 0]))


# 8 -----------------------------------------------------------------------------------------------------------------
def test_layouts_bit_for_bit():
    import torch
    import bayesianfiltering_amd as bfa
    a = cm.cv_model_arrays()
    B, n, T, S = 130, 4, 12, 2
    _, post = _filter(a, B, T, seed=9)
    p = cm.product_params(a)
    xi = _noise((B, S, T, n), 808)
    ref = _np(bfa.posterior_sample(p, post, S, noise=_dev(xi)))
    # batch-inner inputs, noise and output
    _, post_bi = _filter(a, B, T, seed=9, layout="batch_inner")
    xi_bi = _dev(np.transpose(xi, (1, 2, 3, 0))).permute(3, 0, 1, 2)
    assert xi_bi.stride(0) == 1
    x_bi = bfa.posterior_sample(p, post_bi, S, noise=xi_bi, layout="batch_inner")
    assert x_bi.stride(0) == 1 and np.array_equal(_np(x_bi), ref)
    # a stride set neither layout has: every stream, the noise and the output a slice of a longer buffer
    wide = {k: torch.zeros((B, 1, T + 3) + tuple(getattr(post, k).shape[3:]), device="cuda")[:, :, 1:T + 1] for k in STREAMS}
    for k, v in wide.items():
        v.copy_(getattr(post, k))
    xi_w = torch.zeros((B, S, T + 3, n + 1), device="cuda")[:, :, 2:T + 2, :n]
    xi_w.copy_(_dev(xi))
    out_w = torch.full((B, S, T + 5, n + 2), -7.0, device="cuda")
    x_w = bfa.posterior_sample(p, post._replace(**wide), S, noise=xi_w, out=out_w[:, :, 3:T + 3, 1:n + 1])
    assert np.array_equal(_np(x_w), ref)
    rest = _np(out_w).copy()
    rest[:, :, 3:T + 3, 1:n + 1] = -7.0
    assert np.all(rest == -7.0)          # nothing written outside the slice


# 9 -----------------------------------------------------------------------------------------------------------------
def _ext_case(kind, with_inputs):
    import bayesianfiltering_amd as bfa
    from oracle import models as om
    nl = bfa.nonlinearities
    rng = np.random.default_rng(17)
    B, T, n = 5, 16, 3
    if kind == "lorenz63":
        f, fo = nl.lorenz63(), om.Lorenz63()
        m0, Q, R = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32), 0.5 * np.eye(3, dtype=F32)
    else:
        f, fo = nl.sine(3, w0=1.0), om.Sine(3, w0=1.0)
        m0, Q, R = np.array([0.3, -0.2, 0.5], F32), 1e-1 * np.eye(3, dtype=F32), 0.2 * np.eye(3, dtype=F32)
    u = (0.5 * np.cos(1.2 * np.arange(T))).astype(F32) if with_inputs else None
    p = bfa.ParamsNLSSM(m0, np.eye(n, dtype=F32), f, np.zeros(n, F32), Q, nl.linear_emission(np.eye(n, dtype=F32)),
                        np.zeros(n, F32), R)
    xs = np.empty((B, T, n), F32)
    x = m0 + rng.normal(size=(B, n)).astype(F32)
    for t in range(T):
        ut = 0.0 if u is None else u[t]
        x = np.stack([f(x[b], rng.normal(size=n).astype(F32) * np.sqrt(np.diag(Q)), ut) for b in range(B)])
        xs[:, t] = x
    ys = (xs + rng.normal(size=xs.shape) * np.sqrt(np.diag(R))).astype(F32)
    return p, fo, ys, u, B, T, n


@pytest.mark.parametrize("with_inputs", [False, True])
@pytest.mark.parametrize("kind", ["lorenz63", "sine"])
def test_extended_sampler(kind, with_inputs):
    import bayesianfiltering_amd as bfa
    p, fo, ys, u, B, T, n = _ext_case(kind, with_inputs)
    S = 3
    post = bfa.gaussian_sum_filter(p, ys, 1, inputs=u, initial_means=np.tile(p.initial_mean, (B, 1)).reshape(B, 1, n))
    xi = _noise((B, S, T, n), 909)
    zq = np.zeros(n, F32)
    jac = lambda b, m: np.stack([fo.jac_x(m[t], zq, np.array([0.0 if u is None else u[t]], F32)) for t in range(T)])
    ref = _oracle(post, None, xi, inputs_F=jac)
    tag = f"ext_{kind}" + ("_u" if with_inputs else "")
    _check(bfa.posterior_sample(p, post, S, noise=_dev(xi), inputs=u), ref, post, tag)
    _check(bfa.posterior_sample(p, post, S, noise=_dev(xi), inputs=u, options={"force_generic": 1}), ref, post, tag + "_generic")
    key = bfa.PRNGKey(5)
    es = bfa.extended_kalman_posterior_sample(p, ys, S, key, inputs=u)
    assert np.array_equal(_np(es), _np(bfa.posterior_sample(p, post, S, key=key, inputs=u)))


def test_linear_model_through_both_entry_points():
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(4, 2, seed=8)
    _, post = _filter(a, 64, 20, seed=8)
    p = cm.product_params(a)
    xi = _dev(_noise((64, 2, 20, 4), 11))
    lin = bfa.posterior_sample(p, post, 2, noise=xi)
    ext = bfa.posterior_sample(p, post, 2, noise=xi, extended=True)
    assert cm.rel_err(_np(ext), _np(lin)) <= 1e-6


# 10 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [0, 1])
def test_edges(generic):
    import bayesianfiltering_amd as bfa
    a = cm.random_stable_lgssm(3, 2, seed=10)
    p = cm.product_params(a)
    opt = {"force_generic": generic}
    # T = 1: only the first line of the contract
    _, post = _filter(a, 70, 1, seed=1)
    xi = _noise((70, 4, 1, 3), 1)
    x = bfa.posterior_sample(p, post, 4, noise=_dev(xi), options=opt)
    _check(x, _oracle(post, a["A"], xi), post, f"T1_g{generic}")
    L = np.linalg.cholesky(_np(post.covariances)[:, 0, 0].astype(np.float64))
    direct = _np(post.means)[:, 0, 0][:, None] + np.einsum("bij,bsj->bsi", L, xi[:, :, 0].astype(np.float64))
    assert np.max(np.abs(_np(x)[:, :, 0] - direct)) <= TOL * max(1.0, np.max(np.abs(direct)))
    # S = 1
    _, post = _filter(a, 70, 9, seed=2)
    xi = _noise((70, 1, 9, 3), 2)
    _check(bfa.posterior_sample(p, post, 1, noise=_dev(xi), options=opt), _oracle(post, a["A"], xi), post, f"S1_g{generic}")
    # B = 1: one trajectory in, (S, T, n) out
    ys = cm.simulate_batch(a, 1, 9, seed=3)[0]
    post1 = bfa.kalman_filter(p, ys, initial_means=a["m0"].reshape(1, -1))
    assert post1.means.dim() == 3
    xi = _noise((5, 9, 3), 3)
    x1 = bfa.posterior_sample(p, post1, 5, noise=_dev(xi), options=opt)
    assert tuple(x1.shape) == (5, 9, 3)
    lift = post1._replace(**{k: getattr(post1, k).unsqueeze(0) for k in STREAMS})
    _check(x1.unsqueeze(0), _oracle(lift, a["A"], xi[None]), lift, f"B1_g{generic}")
    x1k, c1 = bfa.posterior_sample(p, post1, 5, key=bfa.PRNGKey(1), return_carry=True, options=opt)
    assert tuple(x1k.shape) == (5, 9, 3) and tuple(c1.states.shape) == (1, 5, 3)
    assert np.array_equal(_np(c1.states[0]), _np(x1k[:, 0]))


def test_errors_on_device():
    """n beyond the LDS capacity of the run-time-dimension kernel is refused with the limit, before any launch."""
    import torch
    import bayesianfiltering_amd as bfa
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    n = 96
    big = cm.product_params(cm.random_stable_lgssm(n, 2, seed=2))
    fake = bfa.PosteriorGaussianSumFiltered(None, z(2, 1, 3, n), z(2, 1, 3, n, n), z(2, 1, 3, n), z(2, 1, 3, n, n))
    with pytest.raises(bfa.BayesFiltError) as e:
        bfa.posterior_sample(big, fake, 2, key=bfa.PRNGKey(0))
    assert e.value.code == -2 and "n <= 89" in str(e.value)
