"""parallel_posterior_sample on the GPU: parity with the float64 backward-sampling recursion on the same fp32 filter streams and
noise, the bits it shares with posterior_sample and the bits that must not depend on the launch shape, chunking through the
carry, the smoothed mean at zero noise, the exact joint law end to end, NaN containment, keys, default blocks.

Measured on an MI355X, worst over the parity shapes below against ffbs_f64 on the same streams and noise, error measure _err of
tests/test_sampler_gpu.py (bound 1e-5), predictions given / recomputed: (1,1) 6.2e-7 / 4.6e-7, (2,2) 3.0e-7 / 1.8e-7, (3,1)
4.1e-7 / 3.1e-7, (4,2) 4.5e-7 / 5.8e-7, (4,4) 6.7e-7 / 2.9e-7, biases 2.0e-7 / 2.3e-7, (5,2) 1.3e-6 / 1.6e-6, (6,3) 4.1e-7 /
5.3e-7; constant-velocity model against posterior_sample 2.8e-7 / 2.8e-7; chunks 1.6e-7; zero noise against the smoothed means
1.5e-7; exact joint law 1.2e-6 / 4.2e-6 / 6.6e-6 (bound 1e-4)."""
import functools

import numpy as np
import pytest
import torch

import bayesianfiltering_amd as bfa
from bayesianfiltering_amd import random as bfr
from tests import common as cm
from tests import parallel_sampler_cases as psc
from tests.test_sampler_gpu import _err

pytestmark = pytest.mark.gpu

TOL = 1e-5   # the project's standing fp32 tolerance
# (T, block): 300 spans -- across a wave, across a 256-thread tile into a second one, ragged last block of 3; 16 blocks inside
# one wave, ragged; one interior block; no interior block and one span; one block; one step
SHAPES = [(1203, 4), (1000, 64), (12, 4), (8, 4), (37, 64), (1, 64)]
B, S, TMAX = 3, 5, 1203   # S = 5: the sample blocks are ragged at every samples-per-lane count (1, 2, 4)
SPLS = (1, 2, 4)
PRED = ("predicted_means", "predicted_covariances")
ROUTES = pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])


def host(t):
    return t.cpu().numpy()


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def streams(name, Bn=B):
    """(params, the FULL5 posterior of kalman_filter over TMAX steps -- 'cv': of the float64 filter); shared, never modified."""
    a, ys, init, _ = psc.case(name, Bn, TMAX)
    p = cm.product_params(a)
    if name != "cv":
        return p, bfa.kalman_filter(p, ys, initial_means=init)
    # The constant-velocity model has unit eigenvalues: over 1203 steps the fp32 filter's covariances drift (DESIGN.md, section
    # 6h) until a predicted covariance is no longer positive definite in float64.  Its streams are the jitter-free float64
    # filter's, rounded to fp32: valid inputs for every backward pass.
    kf = [psc.kalman_f64(a, ys[b].astype(np.float64), init[b], a["P0"]) for b in range(Bn)]
    dev = lambda k: torch.as_tensor(np.stack([f[k] for f in kf])[:, None].astype(np.float32), device="cuda")
    return p, bfa.PosteriorGaussianSumFiltered(torch.ones((Bn, 1, TMAX), device="cuda"), dev("m"), dev("P"), dev("pm"), dev("pP"))


@functools.lru_cache(maxsize=None)
def noise(n, Bn=B, Sn=S):
    """Standard normals (Bn, Sn, TMAX, n) on the device; shared, never modified.  A call over [lo, hi) takes the view."""
    xi = np.random.default_rng(1000 + n).normal(size=(Bn, Sn, TMAX, n)).astype(np.float32)
    return torch.as_tensor(xi, device="cuda")


def cut(post, lo, hi, pred=True):
    """The steps [lo, hi) of a posterior as views, with or without the predicted streams."""
    part = post._replace(**{k: getattr(post, k)[:, :, lo:hi] for k in ("weights", "means", "covariances") + PRED})
    return part if pred else part._replace(predicted_means=None, predicted_covariances=None)


@functools.lru_cache(maxsize=None)
def yardstick(name, T, pred):
    """ffbs_f64 on the fp32 streams of steps [0, T) and noise(n)[:, :, :T], per trajectory.  The recomputed route's predictions
    are its definition in float64, m- = A m + G q0 and P- = A P A^T + G Q G^T, from the same fp32 m and P."""
    a = psc.model(name)
    post = cut(streams(name)[1], 0, T)
    m, P, pm, pP = (host(getattr(post, k))[:, 0].astype(np.float64) for k in ("means", "covariances") + PRED)
    if not pred:
        A, Qb, u = psc.terms(a)
        pm, pP = m @ A.T + u, A @ P @ A.T + Qb
    xi = host(noise(m.shape[-1]))[:, :, :T]
    return np.stack([psc.ffbs_f64(m[b], P[b], pm[b], pP[b], a["A"], xi[b]) for b in range(B)])


def draw(name, T, block, pred, Bn=B, lo=0, **kw):
    """parallel_posterior_sample over the steps [lo, lo + T) of the shared streams with the shared noise."""
    p, post = streams(name, Bn)
    n = post.means.shape[-1]
    return bfa.parallel_posterior_sample(p, cut(post, lo, lo + T, pred), S, noise=noise(n, Bn)[:, :, lo:lo + T], block=block, **kw)


def serial(name, T, pred, Bn=B, lo=0, **kw):
    p, post = streams(name, Bn)
    n = post.means.shape[-1]
    return bfa.posterior_sample(p, cut(post, lo, lo + T, pred), S, noise=noise(n, Bn)[:, :, lo:lo + T], **kw)


@ROUTES
@pytest.mark.parametrize("T,block", SHAPES)
@pytest.mark.parametrize("name", psc.MODELS)
def test_parity_with_the_float64_recursion(name, T, block, pred):
    x = draw(name, T, block, pred)
    assert tuple(x.shape) == (B, S, T, psc.model(name)["A"].shape[0])
    err = _err(host(x), yardstick(name, T, pred), cut(streams(name)[1], 0, T))
    print(f"parity {name} T={T} block={block} {'given' if pred else 'recomputed'}: e = {err:.2e}")
    assert err <= TOL, err


@ROUTES
@pytest.mark.parametrize("T,block", SHAPES)
def test_singular_noise_model(T, block, pred):
    """The constant-velocity model: unit eigenvalues, singular G Q G^T, Sigma_t of rank 2.  The yardstick is posterior_sample on
    the same streams and noise: the per-step factor bits (and so every dropped pivot) are shared with it, where the float64
    oracle's decisions at the 2^-17 threshold need not match fp32's (test_rank_deficient_headline_model treats them apart)."""
    x, ref = draw("cv", T, block, pred), serial("cv", T, pred)
    assert torch.isfinite(x).all()
    err = _err(host(x), host(ref).astype(np.float64), cut(streams("cv")[1], 0, T))
    print(f"parity cv T={T} block={block} {'given' if pred else 'recomputed'} against posterior_sample: e = {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("keyed", [False, True], ids=["noise", "key"])
@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@ROUTES
def test_one_block_is_the_serial_sampler_bit_for_bit(pred, layout, keyed):
    """T <= block: the emit launch alone is posterior_sample's recursion; also with a carry."""
    p, post = streams("4x2")
    later, early = cut(post, 37, 74, pred), cut(post, 0, 37, pred)
    rnd = lambda lo: dict(key=bfa.PRNGKey(7 + lo)) if keyed else dict(noise=noise(4)[:, :, lo:lo + 37])
    par, pc = bfa.parallel_posterior_sample(p, later, S, block=64, layout=layout, return_carry=True, **rnd(37))
    seq, sc = bfa.posterior_sample(p, later, S, layout=layout, return_carry=True, **rnd(37))
    assert same_bits(par, seq) and same_bits(pc.states, sc.states)
    assert same_bits(pc.states, par[:, :, 0])
    # the steps before, from that carry; T = block
    par2, pc2 = bfa.parallel_posterior_sample(p, early, S, carry=sc, block=37, layout=layout, return_carry=True, **rnd(0))
    seq2, sc2 = bfa.posterior_sample(p, early, S, carry=sc, layout=layout, return_carry=True, **rnd(0))
    assert same_bits(par2, seq2) and same_bits(pc2.states, sc2.states)


@pytest.mark.parametrize("T,lo", [(301, 300), (303, 300)], ids=["one-step-block", "ragged-block-of-3"])
@ROUTES
def test_last_block_is_the_serial_sampler_bit_for_bit(pred, T, lo):
    """block = 4: the steps from `lo` on are the last block, posterior_sample's recursion from the call's end; the earlier
    steps agree to tolerance."""
    par, seq = draw("4x2", T, 4, pred), serial("4x2", T, pred)
    assert same_bits(par[:, :, lo:], seq[:, :, lo:])
    err = _err(host(par), host(seq).astype(np.float64), cut(streams("4x2")[1], 0, T))
    print(f"last block T={T}: e = {err:.2e}")
    assert err <= TOL


@ROUTES
def test_bits_do_not_depend_on_the_launch(pred):
    T, block = 301, 4
    p, post5 = streams("4x2", 5)
    part, xi = cut(post5, 0, T, pred), noise(4, 5)[:, :, :T]
    call = lambda **kw: bfa.parallel_posterior_sample(p, part, S, noise=xi, block=block, **kw)
    full, carry = call(return_carry=True)
    # the same call twice
    again, carry2 = call(return_carry=True)
    assert same_bits(again, full) and same_bits(carry2.states, carry.states)
    # trajectory b alone
    for b in (0, 3):
        one_post = part._replace(**{k: getattr(part, k)[b:b + 1] for k in ("weights", "means", "covariances") + (PRED if pred else ())})
        one = bfa.parallel_posterior_sample(p, one_post, S, noise=xi[b:b + 1], block=block)
        assert same_bits(one[0], full[b]), b
    # sample s alone, with its noise row
    for s in (0, 3, 4):
        one = bfa.parallel_posterior_sample(p, part, 1, noise=xi[:, s:s + 1], block=block)
        assert same_bits(one[:, 0], full[:, s]), s
    # every samples-per-lane count
    for spl in SPLS:
        assert same_bits(call(options={"ffbs_spl": spl}), full), spl
    # layouts
    assert same_bits(call(layout="batch_inner"), full)
    # out= reuse and a reused workspace pre-filled with 0xFF, 64 bytes oversize, against a fresh one
    ws = torch.full((bfa.parallel_ffbs_workspace_bytes(4, 5, T, S, block) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    reused = call(out=again, workspace=ws)
    assert reused.data_ptr() == again.data_ptr()
    assert same_bits(reused, full)
    assert same_bits(call(workspace=ws), full)
    # the carry-out is step 0 of the samples
    assert same_bits(carry.states, full[:, :, 0])


def test_chunks_through_the_carry():
    """[600, 1203) then [0, 600) with its carry against one shot.  Not bit-equal: the one-shot sample after step 599 comes from
    the scan, the chunked one from the later chunk's emit launch."""
    whole = draw("4x2", TMAX, 4, True)
    second, carry = draw("4x2", TMAX - 600, 4, True, lo=600, return_carry=True)
    first = draw("4x2", 600, 4, True, carry=carry)
    assert same_bits(carry.states, second[:, :, 0])
    joined = np.concatenate([host(first), host(second)], axis=2)
    err = _err(joined, host(whole).astype(np.float64), streams("4x2")[1])
    print(f"chunks: e = {err:.2e}")
    assert err <= TOL


@ROUTES
def test_zero_noise_is_the_smoothed_mean(pred):
    T = 301
    p, post = streams("4x2")
    part = cut(post, 0, T, pred)
    x = bfa.parallel_posterior_sample(p, part, S, noise=torch.zeros((B, S, T, 4), device="cuda"), block=4)
    for label, sm in (("parallel_rts_smoother", bfa.parallel_rts_smoother(p, part, block=4)), ("rts_smoother", bfa.rts_smoother(p, part))):
        ref = host(sm.smoothed_means).astype(np.float64)   # (B, 1, T, n) against every sample
        err = _err(host(x), np.broadcast_to(ref, (B, S, T, 4)), part)
        print(f"zero noise against {label}: e = {err:.2e}")
        assert err <= TOL, label


def test_exact_joint_law_end_to_end():
    """The affine map noise -> samples of parallel_kalman_posterior_sample (filter, then sampler on the recompute route), rebuilt
    from the zero row and the unit rows, against the dense joint Gaussian: mean, marginal covariances, lag-one blocks."""
    T, n, Bn = 12, 2, 2
    a, ys, init, _ = psc.case("2x2", Bn, T)
    Sn = T * n + 1
    xi = np.zeros((Bn, Sn, T, n), np.float32)
    xi[:, 1:] = np.eye(T * n, dtype=np.float32).reshape(T * n, T, n)
    x = bfa.parallel_kalman_posterior_sample(cm.product_params(a), ys, Sn, None, noise=torch.as_tensor(xi, device="cuda"),
                                             initial_means=init, block=4)
    x = host(x).astype(np.float64).reshape(Bn, Sn, T * n)
    for b in range(Bn):
        dm, dP, dC = psc.dense_posterior(a, ys[b].astype(np.float64), init[b], a["P0"])
        cov, cross = psc.joint_blocks((x[b, 1:] - x[b, 0]).T, T, n)
        e = (cm.rel_err(x[b, 0].reshape(T, n), dm), cm.rel_err(cov, dP), cm.rel_err(cross, dC))
        print(f"joint law b={b}: {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
        # the filter's gain carries the reference's +1e-6 on every entry of S: the bound of test_exact_joint_law_from_the_gpu
        assert max(e) < 1e-4, (b, e)


@ROUTES
@pytest.mark.parametrize("field,index", [("means", (1, 0, 7, 0)), ("covariances", (1, 0, 7, 0, 0))])
def test_nan_input_stays_in_its_trajectory_and_flows_backwards(field, index, pred):
    """NaN at (b = 1, t = 7), T = 64, block = 4 (steps 4 ... 6 share the NaN's block).  The NaN pattern is posterior_sample's on
    the same inputs; the steps after 7 and the other trajectories keep the clean run's bits."""
    p, post = streams("4x2")
    T = 64
    clean_post = cut(post, 0, T, pred)
    bad = {k: (getattr(clean_post, k).clone() if getattr(clean_post, k) is not None else None) for k in ("means", "covariances") + PRED}
    bad[field][index] = float("nan")
    bad_post = clean_post._replace(**bad)
    xi = noise(4)[:, :, :T]
    clean = bfa.parallel_posterior_sample(p, clean_post, S, noise=xi, block=4)
    got = bfa.parallel_posterior_sample(p, bad_post, S, noise=xi, block=4)
    seq = bfa.posterior_sample(p, bad_post, S, noise=xi)
    v = host(got)
    assert np.array_equal(np.isnan(v), np.isnan(host(seq)))
    assert np.isfinite(v[1, :, 8:]).all()
    assert np.isnan(v[1, :, :8]).any(axis=-1).all()   # every sample of b = 1 at every step <= 7
    assert np.isnan(v[1, :, :7]).all()
    assert same_bits(got[1, :, 8:], clean[1, :, 8:])
    for b in (0, 2):
        assert same_bits(got[b], clean[b]), b


@ROUTES
def test_key_mode_is_noise_mode_on_the_keys_normals(pred):
    T = 301
    p, post = streams("4x2")
    part = cut(post, 0, T, pred)
    key = bfa.PRNGKey(11)
    keys = bfr.split(key, B)
    xi = torch.as_tensor(np.stack([bfr.normal(keys[b], (S, T, 4)) for b in range(B)]), device="cuda")
    by_key, ck = bfa.parallel_posterior_sample(p, part, S, key=key, block=4, return_carry=True)
    by_noise, cn = bfa.parallel_posterior_sample(p, part, S, noise=xi, block=4, return_carry=True)
    assert same_bits(by_key, by_noise) and same_bits(ck.states, cn.states)
    assert same_bits(by_key, bfa.parallel_posterior_sample(p, part, S, key=keys, block=4))


@pytest.mark.parametrize("Bd,Sd,Td", [(1, 1, 5000), (64, 4, 300), (4096, 2, 16)])
def test_default_block(Bd, Sd, Td):
    a = psc.model("4x2")
    ys = cm.simulate_batch(a, Bd, Td, seed=3)
    x = bfa.parallel_kalman_posterior_sample(cm.product_params(a), ys, Sd, bfa.PRNGKey(5))
    assert tuple(x.shape) == (Bd, Sd, Td, 4)
    assert torch.isfinite(x).all()
