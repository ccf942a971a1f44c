"""parallel_rts_smoother on the GPU: parity with the float64 RTS recursion on the same fp32 filter streams, the bits it shares
with rts_smoother and the bits that must not depend on the launch shape, chunking through the carry, NaN containment, the
filter-then-smoother wrapper end to end, default blocks.

Measured on an MI355X, worst over the parity cases below against rts_f64 on the same streams (bound 1e-5): rel_err 2.9e-7
(smoothed means), 2.3e-6 (covariances), 3.0e-6 (cross-covariances); elem_err(ev=2) 3.9e-6 (covariances), 2.7e-6
(cross-covariances) -- the worst of them at one block, the serial recursion itself; constant-velocity model 3.4e-7 / 1.8e-6 / 1.8e-6
and 2.9e-6 / 2.5e-6."""
import functools

import numpy as np
import pytest
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm
from tests import parallel_smoother_cases as psc

pytestmark = pytest.mark.gpu

TOL = 1e-5   # the project's standing fp32 tolerance
# (T, block): 300 spans -- across a wave, across a 256-thread tile into a second one, ragged last block of 3; 16 blocks inside
# one wave, ragged; one interior block; no interior block and one span; one block; one step
SHAPES = [(1203, 4), (1000, 64), (12, 4), (8, 4), (37, 64), (1, 64)]
B, TMAX = 3, 1203
OUTPUTS = ("smoothed_means", "smoothed_covariances", "smoothed_cross_covariances")
PRED = ("predicted_means", "predicted_covariances")


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
    # 6h) until a predicted covariance is no longer positive definite in float64, and the yardstick's Cholesky refuses it.
    # Its streams are the jitter-free float64 filter's, rounded to fp32: valid inputs for every smoother.
    kf = [psc.kalman_f64(a, ys[b].astype(np.float64), init[b], a["P0"]) for b in range(Bn)]
    dev = lambda k: torch.as_tensor(np.stack([f[k] for f in kf])[:, None].astype(np.float32), device="cuda")
    return p, bfa.PosteriorGaussianSumFiltered(torch.ones((Bn, 1, TMAX), device="cuda"), dev("m"), dev("P"), dev("pm"), dev("pP"))


def cut(post, lo, hi, pred=True):
    """The steps [lo, hi) of a posterior as views, with or without the predicted streams."""
    part = post._replace(**{k: getattr(post, k)[:, :, lo:hi] for k in ("weights", "means", "covariances") + PRED})
    return part if pred else part._replace(predicted_means=None, predicted_covariances=None)


@functools.lru_cache(maxsize=None)
def yardstick(name, T):
    """rts_f64 on the fp32 streams of steps [0, T), per trajectory: (means, covariances, cross-covariances with T-1 steps)."""
    a = psc.model(name)
    post = cut(streams(name)[1], 0, T)
    m, P, pm, pP = (host(getattr(post, k)) for k in ("means", "covariances") + PRED)
    out = [psc.rts_f64(m[b, 0], P[b, 0], pm[b, 0], pP[b, 0], a["A"]) for b in range(B)]
    return tuple(np.stack([o[i] for o in out])[:, None, :T if i < 2 else T - 1] for i in range(3))


def check_parity(name, T, block, pred):
    p, post = streams(name)
    sm = bfa.parallel_rts_smoother(p, cut(post, 0, T, pred), block=block, cross_covariances=True)
    assert sm.smoothed_cross_covariances.shape[2] == T - 1
    for k, ref in zip(OUTPUTS, yardstick(name, T)):
        got = host(getattr(sm, k))
        if ref.size == 0:
            assert got.size == 0
            continue
        err = cm.rel_err(got, ref)
        elem = cm.elem_err(got, ref, ev=2) if "covariances" in k else None
        print(f"parity {name} T={T} block={block} {'given' if pred else 'recomputed'} {k}: rel {err:.2e}"
              + (f" elem {elem:.2e}" if elem is not None else ""))
        assert err <= TOL, (k, err)
        if elem is not None:
            assert elem <= TOL, (k, elem)


@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
@pytest.mark.parametrize("T,block", SHAPES)
@pytest.mark.parametrize("name", psc.MODELS)
def test_parity_with_the_float64_recursion(name, T, block, pred):
    check_parity(name, T, block, pred)


@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
@pytest.mark.parametrize("T,block", SHAPES)
def test_marginally_stable_model(T, block, pred):
    """The constant-velocity model: unit eigenvalues, singular G Q G^T."""
    check_parity("cv", T, block, pred)


@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
def test_one_block_is_the_serial_smoother_bit_for_bit(pred, layout):
    """T <= block: the emit launch alone is rts_smoother's recursion; also with a carry."""
    p, post = streams("4x2")
    later, early = cut(post, 37, 74, pred), cut(post, 0, 37, pred)
    kw = dict(cross_covariances=True, layout=layout, return_carry=True)
    par, pc = bfa.parallel_rts_smoother(p, later, block=64, **kw)
    seq, sc = bfa.rts_smoother(p, later, **kw)
    assert par.smoothed_cross_covariances.shape[2] == 36
    for x, y in zip(tuple(getattr(par, k) for k in OUTPUTS) + tuple(pc), tuple(getattr(seq, k) for k in OUTPUTS) + tuple(sc)):
        assert same_bits(x, y)
    # the steps before, from that carry: cross-covariances at every step of the chunk; T = block
    par2 = bfa.parallel_rts_smoother(p, early, carry=sc, block=37, cross_covariances=True, layout=layout)
    seq2 = bfa.rts_smoother(p, early, carry=sc, cross_covariances=True, layout=layout)
    assert par2.smoothed_cross_covariances.shape[2] == 37
    for k in OUTPUTS:
        assert same_bits(getattr(par2, k), getattr(seq2, k)), k


@pytest.mark.parametrize("T,lo", [(301, 300), (303, 300)], ids=["one-step-block", "ragged-block-of-3"])
@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
def test_last_block_is_the_serial_smoother_bit_for_bit(pred, T, lo):
    """block = 4: the steps from `lo` on are the last block, rts_smoother's recursion from the call's end; the earlier steps
    agree to tolerance."""
    p, post = streams("4x2")
    part = cut(post, 0, T, pred)
    par = bfa.parallel_rts_smoother(p, part, block=4, cross_covariances=True)
    seq = bfa.rts_smoother(p, part, cross_covariances=True)
    for k in OUTPUTS:
        assert same_bits(getattr(par, k)[:, :, lo:], getattr(seq, k)[:, :, lo:]), k
        assert cm.rel_err(host(getattr(par, k)), host(getattr(seq, k))) <= TOL, k


@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
def test_bits_do_not_depend_on_the_launch(pred):
    T, block = 301, 4
    p, post5 = streams("4x2", 5)
    part = cut(post5, 0, T, pred)
    call = lambda **kw: bfa.parallel_rts_smoother(p, part, block=block, **kw)
    full, carry = call(cross_covariances=True, return_carry=True)
    # the same call twice
    again, carry2 = call(cross_covariances=True, return_carry=True)
    for x, y in zip(tuple(getattr(full, k) for k in OUTPUTS) + tuple(carry), tuple(getattr(again, k) for k in OUTPUTS) + tuple(carry2)):
        assert same_bits(x, y)
    # trajectory b alone
    for b in (0, 3):
        one_post = part._replace(**{k: getattr(part, k)[b:b + 1] for k in ("weights", "means", "covariances")
                                    + (PRED if pred else ())})
        one = bfa.parallel_rts_smoother(p, one_post, block=block, cross_covariances=True)
        for k in OUTPUTS:
            assert same_bits(getattr(one, k)[0], getattr(full, k)[b]), (b, k)
    # layouts; cross-covariances off
    inner = call(cross_covariances=True, layout="batch_inner")
    plain = call()
    assert plain.smoothed_cross_covariances is None
    for k in OUTPUTS:
        assert same_bits(getattr(inner, k), getattr(full, k)), k
        if "cross" not in k:
            assert same_bits(getattr(plain, k), getattr(full, k)), k
    # out= reuse and a reused workspace pre-filled with 0xFF against a fresh one
    ws = torch.full((bfa.parallel_rts_workspace_bytes(4, 5, T, block) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    reused = call(out=again, workspace=ws)
    assert reused.smoothed_means.data_ptr() == again.smoothed_means.data_ptr()
    twice = call(cross_covariances=True, workspace=ws)
    for k in OUTPUTS:
        assert same_bits(getattr(reused, k), getattr(full, k)), k
        assert same_bits(getattr(twice, k), getattr(full, k)), k
    # the carry-out is the smoothed step 0
    assert same_bits(carry.means, full.smoothed_means[:, 0, 0])
    assert same_bits(carry.covariances, full.smoothed_covariances[:, 0, 0])


def test_chunks_through_the_carry():
    """[600, 1203) then [0, 600) with its carry against one shot.  Not bit-equal: the one-shot state after step 599 comes from
    the scan, the chunked one from the later chunk's emit launch."""
    p, post = streams("4x2")
    whole = bfa.parallel_rts_smoother(p, post, block=4, cross_covariances=True)
    second, carry = bfa.parallel_rts_smoother(p, cut(post, 600, TMAX), block=4, cross_covariances=True, return_carry=True)
    first = bfa.parallel_rts_smoother(p, cut(post, 0, 600), carry=carry, block=4, cross_covariances=True)
    assert first.smoothed_cross_covariances.shape[2] == 600 and second.smoothed_cross_covariances.shape[2] == TMAX - 601
    assert same_bits(carry.means, second.smoothed_means[:, 0, 0])
    assert same_bits(carry.covariances, second.smoothed_covariances[:, 0, 0])
    for k in OUTPUTS:
        joined = np.concatenate([host(getattr(first, k)), host(getattr(second, k))], axis=2)
        err = cm.rel_err(joined, host(getattr(whole, k)))
        print(f"chunks {k}: rel {err:.2e}")
        assert err <= TOL, k


@pytest.mark.parametrize("pred", [True, False], ids=["given", "recomputed"])
@pytest.mark.parametrize("field,index", [("means", (1, 0, 7, 0)), ("covariances", (1, 0, 7, 0, 0))])
def test_nan_input_stays_in_its_trajectory_and_flows_backwards(field, index, pred):
    """NaN at (b = 1, t = 7), T = 64, block = 4 (steps 4 ... 6 share the NaN's block).  The NaN pattern of every output is
    rts_smoother's on the same streams: finite after step 7 with the clean run's bits, and NaN at every step <= 7 in every output
    that reads the entry -- all three for a NaN covariance; the smoothed means alone for a NaN mean, which neither recursion
    reads for a covariance.  The other trajectories keep the clean run's bits."""
    p, post = streams("4x2")
    T = 64
    clean_post = cut(post, 0, T, pred)
    bad = {k: (getattr(clean_post, k).clone() if getattr(clean_post, k) is not None else None) for k in ("means", "covariances") + PRED}
    bad[field][index] = float("nan")
    bad_post = clean_post._replace(**bad)
    clean = bfa.parallel_rts_smoother(p, clean_post, block=4, cross_covariances=True)
    got = bfa.parallel_rts_smoother(p, bad_post, block=4, cross_covariances=True)
    seq = bfa.rts_smoother(p, bad_post, cross_covariances=True)
    for k in OUTPUTS:
        v = host(getattr(got, k))
        assert np.array_equal(np.isnan(v), np.isnan(host(getattr(seq, k)))), k
        assert np.isfinite(v[1, :, 8:]).all(), k
        if field == "covariances" or k == "smoothed_means":
            assert np.isnan(v[1, 0, :8]).reshape(8, -1).any(axis=1).all(), k   # (step 7 itself: the entries the NaN reaches)
            assert np.isnan(v[1, 0, :7 if "cross" not in k else 6]).all(), k
        assert same_bits(getattr(got, k)[1, :, 8:], getattr(clean, k)[1, :, 8:]), k
        for b in (0, 2):
            assert same_bits(getattr(got, k)[b], getattr(clean, k)[b]), (k, b)


def test_parallel_kalman_smoother_end_to_end():
    a, ys, init, _ = psc.case("4x2", B, TMAX)
    p = cm.product_params(a)
    par = bfa.parallel_kalman_smoother(p, ys[:, :301], initial_means=init, block=4, cross_covariances=True)
    seq = bfa.kalman_smoother(p, ys[:, :301], initial_means=init, cross_covariances=True)
    for k in ("filtered_means", "filtered_covariances") + OUTPUTS:
        err = cm.rel_err(host(getattr(par, k)), host(getattr(seq, k)))
        print(f"end to end {k}: rel {err:.2e}")
        assert err <= TOL, k
    # against the exact dense joint Gaussian, at the tolerance test_kalman_smoother_vs_exact_posterior uses (the filter's gain
    # carries the reference's +1e-6 on every entry of S)
    T = 48
    sm = bfa.parallel_kalman_smoother(p, ys[:, :T], initial_means=init, block=4, cross_covariances=True)
    for b in range(B):
        dm, dP, dC = psc.dense_posterior(a, ys[b, :T].astype(np.float64), init[b], a["P0"])
        e = (cm.rel_err(host(sm.smoothed_means[b, 0]), dm), cm.rel_err(host(sm.smoothed_covariances[b, 0]), dP),
             cm.rel_err(host(sm.smoothed_cross_covariances[b, 0]), dC))
        print(f"dense b={b}: {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
        assert max(e) < 1e-4, (b, e)


@pytest.mark.parametrize("Bd,Td", [(1, 5000), (64, 300), (4096, 16)])
def test_default_block(Bd, Td):
    a = psc.model("4x2")
    ys = cm.simulate_batch(a, Bd, Td, seed=3)
    sm = bfa.parallel_kalman_smoother(cm.product_params(a), ys, cross_covariances=True)
    for k in OUTPUTS:
        assert torch.isfinite(getattr(sm, k)).all(), k
