"""parallel_kalman_filter(..., missing="nan") / observed= on the GPU: parity with both float64 yardsticks of
tests/parallel_kalman_missing_cases.py, the gap identities, the plain route's bits with nothing missing, the bits that must not
depend on the launch, the mask route, chunks through the carry, poison, the smoother and the sampler downstream.

Measured on an MI355X, worst over the 48 parity cases ("Gaps").  Against the scheme (bound 1e-5): rel_err 4.3e-7
(means), 2.9e-7 (covariances), 4.6e-7 (predicted means), 3.0e-7 (predicted covariances), 3.9e-7 (log-likelihood); elem_err(ev=2)
1.8e-6 / 1.5e-6 on the covariance streams.  Against the contract (bound: the case's float64 jitter gap + 1e-5): rel_err 2.1e-6,
1.0e-6, 2.3e-6, 1.0e-6, 2.3e-6; elem_err 8.3e-6 on both covariance streams.  Smoother downstream 3.0e-7 / 1.4e-6, sampler 1.7e-6.
Nothing missing: bit-equal to the plain route but at (3, 1): 1.6e-7 (means), 2.6e-8 (covariances) at (1000, 64).
"""
import numpy as np
import pytest
import torch

import bayesianfiltering_amd as bfa
from tests import common as cm
from tests import kalman_missing_cases as kc
from tests import parallel_kalman_cases as pk
from tests import parallel_kalman_missing_cases as pm

pytestmark = pytest.mark.gpu

TOL = pm.TOL
B = pm.B
NAN = float("nan")


def host(t):
    return t.cpu().numpy()


def same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def streams(post, ll):
    return {k: getattr(post, k) for k in kc.STREAMS} | {"loglik": ll}


def run(c, block, **kw):
    return bfa.parallel_kalman_filter(cm.product_params(c["a"]), c["gapped"], initial_means=c["init"], block=block,
                                      missing="nan", **kw)


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,block", pm.SHAPES)
@pytest.mark.parametrize("name", pm.MODELS)
def test_parity_with_the_scheme_and_the_contract(name, T, block):
    c = pm.case(name, T, block)
    gap = pm.jitter_gap(name, T, block)
    post, ll, carry = run(c, block, return_loglik=True, return_carry=True)
    got = streams(post, ll)
    assert host(got.pop("weights")).min() == 1.0 and host(post.weights).max() == 1.0
    for k, v in got.items():
        v = host(v)
        for yard, slack in (("scheme", None), ("contract", gap[k])):
            err = pm.errors(v, c[yard][k], k)
            for metric, e in err.items():
                bound = TOL + (slack[metric] if slack else 0.0)
                print(f"parity {name} T={T} block={block} {k} vs {yard}: {metric} {e:.2e} (bound {bound:.2e})")
                assert e <= bound, (k, yard, metric, e, bound)
    # the gap identities: a wholly missing step has log-likelihood 0 and keeps the prediction it started from, bit for bit.
    # Inside a block that prediction is the previous step's predicted stream.  At the first step of a block it is the block's
    # start state, which comes from the scan and is no output: the previous block's last prediction, emitted from ITS start
    # state, agrees with it to the tolerance of the streams, not bit for bit (in the float64 scheme neither).
    whole = ~c["mask"].any(axis=2)
    whole[:, 0] = False                                    # (step 0's prediction is the carry-in)
    assert (ll[torch.as_tensor(whole, device=ll.device)[:, None]] == 0).all()
    first = np.zeros_like(whole)
    first[:, ::block] = True
    for sel, exact in ((whole & ~first, True), (whole & first, False)):
        b, t = (torch.as_tensor(i, device=ll.device) for i in np.nonzero(sel))
        if not b.numel():
            continue
        for now, before in (("means", "predicted_means"), ("covariances", "predicted_covariances")):
            x, y = getattr(post, now)[b, 0, t], getattr(post, before)[b, 0, t - 1]
            if exact:
                assert same_bits(x, y), now
            else:
                assert cm.rel_err(host(x), host(y)) <= TOL + gap[before]["rel"], now
    # the carry is the last prediction
    assert same_bits(carry.means[:, 0], post.predicted_means[:, 0, -1])
    assert same_bits(carry.covariances[:, 0], post.predicted_covariances[:, 0, -1])
    assert host(carry.weights).tolist() == [[1.0]] * B


# ---- nothing missing through the new route ------------------------------------------------------------------------------------
# (n, m) = (3, 1) -- and (5, 1), which is no case here: the streams differ from the plain route's by 1.6e-7 over the block or
# blocks that follow block 0 and are bit-equal again after them.  The emit launch's block 0 is bit-equal at every pair, so the
# step's functions agree; what differs is the end state of block 0 that the FOLD launch computes with the same functions
# inlined into its own loop, where the compiler is free to contract a multiply-add of the m = 1 update differently.  The
# filter forgets a perturbation of its state in the last bit within a few dozen steps, which is why later blocks agree again.
NOT_BIT_EQUAL = {"3x1"}


@pytest.mark.parametrize("T,block", [(301, 4), (1000, 64), (8, 4), (37, 64)])
@pytest.mark.parametrize("name", pm.MODELS)
def test_nothing_missing_is_the_plain_route(name, T, block):
    """The fold selects entry 2^m - 1, the plain route's constants; the masked step with every row observed is the plain
    step's operations.  The streams are expected bit for bit; the log-likelihood's run-time count term may contract
    differently (it does at every m = 3) and is held to 1e-5.  NOT_BIT_EQUAL: the pairs whose streams leave the plain route's
    bits on the device; they are held to 1e-5 instead (DESIGN.md 6h has the distances)."""
    c = pm.case(name, T, block)
    p = cm.product_params(c["a"])
    plain, ll_plain = bfa.parallel_kalman_filter(p, c["ys"], initial_means=c["init"], block=block, return_loglik=True)
    new, ll_new = bfa.parallel_kalman_filter(p, c["ys"], initial_means=c["init"], block=block, return_loglik=True, missing="nan")
    for k in kc.STREAMS:
        x, y = getattr(new, k), getattr(plain, k)
        if name in NOT_BIT_EQUAL:
            e = cm.rel_err(host(x), host(y))
            print(f"nothing missing {name} T={T} block={block} {k}: rel {e:.2e}, bit-equal {same_bits(x, y)}")
            assert e <= TOL, k
        else:
            assert same_bits(x, y), k
    e = cm.rel_err(host(ll_new), host(ll_plain))
    print(f"nothing missing {name} T={T} block={block} loglik: rel {e:.2e}, bit-equal {same_bits(ll_new, ll_plain)}")
    assert e <= TOL


# ---- launch independence --------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_launch():
    T, block = 301, 4
    c = pm.case("4x2", T, block)
    p = cm.product_params(c["a"])
    yg, init = c["gapped"], c["init"]
    call = lambda **kw: bfa.parallel_kalman_filter(p, yg, initial_means=init, block=block, missing="nan", **kw)
    full, ll, carry = call(return_loglik=True, return_carry=True)
    again, ll2, carry2 = call(return_loglik=True, return_carry=True)
    for x, y in zip(full + (ll,) + tuple(carry), again + (ll2,) + tuple(carry2)):
        assert same_bits(x, y)
    for b in (0, kc.NONE, 4):                               # a trajectory alone: its neighbours' patterns do not reach it
        one = bfa.parallel_kalman_filter(p, yg[b:b + 1], initial_means=init[b:b + 1], block=block, missing="nan")
        for k in bfa.FULL5:
            assert same_bits(getattr(one, k)[0], getattr(full, k)[b]), (b, k)
    inner, ll_inner = call(layout="batch_inner", return_loglik=True)
    for k in bfa.FULL5:
        assert same_bits(getattr(inner, k), getattr(full, k)), k
    assert same_bits(ll_inner, ll)
    for fields in (("means",), bfa.FILTERED):
        part = call(fields=fields)
        for k in bfa.FULL5:
            assert (getattr(part, k) is None) == (k not in fields)
            if k in fields:
                assert same_bits(getattr(part, k), getattr(full, k)), (fields, k)
    ws = torch.full((bfa.parallel_kalman_workspace_bytes(4, 2, B, T, block) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    reused = call(out=again, workspace=ws)
    assert reused.means.data_ptr() == again.means.data_ptr()
    twice = call(workspace=ws)
    for k in bfa.FULL5:
        assert same_bits(getattr(reused, k), getattr(full, k)), k
        assert same_bits(getattr(twice, k), getattr(full, k)), k


# ---- observed= ------------------------------------------------------------------------------------------------------------------
def test_a_mask_gives_the_bits_of_nans_written_by_the_caller():
    T, block = 301, 4
    c = pm.case("4x2", T, block)
    p = cm.product_params(c["a"])
    by_nan, ll_nan = run(c, block, return_loglik=True)
    ys = torch.tensor(c["ys"]).cuda()
    before = ys.clone()
    by_mask, ll_mask = bfa.parallel_kalman_filter(p, ys, initial_means=c["init"], block=block, observed=c["mask"],
                                                  return_loglik=True)
    assert torch.equal(ys, before)                          # the caller's tensor is unchanged
    for k in bfa.FULL5:
        assert same_bits(getattr(by_mask, k), getattr(by_nan, k)), k
    assert same_bits(ll_mask, ll_nan)
    # a (B, T) mask of whole steps, and missing="nan" next to a mask
    steps = c["mask"].all(axis=2)
    a1 = bfa.parallel_kalman_filter(p, ys, initial_means=c["init"], block=block, observed=steps, missing="nan")
    a2 = bfa.parallel_kalman_filter(p, kc.gapped(c["ys"], steps[..., None]), initial_means=c["init"], block=block, missing="nan")
    for k in bfa.FULL5:
        assert same_bits(getattr(a1, k), getattr(a2, k)), k


# ---- chunks ---------------------------------------------------------------------------------------------------------------------
def test_chunks_through_the_carry_cut_inside_a_gap():
    """[0, 90) then [90, 301): the cut lies inside trajectory 4's long gap (steps 40 ... 139).  Not bit-equal: the one-shot start
    state of block 23 comes from the scan, the chunked one from the first chunk's emit launch."""
    T, block, cut = 301, 4, 90
    c = pm.case("4x2", T, block)
    p = cm.product_params(c["a"])
    assert not c["mask"][pm.LONG_GAP[0], cut - 5:cut + 5].any()
    whole, ll = run(c, block, return_loglik=True)
    kw = dict(block=block, missing="nan", return_loglik=True)
    first, ll1, carry = bfa.parallel_kalman_filter(p, c["gapped"][:, :cut], initial_means=c["init"], return_carry=True, **kw)
    second, ll2 = bfa.parallel_kalman_filter(p, c["gapped"][:, cut:], carry=carry, **kw)
    for k in pk.STREAMS:
        joined = np.concatenate([host(getattr(first, k)), host(getattr(second, k))], axis=2)
        assert cm.rel_err(joined, host(getattr(whole, k))) <= TOL, k
    assert cm.rel_err(np.concatenate([host(ll1), host(ll2)], axis=2), host(ll)) <= TOL
    assert host(second.weights).min() == 1.0


# ---- poison ---------------------------------------------------------------------------------------------------------------------
def _poison_runs(value):
    T, block = 64, 4
    c = pm.case("4x2", 301, 4)
    p = cm.product_params(c["a"])
    yg = np.array(c["gapped"][:, :T])
    yg[1, 7] = c["ys"][1, 7]                                # (trajectory 1 = FULL is observed anyway)
    yg[1, 20] = NAN                                         # a wholly missing step after the poison
    clean, ll_clean = bfa.parallel_kalman_filter(p, yg, initial_means=c["init"], block=block, missing="nan", return_loglik=True)
    bad = yg.copy()
    bad[1, 7, 0] = value
    post, ll, carry = bfa.parallel_kalman_filter(p, bad, initial_means=c["init"], block=block, missing="nan", return_loglik=True,
                                                 return_carry=True)
    return streams(clean, ll_clean), streams(post, ll), carry


def test_inf_in_an_observed_entry_poisons_its_trajectory_only():
    """+Inf at (b = 1, t = 7), block 4: NaN in every stream of trajectory 1 from step 7 on, finite before (steps 4 ... 6 share
    the block), the other trajectories keep their bits; the wholly missing step 20 after it reports log-likelihood 0."""
    clean, post, carry = _poison_runs(np.inf)
    for k in post:
        v = host(post[k])
        later = np.ones(v.shape[2], bool)
        later[:7] = False
        if k == "loglik":
            later[20] = False
        assert np.isnan(v[1][:, later]).all(), k
        assert np.isfinite(v[1, :, :7]).all(), k
        assert same_bits(post[k][1, :, :7], clean[k][1, :, :7]), k
        for b in (0, 2, 3, 4, 5):
            assert same_bits(post[k][b], clean[k][b]), (k, b)
    assert host(post["loglik"])[1, 0, 20] == 0.0
    assert np.isnan(host(post["weights"])[1, 0, 20])
    for x in carry:
        assert np.isnan(host(x)[1]).all() and np.isfinite(host(x)[[0, 2, 3, 4, 5]]).all()


def test_nan_in_the_same_place_is_a_gap():
    clean, post, carry = _poison_runs(NAN)
    for k in post:
        assert np.isfinite(host(post[k])).all(), k
        assert same_bits(post[k][1, :, :7], clean[k][1, :, :7]), k
    assert not same_bits(post["means"][1, :, 7], clean["means"][1, :, 7])
    assert host(post["weights"]).min() == 1.0


def test_without_the_keyword_a_nan_still_poisons():
    c = pm.case("4x2", 37, 64)
    post = bfa.parallel_kalman_filter(cm.product_params(c["a"]), c["gapped"], initial_means=c["init"], block=64)
    v = host(post.means)
    assert np.isnan(v[0]).all() and np.isfinite(v[kc.FULL]).all()      # step 0 is missing on every trajectory but FULL


# ---- downstream -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def downstream():
    """The 4x2 case at (301, 4) with the float64 RTS pass over both yardsticks' streams and the jitter gap between them."""
    c = pm.case("4x2", 301, 4)
    sm = {}
    for yard in ("contract", "scheme"):
        per = [kc.rts_f64(c["a"], {k: c[yard][k][b, 0] for k in pk.STREAMS}) for b in range(B)]
        sm[yard] = {"smoothed_means": np.stack([s[0] for s in per])[:, None],
                    "smoothed_covariances": np.stack([s[1] for s in per])[:, None]}
    gap = {k: pm.errors(sm["scheme"][k], sm["contract"][k], k) for k in sm["contract"]}
    return c, sm, gap


def test_smoother_downstream(downstream):
    c, sm, gap = downstream
    got = bfa.parallel_kalman_smoother(cm.product_params(c["a"]), c["gapped"], initial_means=c["init"], block=4, missing="nan")
    for k in ("smoothed_means", "smoothed_covariances"):
        for metric, e in pm.errors(host(getattr(got, k)), sm["contract"][k], k).items():
            bound = TOL + gap[k][metric]
            print(f"smoother {k}: {metric} {e:.2e} (bound {bound:.2e})")
            assert e <= bound, (k, metric, e, bound)
    by_mask = bfa.parallel_kalman_smoother(cm.product_params(c["a"]), c["ys"], initial_means=c["init"], block=4, observed=c["mask"])
    assert same_bits(by_mask.smoothed_means, got.smoothed_means)


def test_sampler_downstream(downstream):
    """The same noise through the parallel pair and through the serial pair: the samples differ by fp32 rounding and by the
    jitter of the folded steps, whose worth is the float64 distance between backward samples over the two yardsticks."""
    c, sm, _ = downstream
    p = cm.product_params(c["a"])
    S, T, n = 3, 301, 4
    noise = torch.randn(B, S, T, n, generator=torch.Generator().manual_seed(7))
    z = noise.numpy().astype(np.float64)
    both = [np.stack([pm.backward_samples_f64(c["a"], {k: c[yard][k][b, 0] for k in pk.STREAMS}, z[b]) for b in range(B)])
            for yard in ("scheme", "contract")]
    gap = cm.rel_err(both[0], both[1])
    noise = noise.cuda()
    par = bfa.parallel_kalman_posterior_sample(p, c["gapped"], S, None, noise=noise, initial_means=c["init"], block=4, missing="nan")
    seq = bfa.kalman_posterior_sample(p, c["gapped"], S, None, noise=noise, initial_means=c["init"], missing="nan")
    assert torch.isfinite(par).all() and par.shape == seq.shape
    e = cm.rel_err(host(par), host(seq))
    bound = TOL + gap
    print(f"sampler: rel {e:.2e} (bound {bound:.2e}), against float64 over the scheme {cm.rel_err(host(par), both[0]):.2e}")
    assert e <= bound
