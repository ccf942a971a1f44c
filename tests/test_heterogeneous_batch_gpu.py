"""Linear-model kernels on batches in which every trajectory -- and every Gaussian-sum component -- has a covariance of its
own (tests/heterogeneous_cases.py; tests/test_heterogeneous_batch_cpu.py shows for every case that trajectories differ by
>= 100 tolerances and that the reference has headroom).  With one P0 for the whole batch the covariance streams and gains
of a linear model are identical in every slot, and a kernel that reads carry.P_in of another chain, stages or stores a
covariance tile into another slot, reuses a neighbour's gain, or hands a carry to the wrong slot passes every other test.

A. the Kalman entry point on all four kernel families against the per-trajectory reference (all five streams,
   log-likelihood, carry; whole arrays), with a witness that the fast path ran;
B. Gaussian sums of a linear model with one prior per (b, k): step 0 from the given priors, every later step teacher-forced
   on the engine's own carry, the fast path against the run-time-dimension kernel;
C. placement: the batch reversed along B (and K) computes the same bits in the mirrored slots;
D. two chunks through the carry == one shot, bit for bit;
E. the RTS smoother and the FFBS sampler on those heterogeneous filtered streams."""
import functools

import numpy as np
import pytest

from tests import common as cm
from tests import heterogeneous_cases as hc
from tests.test_kalman_gpu import _run as _kalman_run
from tests.test_smoother_gpu import _oracle as _rts_oracle, _check as _rts_check
from tests.test_sampler_gpu import _oracle as _ffbs_oracle, _check as _ffbs_check, _noise, _dev, SPLS

pytestmark = pytest.mark.gpu

FORCED = {"force_generic": 1}
KF_CARRY = ("weights", "means", "covariances")


def _np(x):
    return x.detach().cpu().numpy()


def _is_forced(c):
    """The cases of the run-time-dimension family that a compiled instance would take otherwise."""
    return c["family"] == "runtime" and c["n"] <= 8


def _kalman(name, layout="reference", mode=-1, lanes=0, forced=None, data=None, carry=None, cols=slice(None)):
    """kalman_filter on the case (options as tests/test_kalman_gpu.py::_run sets them): (posterior, loglik, carry)."""
    c = hc.CASES[name]
    ys, m0s, P0s = hc.data(name) if data is None else data
    kw = dict(return_loglik=True, return_carry=True)
    if _is_forced(c) if forced is None else forced:
        kw["options"] = FORCED
    if carry is None:
        kw["initial_covariances"] = np.array(P0s[:, 0])       # (copies: the shared arrays are read-only)
    else:
        kw["carry"] = carry
    return _kalman_run(hc.model(name), np.array(ys[:, cols]), None if carry is not None else np.array(m0s[:, 0]), layout, mode,
                       lanes, **kw)


def _gsf(name, forced=None, data=None, carry=None, cols=slice(None)):
    import bayesianfiltering_amd as bfa
    c = hc.CASES[name]
    ys, m0s, P0s = hc.data(name) if data is None else data
    kw = dict(return_loglik=True, return_carry=True)
    if (c["family"] == "runtime") if forced is None else forced:
        kw["options"] = FORCED
    if carry is None:
        kw.update(initial_means=np.array(m0s), initial_covariances=np.array(P0s))
    else:
        kw["carry"] = carry
    return bfa.gaussian_sum_filter(cm.product_params(hc.model(name)), np.array(ys[:, cols]), c["K"], 1, **kw)


@functools.lru_cache(maxsize=None)
def _kalman_default(name, forced=False):
    """The case through the entry point's own routing (or forced onto the run-time-dimension kernel), run once."""
    return _kalman(name, forced=forced)


def _spread(B):
    return range(B) if B <= 8 else sorted({0, 1, 63, 64, B // 2, B - 2, B - 1})


def _teacher_forced(name, post, ll):
    """Worst one-step errors over a spread of trajectories (recorded beside the free-running figures, not asserted: a slot
    mix-up inside the scan shows in the free-running comparison of the whole array)."""
    c = hc.CASES[name]
    a = hc.model(name)
    ys = hc.data(name)[0]
    m, P, pm, pP = (_np(getattr(post, k))[:, 0] for k in hc.STREAMS)
    l = _np(ll)[:, 0]
    worst = {}
    for b in _spread(c["B"]):
        w = cm.one_step_parity(a, ys[b], pm[b], pP[b], m[b], P[b], l[b], range(1, c["T"]))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    return worst


def _check_kalman(name, run, tag, **how):
    """All five streams, the log-likelihood and the carry of a Kalman run against the per-trajectory reference: whole
    arrays, the tolerances of the family's existing oracle test.  ``how``: the layout / mode / lanes of the run."""
    import torch
    c = hc.CASES[name]
    post, ll, carry = run
    ref = hc.reference(name)
    e = {}
    for k in hc.FIELDS:
        got = _np(getattr(post, k))
        assert got.shape == ref[k].shape, k
        e[k] = cm.rel_err(got, ref[k])
    e["loglik"] = cm.rel_err(_np(ll), ref["loglik"])
    # the carry is the last step's prediction, chain by chain: bit for bit the last entries of the run's own streams ...
    assert tuple(carry.weights.shape) == (c["B"], 1)
    assert torch.equal(carry.weights, post.weights[:, :, -1]), (name, tag)
    assert torch.equal(carry.means, post.predicted_means[:, :, -1]), (name, tag)
    assert torch.equal(carry.covariances, post.predicted_covariances[:, :, -1]), (name, tag)
    # ... and held against the reference on its own scale, after carry_T steps (= T but on kf-cv: hc.KALMAN_CASES says why)
    t = c["carry_T"] - 1
    if c["carry_T"] != c["T"]:
        short_post, _, carry = _kalman(name, cols=slice(0, c["carry_T"]), **how)
        assert torch.equal(carry.covariances, short_post.predicted_covariances[:, :, -1]), (name, tag)
    e["carry_weights"] = cm.rel_err(_np(carry.weights), ref["weights"][:, :, t])
    e["carry_means"] = cm.rel_err(_np(carry.means), ref["predicted_means"][:, :, t])
    e["carry_covariances"] = cm.rel_err(_np(carry.covariances), ref["predicted_covariances"][:, :, t])
    forced = _teacher_forced(name, post, ll)
    cm.record(f"heterogeneous_kalman[{c['family']}:{name}:{tag}]", free_running=e, teacher_forced=forced)
    print(f"{name} {tag}: free-running " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    print(f"{name} {tag}: teacher-forced " + ", ".join(f"{k} {v:.2e}" for k, v in forced.items()))
    for k, v in e.items():
        assert v < (c["tol_ll"] if k == "loglik" else c["tol"]), (name, tag, k, v)


def _witness(name, post):
    """The case again on the run-time-dimension kernel, which rounds differently: ``not torch.equal`` witnesses that the fast
    path ran (the entry point falls back to that kernel quietly where an instance is missing), as in tests/test_generic_gpu.py.
    Not on kf-cv and gsf-3-3-K5, where the two kernels produce the same bits (hc.KALMAN_CASES): there the outcome is recorded.
    Everywhere the two runs agree to the tolerance."""
    import torch
    c = hc.CASES[name]
    slow = _kalman_default(name, forced=True)[0]
    differs = not torch.equal(post.covariances, slow.covariances)
    cm.record(f"heterogeneous_witness[{c['family']}:{name}]", differs_from_runtime_kernel=float(differs))
    if c["witness"]:
        assert differs, name
    for k in hc.STREAMS:
        assert cm.rel_err(_np(getattr(post, k)), _np(getattr(slow, k))) < c["tol"], (name, k)


# ---- A -------------------------------------------------------------------------------------------------------------------
# lanes = lanes cooperating on one trajectory (0 = shipping default); mode 2 = LDS-staged stores (B = 130 = 2 * 64 + 2:
# whole waves staged, the tail of two through the strided kernel), mode 0 = strided stores
@pytest.mark.parametrize("lanes", [0, 1, 2, 4])
@pytest.mark.parametrize("layout,mode", [("reference", 2), ("reference", 0), ("batch_inner", -1)])
def test_kalman_register_kernel_cv(lanes, layout, mode):
    run = _kalman("kf-cv", layout, mode, lanes)
    _check_kalman("kf-cv", run, f"lanes{lanes}-{layout}-mode{mode}", layout=layout, mode=mode, lanes=lanes)
    _witness("kf-cv", run[0])


@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
@pytest.mark.parametrize("name", ["kf-3-2", "kf-7-4", "kf-8-4", "kf-4-2-b130"])
def test_kalman_register_kernel_random(name, layout):
    run = _kalman(name, layout)
    _check_kalman(name, run, layout, layout=layout)
    _witness(name, run[0])


@pytest.mark.parametrize("name", ["kf-4-2", "kf-8-4-forced", "kf-9-2", "kf-12-4"])
def test_kalman_runtime_dimension_kernel(name):
    import torch
    run = _kalman(name)
    _check_kalman(name, run, "forced" if _is_forced(hc.CASES[name]) else "routed")
    if _is_forced(hc.CASES[name]):      # the option took effect: the compiled instance rounds differently on these models
        fast = _kalman_default(name)[0]
        assert not torch.equal(run[0].covariances, fast.covariances), name
        for k in hc.STREAMS:
            assert cm.rel_err(_np(getattr(run[0], k)), _np(getattr(fast, k))) < hc.CASES[name]["tol"], (name, k)


@pytest.mark.parametrize("name", ["kf-16-8", "kf-17-3", "kf-32-32", "kf-24-12"])
def test_kalman_one_wave_matrix_core_kernel(name):
    run = _kalman_default(name)
    _check_kalman(name, run, "bf32")
    _witness(name, run[0])


@pytest.mark.parametrize("name", ["kf-64-32", "kf-40-24", "kf-48-20"])
def test_kalman_64_32_kernel(name):
    run = _kalman_default(name)
    _check_kalman(name, run, "mfma")
    _witness(name, run[0])


# ---- B -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.GSF_CASES))
def test_gaussian_sum_one_covariance_per_component(name):
    """Step 0 against the oracle's scan body on the GIVEN priors, every later step teacher-forced on the engine's own carry
    (cm.gsf_one_step_parity: needs no initial covariance and does not compound); streams 1e-5, weights 2e-5 absolutely
    (tests/test_generic_gpu.py::test_gaussian_sum_of_a_linear_model_on_the_matrix_cores).  The chain-wise free-running
    reference of tests/heterogeneous_cases.py is recorded beside it."""
    import torch
    c = hc.CASES[name]
    K, T, B, tol, tol_w = c["K"], c["T"], c["B"], c["tol"], c["tol_w"]
    ys = hc.data(name)[0]
    po = cm.oracle_params(hc.model(name))
    post, ll, carry = _gsf(name)
    got = {k: _np(getattr(post, k)) for k in hc.FIELDS}
    got["loglik"] = _np(ll)
    first, forced = {k: 0.0 for k in got}, {}
    for b in range(B):
        s0 = hc.gsf_first_step(name, b)
        for k in hc.STREAMS + ("loglik",):
            first[k] = max(first[k], cm.rel_err(got[k][b, :, 0], s0[k]))
        first["weights"] = max(first["weights"], float(np.max(np.abs(got["weights"][b, :, 0] - s0["weights"]))))
        w = cm.gsf_one_step_parity(po, K, ys[b], {k: got[k][b] for k in hc.FIELDS}, range(1, T))
        assert w["skipped"] == 0
        for k in hc.FIELDS:
            forced[k] = max(forced.get(k, 0.0), w[k][0])
    ref = hc.reference(name)
    free = {k: cm.rel_err(got[k], ref[k]) for k in hc.STREAMS + ("loglik",)}
    free["weights"] = float(np.max(np.abs(got["weights"] - ref["weights"])))
    cm.record(f"heterogeneous_gsf[{c['family']}:{name}]", first_step=first, teacher_forced=forced, free_running=free)
    for label, e in (("step 0", first), ("teacher-forced", forced), ("free-running (recorded)", free)):
        print(f"{name}: {label}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for e in (first, forced):
        for k in hc.STREAMS:
            assert e[k] < tol, (name, k, e[k])
        assert e["weights"] < tol_w, (name, e["weights"])
    assert first["loglik"] < c["tol_ll"], (name, first["loglik"])
    # the carry is the last step's prediction and weights, chain by chain
    cm.record(f"heterogeneous_gsf_carry[{c['family']}:{name}]",
              equals_own_stream=float(torch.equal(carry.means, post.predicted_means[:, :, -1]) and
                                      torch.equal(carry.covariances, post.predicted_covariances[:, :, -1])))
    assert cm.rel_err(_np(carry.means), got["predicted_means"][:, :, -1]) < tol
    assert cm.rel_err(_np(carry.covariances), got["predicted_covariances"][:, :, -1]) < tol
    assert np.max(np.abs(_np(carry.weights) - got["weights"][:, :, -1])) < tol_w
    if c["family"] != "runtime":        # fast path against the run-time-dimension kernel (the witness: see _witness)
        slow = _gsf(name, forced=True)[0]
        differs = not torch.equal(post.covariances, slow.covariances)
        cm.record(f"heterogeneous_witness[{c['family']}:{name}]", differs_from_runtime_kernel=float(differs))
        if c["witness"]:
            assert differs, name
        for k in hc.STREAMS:
            assert cm.rel_err(got[k], _np(getattr(slow, k))) < 1e-5, (name, k)
        assert np.max(np.abs(got["weights"] - _np(slow.weights))) < tol_w


# ---- C -------------------------------------------------------------------------------------------------------------------
def _mirrored(data, axes):
    return tuple(np.ascontiguousarray(np.flip(v, axis=axes if i else 0)) for i, v in enumerate(data))


# B without a ragged tail, so that every trajectory runs the same code in either slot.  No family's arithmetic depends on
# the slot: the register kernel's lane group g = lane / NL only selects addresses (csrc/kf_scan_group.hpp:103-128), the
# run-time-dimension kernel takes one workgroup per trajectory (csrc/generic_device.hpp:488), the one-wave kernel's wave
# index selects its LDS region only (csrc/kf_scan_bf32.hip:72-90), and the (64, 32) kernel's rotation s_rot permutes which
# physical wave plays which tile role, not what a role computes (csrc/kf_scan_mfma.hip:128-136) -- so every family is held
# to bit equality.
@pytest.mark.parametrize("name,B,layout", [("kf-cv", 128, "reference"), ("kf-cv", 128, "batch_inner"), ("kf-8-4", 128, "reference"),
                                           ("kf-12-4", 4, "reference"), ("kf-17-3", 4, "reference"), ("kf-40-24", 4, "reference")])
def test_kalman_placement_invariance(name, B, layout):
    import torch
    data = hc.data(name, B)
    one = _kalman(name, layout, data=data)
    two = _kalman(name, layout, data=_mirrored(data, 0))
    for k in hc.FIELDS:
        assert torch.equal(torch.flip(getattr(two[0], k), dims=[0]), getattr(one[0], k)), (name, k)
    assert torch.equal(torch.flip(two[1], dims=[0]), one[1]), (name, "loglik")
    for x, y, k in zip(two[2], one[2], KF_CARRY):
        assert torch.equal(torch.flip(x, dims=[0]), y), (name, "carry." + k)
    # (the comparison is not vacuous: neighbours differ)
    assert not torch.equal(one[0].covariances[0], one[0].covariances[1])


# Components reversed along K too.  Means, covariances and per-component log-likelihoods are chain-wise (register kernel:
# csrc/gsf_scan.hpp:100-135; matrix cores: chain = b K + k, csrc/kf_scan_bf32.hip:75-77, csrc/kf_scan_mfma.hip:137-139) and
# held to bit equality; the weights see the component order through the sum of reweight: 2e-5.
@pytest.mark.parametrize("name,B", [("gsf-4-2-K4", 128), ("gsf-16-8-K4", 4), ("gsf-33-7-K2", 4), ("gsf-12-4-K3", 4)])
def test_gaussian_sum_placement_invariance(name, B):
    import torch
    tol_w = hc.CASES[name]["tol_w"]
    data = hc.data(name, B)
    one = _gsf(name, data=data)
    two = _gsf(name, data=_mirrored(data, (0, 1)))
    back = lambda x: torch.flip(x, dims=[0, 1])
    for k in hc.STREAMS:
        assert torch.equal(back(getattr(two[0], k)), getattr(one[0], k)), (name, k)
    assert torch.equal(back(two[1]), one[1]), (name, "loglik")
    assert float((back(two[0].weights) - one[0].weights).abs().max()) < tol_w
    assert torch.equal(back(two[2].means), one[2].means) and torch.equal(back(two[2].covariances), one[2].covariances)
    assert float((back(two[2].weights) - one[2].weights).abs().max()) < tol_w
    assert not torch.equal(one[0].covariances[0, 0], one[0].covariances[0, 1])


# ---- D -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hc.CHUNK_CUTS))
def test_heterogeneous_carry_through_chunks(name):
    """Two chunks through return_carry= / carry= == the one-shot run on every element of every stream, the log-likelihood
    and the final carry: with covariances that differ per chain at the cut (by >= 100 tolerances, shown on the CPU), a carry
    written to or read from another slot shows."""
    import torch
    cut = hc.CHUNK_CUTS[name]
    run = _gsf if name in hc.GSF_CASES else _kalman
    whole = run(name)
    first = run(name, cols=slice(0, cut))
    second = run(name, carry=first[2], cols=slice(cut, None))
    for k in hc.FIELDS:
        assert torch.equal(torch.cat([getattr(first[0], k), getattr(second[0], k)], dim=2), getattr(whole[0], k)), (name, k)
    assert torch.equal(torch.cat([first[1], second[1]], dim=2), whole[1]), (name, "loglik")
    for x, y, k in zip(second[2], whole[2], KF_CARRY):
        assert torch.equal(x, y), (name, "carry." + k)
    assert not torch.equal(first[2].covariances[0], first[2].covariances[1])     # the carries still differ at the cut


# ---- E -------------------------------------------------------------------------------------------------------------------
# register instances n = 4 (B = 130: the constant-velocity batch and a random model) and n = 8 (B = 70), the run-time-dimension
# path at n = 12, 24, 48 (B = 5)
@pytest.mark.parametrize("name", list(hc.SMOOTHER_CASES))
def test_smoother_on_heterogeneous_streams(name):
    """rts_smoother on the posteriors of A against the float64 RTS over the GPU's own streams, trajectory by trajectory
    (tests/test_smoother_gpu.py::_oracle), at its 1e-5.  Measured (means, covariances, cross-covariances): kf-cv 7.1e-8,
    9.1e-6, 4.1e-6 -- the constant-velocity batch with its large early covariances is the sensitive input: a plain fp32
    evaluation of the recursion is 1.6e-5 from float64 there and at most 1.6e-6 on the other inputs
    (hc.smoother_fp32_error, tests/test_heterogeneous_batch_cpu.py::test_smoother_input_headroom); kf-4-2-b130 is the same
    shape with headroom -- the others <= 4.0e-7, 1.8e-6, 1.5e-6."""
    import bayesianfiltering_amd as bfa
    post = _kalman_default(name)[0]
    a = hc.model(name)
    sm = bfa.rts_smoother(cm.product_params(a), post, cross_covariances=True)
    _rts_check(sm, _rts_oracle(post, a["A"]), name=f"_heterogeneous[{name}]")


# n = 4 on the register kernel (every samples-per-lane instance, as test_parity_every_register_instance), n = 8 with a
# ragged batch of 70, n = 12 and 24 on the run-time-dimension kernel (as test_parity_runtime_dimension)
@pytest.mark.parametrize("name", ["kf-4-2", "kf-8-4", "kf-12-4", "kf-24-12"])
def test_sampler_on_heterogeneous_streams(name):
    import bayesianfiltering_amd as bfa
    c = hc.CASES[name]
    B, T, n, S = c["B"], c["T"], c["n"], 3
    post = _kalman_default(name)[0]
    a = hc.model(name)
    p = cm.product_params(a)
    xi = _noise((B, S, T, n), 500 + n)
    ref = _ffbs_oracle(post, a["A"], xi)
    x = bfa.posterior_sample(p, post, S, noise=_dev(xi))
    assert tuple(x.shape) == (B, S, T, n)
    _ffbs_check(x, ref, post, f"heterogeneous[{name}]")
    if n <= 8:
        for spl in SPLS:
            _ffbs_check(bfa.posterior_sample(p, post, S, noise=_dev(xi), options={"ffbs_spl": spl}), ref, post,
                        f"heterogeneous[{name}]_spl{spl}")
