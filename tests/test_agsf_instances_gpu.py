"""GPU sweep of the augmented Gaussian-sum register kernels (csrc/agsf_scan.hpp) over every compiled instance and launch geometry:
8 extended-Kalman instances (n, m) and 5 unscented ones (n, dq, m, dr), each with one wave per trajectory and -- up to n = 4 -- with
2, 4, 8 and 16 waves, 61 kernels, against the NumPy oracle.  The cases live in tests/agsf_instance_cases.py;
tests/test_agsf_instances_cpu.py shows, without a GPU, that each is finite, not degenerate and drawn with room to spare, and that
together they reach exactly the compiled table.

What is asserted.
(1) Parity, every case: the leaves drawn at every step are EQUAL to the oracle's (never relaxed); shapes as the reference returns
    them; means and covariances norm-wise (cm.rel_err) within 2e-5 for extended nodes (the bound of tests/test_agsf_gpu.py) and
    max(2e-5, 8 d32) for unscented ones, d32 being the distance between the oracle and its twin with a float32 sqrtm, measured per
    case on the CPU (the rule of tests/test_agsf_generic_gpu.py); weights np.allclose for jr.choice, rtol 3e-4 / atol 1e-7 for
    optimal resampling (the bound of test_optimal_variant), whose reference weights are not 1 / N0.
(2) Position in the batch (one wave per trajectory: 16 or 4 trajectories per workgroup, full workgroups and a ragged tail): the
    single-trajectory call equals the batched call's row bit for bit.
(3) Linear rows: the device's covariances against a float64 recursion teacher-forced from the device's own previous covariances and
    drawn leaves, within max(2e-5, 8 x the float32 oracle's own distance to the same formula).
(4) Two chunks through the carry, cut at an odd step, equal the single call bit for bit, optimal resampling's unequal carried
    weights included; so does the final carry.
(5) A nonlinear registry model at an uncompiled small shape is refused with extended nodes, and runs on the run-time-dimension
    kernel on request.
Every figure is printed before it is asserted (pytest -s shows them; DESIGN.md 4e records the worst)."""
import functools

import numpy as np
import pytest

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import agsf_instance_cases as ic
from tests import common as cm
from tests.test_agsf_generic_gpu import _float32_sqrtm

pytestmark = pytest.mark.gpu
F32 = np.float32
STREAMS = ("weights", "means", "covariances", "leaf_indices")


def _bfa():
    import bayesianfiltering_amd as bfa
    return bfa


def _call(name, ys, nc=None, u=None, **kw):
    """The entry point of the case's variant and node kind on the emissions ``ys`` (inputs ``u``)."""
    bfa = _bfa()
    c = ic.CASES[name]
    pp = ic.product_model(c["row"])
    args = (np.array(ys), c["nc"] if nc is None else nc, None, 1, (0.1, 0.1), u)
    if c["uparams"] is not None:
        fn = (bfa.speedy_unscented_agsf, bfa.unscented_agsf)[c["variant"]]
        return fn(pp, bfa.ParamsUKF(*c["uparams"]), *args, return_leaf_indices=True, **kw)
    fn = (bfa.speedy_augmented_gaussian_sum_filter, bfa.augmented_gaussian_sum_filter, bfa.augmented_gaussian_sum_filter_optimal)[c["variant"]]
    return fn(pp, *args, return_leaf_indices=True, **kw)


def _streams(post, aux):
    return {"weights": post.weights, "means": post.means, "covariances": post.covariances, "leaf_indices": aux["leaf_indices"]}


@functools.lru_cache(maxsize=None)
def _batched(name):
    """The device's run of the whole batch of a case, as tensors (computed once; nothing writes to them)."""
    ys, init = ic.data(name)
    post, aux = _call(name, ys, u=ic.inputs(name), initial_means=np.array(init))
    assert post.predicted_means is None and post.predicted_covariances is None
    return _streams(post, aux)


def _tolerance(name, b):
    """2e-5 for extended nodes; max(2e-5, 8 d32) for unscented ones."""
    if ic.CASES[name]["uparams"] is None:
        return 2e-5
    ref, _ = ic.reference(name, b)
    with _float32_sqrtm():
        twin, _ = ic.run_oracle(name, b)
    d32 = max(cm.rel_err(getattr(twin, k), getattr(ref, k)) for k in ("means", "covariances"))
    print(f"  {name}[{b}]: oracle float32-sqrtm floor d32 = {d32:.2e} -> tolerance {max(2e-5, 8 * d32):.1e}")
    return max(2e-5, 8 * d32)


def _check(got, name, b, tol=None):
    """``got``: the four streams of ONE trajectory as numpy arrays, against the oracle on trajectory b of the case."""
    c = ic.CASES[name]
    ref, _ = ic.reference(name, b)
    tol = _tolerance(name, b) if tol is None else tol
    errs = {k: cm.rel_err(got[k], getattr(ref, k)) for k in ("means", "covariances")}
    ew = float(np.max(np.abs(got["weights"] - ref.weights) / np.maximum(np.abs(ref.weights), 1e-30)))
    same = np.array_equal(got["leaf_indices"], ic.oracle_leaf_indices(name, b))
    print(f"  {name}[{b}] device vs oracle: leaves {'equal' if same else 'DIFFER'}, means {errs['means']:.2e}, "
          f"covariances {errs['covariances']:.2e}, weights {ew:.2e} (rel); tolerance {tol:.1e}")
    cm.record(f"agsf_instances {ic.ROWS[c['row']]['kind']} {name}[{b}]", means=errs["means"], covariances=errs["covariances"], weights=ew, tol=tol)
    assert same, "resampled leaves differ"
    N0, T, n = c["nc"][0], c["T"], c["n"]
    assert got["means"].shape == (N0, T, n) and got["covariances"].shape == (N0, T, n, n) and got["weights"].shape == (N0, T)
    assert got["leaf_indices"].shape == (T, N0)
    for k, e in errs.items():
        assert e < tol, (name, b, k, e, tol)
    if c["variant"] == 2:
        assert np.allclose(got["weights"], ref.weights, rtol=3e-4, atol=1e-7), (name, b, ew)
        assert not np.allclose(ref.weights, 1.0 / N0)     # the point of the variant
    else:
        assert np.allclose(got["weights"], ref.weights)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_parity(name):
    """(1): every (row, tier, variant) -- that is every compiled instance on every launch geometry -- against the oracle on the
    referenced trajectories of its batch (the first, one in the middle of a full workgroup, the last of the ragged tail)."""
    c = ic.CASES[name]
    full = {k: v.cpu().numpy() for k, v in _batched(name).items()}
    assert full["means"].shape[:2] == (c["B"], c["nc"][0]) and full["leaf_indices"].shape == (c["B"], c["T"], c["nc"][0])
    for b in c["refs"]:
        _check({k: v[b] for k, v in full.items()}, name, b)


@pytest.mark.parametrize("name", [n for n, c in ic.CASES.items() if c["tier"] in ic.ONE_WAVE])
def test_position_in_the_batch(name):
    """(2): trajectory 20 (G1a) and the last trajectory of the tail workgroup, filtered alone -- first slot of the only workgroup --
    equal their rows of the batched call bit for bit: the slot-major carry records and the shadowing of the trajectories beyond B."""
    import torch
    c = ic.CASES[name]
    full = _batched(name)
    ys, init = ic.data(name)
    for b in ((20, c["B"] - 1) if c["tier"] == "G1a" else (c["B"] - 1,)):
        one = _streams(*_call(name, ys[b], u=ic.inputs(name), initial_means=np.array(init[b])))
        for k in STREAMS:
            same = torch.equal(one[k], full[k][b])
            print(f"  {name}[{b}] alone vs in the batch: {k} {'equal' if same else 'DIFFER'}")
            assert same, (name, b, k)


LINEAR = [n for n, c in ic.CASES.items() if ic.ROWS[c["row"]]["model"] == "linear"]


@pytest.mark.parametrize("name", LINEAR)
def test_linear_rows_against_float64_recursion(name):
    """(3): a second reference that does not share the oracle's float32 arithmetic.  For a linear model the covariance of a leaf is
    a function of its parent's covariance alone (ic.linear_covariances_f64); evaluated in float64 on the device's own previous
    covariances and drawn leaves it must reproduce the device's covariances within max(2e-5, 8 x floor), the floor being the
    distance of the float32 oracle from the same formula on its own run (for unscented nodes the larger of the oracle's and its
    float32-sqrtm twin's: the device takes its matrix square roots in float32)."""
    c = ic.CASES[name]
    P0 = ic.model_arrays(c["row"])["P0"]
    full = _batched(name)
    for b in c["refs"]:
        runs = [ic.reference(name, b)]
        if c["uparams"] is not None:
            with _float32_sqrtm():
                runs.append(ic.run_oracle(name, b))
        floor = max(cm.rel_err(post.covariances, ic.linear_covariances_f64(c["row"], c["nc"], aux["leaf_indices"], post.covariances, P0))
                    for post, aux in runs)
        covs, leaf = full["covariances"][b].cpu().numpy(), full["leaf_indices"][b].cpu().numpy()
        e = cm.rel_err(covs, ic.linear_covariances_f64(c["row"], c["nc"], leaf, covs, P0))
        tol = max(2e-5, 8 * floor)
        print(f"  {name}[{b}] covariances vs float64 recursion: device {e:.2e}, float32 oracle {floor:.2e}; tolerance {tol:.1e}")
        cm.record(f"agsf_instances_f64 {name}[{b}]", device=e, oracle=floor, tol=tol)
        assert e < tol, (name, b, e, tol)


CHUNKED = [n for n, c in ic.CASES.items() if c["row"] in ("e22-sv", "e33-l63", "u3311-l63") and c["tier"] in ("G1a", "G2") and c["variant"] in (0, 2)]


@pytest.mark.parametrize("name", CHUNKED)
def test_chunks_through_the_carry(name):
    """(4): 3 steps (1 step where a replacement has shortened the series to 3), then the rest from the returned carry, on the whole
    batch: means, covariances, weights and drawn leaves equal the single call's bit for bit, and so does the carry at the end.
    With optimal resampling the carried weights are unequal: the second chunk reads them back, each leaf the weight of ITS parent
    component."""
    import torch
    c = ic.CASES[name]
    ys, init = (np.array(v) for v in ic.data(name))
    u = ic.inputs(name)
    cut = 3 if c["T"] > 4 else 1      # an odd step inside the series (a replacement may have shortened it)
    whole, wa = _call(name, ys, u=u, initial_means=init, return_carry=True)
    p1, a1 = _call(name, ys[:, :cut], u=None if u is None else u[:cut], initial_means=init, return_carry=True)
    p2, a2 = _call(name, ys[:, cut:], u=None if u is None else u[cut:], carry=a1["carry"], return_carry=True)
    one, s1, s2 = _streams(whole, wa), _streams(p1, a1), _streams(p2, a2)
    for k in STREAMS:
        same = torch.equal(torch.cat([s1[k], s2[k]], dim=1 if k == "leaf_indices" else 2), one[k])
        print(f"  {name} {cut} + {c['T'] - cut} steps vs {c['T']}: {k} {'equal' if same else 'DIFFER'}")
        assert same, (name, k)
        assert torch.equal(one[k], _batched(name)[k]), (name, k)      # (and returning the carry changes nothing)
    for k in ("weights", "means", "covariances"):
        assert torch.equal(getattr(a2["carry"], k), getattr(wa["carry"], k)), (name, "carry", k)
    if c["variant"] == 2:
        w = a1["carry"].weights.cpu().numpy()
        assert not np.allclose(w, 1.0 / c["nc"][0])      # the carry that went through carry= was an unequal one


def test_uncompiled_nonlinear_shape_is_refused_or_runs_on_request():
    """(5): Lorenz-96 with six states and three observations is no compiled (n, m) pair: extended nodes refuse it, naming the
    dimensions (the analytic Jacobians of the registry's nonlinear functions exist in the compiled instances only); with
    options={"agsf_force_generic": 1} the same call runs on the run-time-dimension kernel and matches the oracle."""
    bfa = _bfa()
    nl = bfa.nonlinearities
    n, m, T, nc = 6, 3, 8, (3, 2, 2)
    arr = (np.zeros(n, F32), np.eye(n, dtype=F32), np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32), np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))
    po = go.ParamsNLSSM(arr[0], arr[1], om.Lorenz96(n), arr[2], arr[3], om.PickEven(n), arr[4], arr[5])
    pp = bfa.ParamsNLSSM(arr[0], arr[1], nl.lorenz96(n), arr[2], arr[3], nl.pick_even(n), arr[4], arr[5])
    ys = go.sample_ssm(po, otf.PRNGKey(2), T)[1]
    init = np.random.default_rng(1).normal(size=(nc[0], n)).astype(F32)
    with pytest.raises(bfa.BayesFiltError, match=r"\(n=6, m=3\) is not compiled in") as ei:
        bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, initial_means=init)
    assert ei.value.code == -2      # BF_EUNSUPPORTED (include/bayesfilt.h)
    ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys, nc, initial_means=init, debug=True)
    post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, initial_means=init, return_leaf_indices=True,
                                                         options={"agsf_force_generic": 1})
    idx = np.stack([np.minimum(otf.choice_indices(otf.cumsum_assoc(w), otf.uniform(otf.PRNGKey(0), nc[0])), w.size - 1) for w in raux["pre_weights"]])
    same = np.array_equal(aux["leaf_indices"].cpu().numpy(), idx)
    errs = {k: cm.rel_err(getattr(post, k).cpu().numpy(), getattr(ref, k)) for k in ("means", "covariances")}
    print(f"  lorenz96(6) on request: leaves {'equal' if same else 'DIFFER'}, means {errs['means']:.2e}, covariances {errs['covariances']:.2e}")
    assert same
    assert tuple(post.means.shape) == (nc[0], T, n) and tuple(post.covariances.shape) == (nc[0], T, n, n)
    assert max(errs.values()) < 2e-5, errs
    assert np.allclose(post.weights.cpu().numpy(), ref.weights)
    with pytest.raises(bfa.BayesFiltError):      # the option was that call's only
        bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, initial_means=init)
