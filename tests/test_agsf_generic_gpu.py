"""GPU parity of the run-time-dimension augmented Gaussian-sum filters (csrc/agsf_generic.hip: the tree's nodes take turns in
LDS; any of n, dq, m, dr above 8, or options={"agsf_force_generic": 1}) against the NumPy oracle
(gaussfiltax/inference.py:458-1300).  The configurations live in tests/agsf_generic_cases.py; tests/test_agsf_generic_cpu.py
shows, without a GPU, that each of them is finite, not degenerate and drawn with room to spare.

What is asserted.  The leaves drawn at every step are EQUAL to the oracle's (never relaxed).  Means and covariances, norm-wise
(cm.rel_err): extended nodes 2e-5 (the bound of tests/test_agsf_gpu.py); unscented nodes max(2e-5, 8 d32), d32 being the distance
between the oracle and its twin with a float32 sqrtm -- the rule of tests/test_ugsf_generic_gpu.py, measured here per case on
the CPU.  Weights: np.allclose for jr.choice (they are 1 / N0), 5e-5 absolute for optimal resampling.  Every figure is printed
before it is asserted (pytest -s shows them; DESIGN.md 4d records them)."""
import contextlib

import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import agsf_generic_cases as ac
from tests import common as cm

pytestmark = pytest.mark.gpu
F32 = np.float32
FORCE = {"agsf_force_generic": 1}


def _bfa():
    import bayesianfiltering_amd as bfa
    return bfa


def _sqrtm_f32(P):
    """go.sym_sqrtm with the eigen-decomposition in float32: the precision the device works in."""
    P = np.asarray(P, dtype=F32)
    if not np.all(np.isfinite(P)):
        return np.full(P.shape, np.nan, dtype=F32)
    lam, V = np.linalg.eigh(P)
    return ((V * np.sqrt(np.maximum(lam, F32(0)))) @ V.T).astype(F32)


@contextlib.contextmanager
def _float32_sqrtm():
    keep = go.sym_sqrtm
    go.sym_sqrtm = _sqrtm_f32
    try:
        yield
    finally:
        go.sym_sqrtm = keep


def _tolerance(name, b=0):
    """2e-5 for extended nodes; max(2e-5, 8 d32) for unscented ones."""
    if ac.CASES[name]["uparams"] is None:
        return 2e-5
    ref, _ = ac.reference(name, b)
    with _float32_sqrtm():
        twin, _ = ac.run_oracle(name, b)
    d32 = max(cm.rel_err(getattr(twin, k), getattr(ref, k)) for k in ("means", "covariances"))
    print(f"  {name}: oracle float32-sqrtm floor d32 = {d32:.2e} -> tolerance {max(2e-5, 8 * d32):.1e}")
    return max(2e-5, 8 * d32)


def _run(name, b=None, options=None, **kw):
    """The device's run of a case: trajectory b, or the whole batch of the case."""
    bfa = _bfa()
    c = ac.CASES[name]
    ys, init = ac.data(name)
    ys, init = (np.array(v if b is None else v[b]) for v in (ys, init))     # (the shared arrays are read-only)
    pp = ac.product_model(name)
    args = (ys, c["nc"], None, 1, (0.1, 0.1), ac.inputs_of(name))
    kw = dict(initial_means=init, return_leaf_indices=True, options=options, **kw)
    if c["uparams"] is not None:
        fn = (bfa.speedy_unscented_agsf, bfa.unscented_agsf)[c["variant"]]
        return fn(pp, bfa.ParamsUKF(*c["uparams"]), *args, **kw)
    fn = (bfa.speedy_augmented_gaussian_sum_filter, bfa.augmented_gaussian_sum_filter, bfa.augmented_gaussian_sum_filter_optimal)[c["variant"]]
    return fn(pp, *args, **kw)


def _np(post, aux):
    return {"weights": post.weights.cpu().numpy(), "means": post.means.cpu().numpy(), "covariances": post.covariances.cpu().numpy(),
            "leaf_indices": aux["leaf_indices"].cpu().numpy()}


def _check(got, name, b=0, what=""):
    c = ac.CASES[name]
    ref, _ = ac.reference(name, b)
    tol = _tolerance(name, b)
    errs = {k: cm.rel_err(got[k], getattr(ref, k)) for k in ("means", "covariances")}
    ew = float(np.max(np.abs(got["weights"] - ref.weights)))
    same = np.array_equal(got["leaf_indices"], ac.oracle_leaf_indices(name, b))
    print(f"  {name}[{b}] {what} device vs oracle: leaves {'equal' if same else 'DIFFER'}, means {errs['means']:.2e}, "
          f"covariances {errs['covariances']:.2e}, weights {ew:.2e} (abs); tolerance {tol:.1e}")
    assert same, "resampled leaves differ"
    N0, T, n = c["nc"][0], c["T"], c["n"]
    assert got["means"].shape == (N0, T, n) and got["covariances"].shape == (N0, T, n, n) and got["weights"].shape == (N0, T)
    for k, e in errs.items():
        assert e < tol, (name, k, e, tol)
    if c["variant"] == 2:
        assert ew < 5e-5, (name, ew)
        assert not np.allclose(ref.weights, 1.0 / N0)     # the point of the variant
    else:
        assert np.allclose(got["weights"], ref.weights)
    return errs


@pytest.mark.parametrize("name", ["a-v0", "a-v1", "a-v2", "a-v0-unscented", "b-v1", "c-v0", "d-v2", "e-v1-n40", "e-v1-n20-unscented"])
def test_lorenz96_cases(name):
    """Cases a-d of the issue: Lorenz-96 with the even-state emission at n = 12 (one wave, 12 leaves; every variant; unscented
    nodes), n = 20, n = 9 with 72 leaves (more than a wave: four waves per workgroup), n = 12 with the reference's own (5, 5, 5)
    tree and optimal resampling.  Cases e add the workgroups that have four waves because of the dimension alone: n = 40 with
    extended nodes, n = 20 with unscented ones.  Without the kernel each of them is BF_EUNSUPPORTED."""
    post, aux = _run(name, 0)
    assert post.predicted_means is None and post.predicted_covariances is None
    _check(_np(post, aux), name)


@pytest.mark.parametrize("name", ["linear-unscented-v0", "linear-unscented-v1"])
def test_unscented_nodes_linear_awkward_sizes(name):
    """n = 9, dq = 3 (non-identity G), m = dr = 5, biases: the first shape of test_ugsf_generic_gpu.py under the (3, 2, 2) tree,
    speedy_unscented_agsf and unscented_agsf."""
    _check(_np(*_run(name, 0)), name)


@pytest.mark.parametrize("name", ["sine-tables-extended", "sine-tables-unscented"])
def test_sine_dynamics_inputs_and_per_step_tables(name):
    """n = 10, tree (2, 2, 2), T = 10, non-diagonal SPD tables Q_t / R_t and an input that switches 0 -> 1 halfway: a dense
    linear emission under extended nodes, the multiplicative-noise emission (the registry emission that reads the input;
    extended nodes cannot take R_t with it) under unscented nodes.  The constant-covariance posterior is a different one; a
    table with the wrong number of steps raises."""
    bfa = _bfa()
    c = ac.CASES[name]
    got = _np(*_run(name, 0))
    _check(got, name)
    d = ac.model_arrays(name)
    pp = ac.product_model(name)
    ys, init = (np.array(v) for v in ac.data(name))
    up = () if c["uparams"] is None else (bfa.ParamsUKF(*c["uparams"]),)
    fn = bfa.speedy_augmented_gaussian_sum_filter if c["uparams"] is None else bfa.speedy_unscented_agsf
    const, _ = fn(pp._replace(dynamics_noise_covariance=d["Q"], emission_noise_covariance=d["R"]), *up, ys[0], c["nc"], None, 1,
                  (0.1, 0.1), ac.inputs_of(name), initial_means=init[0])
    assert cm.rel_err(const.covariances.cpu().numpy(), got["covariances"]) > 1e-3     # the tables are not ignored
    for kw in ({"dynamics_noise_covariance": d["Qt"][:5]}, {"emission_noise_covariance": d["Rt"][:7]}):
        with pytest.raises(bfa.BayesFiltError, match="one matrix per step"):
            fn(pp._replace(**kw), *up, ys[0], c["nc"], None, 1, (0.1, 0.1), ac.inputs_of(name), initial_means=init[0])


def test_batch_and_chunks_bit_for_bit():
    """Case a, variant 0, three trajectories with different emissions and initial means: each row of the batched call equals its
    single-trajectory call, and two chunks (5 + 7 steps) through return_carry / carry equal the single scan -- exactly, on
    weights, means and covariances (and the drawn leaves)."""
    bfa = _bfa()
    name = "a-v0"
    c = ac.CASES[name]
    B = c["B"]
    full = _np(*_run(name))
    assert full["means"].shape == (B, c["nc"][0], c["T"], c["n"]) and full["leaf_indices"].shape == (B, c["T"], c["nc"][0])
    for b in range(B):
        one = _np(*_run(name, b))
        for k in one:
            assert np.array_equal(one[k], full[k][b]), (k, b)
        _check(one, name, b)
    ys, init = (np.array(v) for v in ac.data(name))
    pp = ac.product_model(name)
    p1, a1 = bfa.speedy_augmented_gaussian_sum_filter(pp, ys[:, :5], c["nc"], initial_means=init, return_carry=True,
                                                      return_leaf_indices=True)
    p2, a2 = bfa.speedy_augmented_gaussian_sum_filter(pp, ys[:, 5:], c["nc"], carry=a1["carry"], return_leaf_indices=True)
    for k in ("weights", "means", "covariances"):
        cat = np.concatenate([getattr(p1, k).cpu().numpy(), getattr(p2, k).cpu().numpy()], axis=2)
        assert np.array_equal(cat, full[k]), k
    assert np.array_equal(np.concatenate([a1["leaf_indices"].cpu().numpy(), a2["leaf_indices"].cpu().numpy()], axis=1), full["leaf_indices"])


@pytest.mark.parametrize("name", ["l96-n8", "cv-n4"])
def test_both_kernels_on_one_model(name):
    """The n = 8 Lorenz-96 model of test_agsf_gpu.py::test_lorenz96_and_errors and the linear n = 4 model under the (2, 2, 2) tree,
    through the register kernel and through options={"agsf_force_generic": 1}: the same leaves, each within the tolerance of
    the oracle and of the other."""
    reg = _np(*_run(name, 0))
    gen = _np(*_run(name, 0, options=FORCE))
    _check(reg, name, what="register kernel")
    _check(gen, name, what="run-time-dimension kernel")
    assert np.array_equal(reg["leaf_indices"], gen["leaf_indices"])
    # (that the option selects another kernel is shown by test_forced_kernel_lifts_the_leaf_limit_and_does_not_leak: on the
    # linear n = 4 model the two kernels' fused multiply-add chains coincide and so do their bits)
    for k in ("means", "covariances"):
        e = cm.rel_err(gen[k], reg[k])
        print(f"  between the kernels: {k} {e:.2e}")
        assert e < 2e-5, k


def test_forced_kernel_lifts_the_leaf_limit_and_does_not_leak():
    """(5, 5, 5) at n = 8: 125 leaves are more than the register kernel takes above n = 4.  With the option the call runs and
    matches the oracle; without it the call still raises -- also right after a call that carried the option."""
    bfa = _bfa()
    name = "l96-n8-555"
    with pytest.raises(bfa.BayesFiltError):
        _run(name, 0)
    _check(_np(*_run(name, 0, options=FORCE)), name)
    with pytest.raises(bfa.BayesFiltError):      # the option was this call's only
        _run(name, 0)


def test_refusals_before_any_launch():
    """What the kernel cannot hold is refused with the limit in the message: a model whose LDS need exceeds a workgroup's 160 KiB
    (n = 120: the prediction scratch alone is 3 x 120 x 124 floats), a tree above 256 leaves, and functions from source above
    dimension 8."""
    bfa = _bfa()
    nl = bfa.nonlinearities
    n = 120
    big = bfa.ParamsNLSSM(np.zeros(n, F32), np.eye(n, dtype=F32), nl.linear_dynamics(0.9 * np.eye(n, dtype=F32)), np.zeros(n, F32),
                          1e-2 * np.eye(n, dtype=F32), nl.linear_emission(np.ones((1, n), F32) / n), np.zeros(1, F32), 1e-1 * np.eye(1, dtype=F32))
    with pytest.raises(bfa.BayesFiltError, match="bytes of LDS"):
        bfa.speedy_augmented_gaussian_sum_filter(big, np.zeros((3, 1), F32), (2, 2, 2))
    with pytest.raises(bfa.BayesFiltError, match="bytes of LDS"):
        bfa.speedy_unscented_agsf(big, bfa.ParamsUKF(1, 0, 0), np.zeros((3, 1), F32), (2, 2, 2))
    ys = np.array(ac.data("a-v0")[0])
    pp = ac.product_model("a-v0")
    with pytest.raises(bfa.BayesFiltError, match="exceed the limit of 256"):
        bfa.speedy_augmented_gaussian_sum_filter(pp, ys[0], (7, 7, 7))
    src = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  for (int i = 0; i < BF_N; ++i) out[i] = sin(th[0] * x[i]) + q[i];
}
"""
    n = 10
    user = bfa.ParamsNLSSM(np.zeros(n, F32), np.eye(n, dtype=F32), nl.user_dynamics(src, n, theta=[1.5]), np.zeros(n, F32),
                           0.1 * np.eye(n, dtype=F32), nl.pick_even(n), np.zeros(n // 2, F32), 0.1 * np.eye(n // 2, dtype=F32))
    with pytest.raises(bfa.BayesFiltError, match="registry functions above dimension 8"):
        bfa.speedy_augmented_gaussian_sum_filter(user, np.zeros((3, n // 2), F32), (2, 2, 2))
