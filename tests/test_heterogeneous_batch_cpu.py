"""Batches with a covariance of their own per trajectory / component, no GPU: the inputs and references of
tests/test_heterogeneous_batch_gpu.py are validated here, so that the GPU tests can neither pass vacuously (every case must
tell trajectories apart, and must tell the true reference from the one a kernel reading the wrong P_in would produce, by 100
times the asserted tolerance) nor fail because of their own reference (the fp32 oracle must be within a fifth of the asserted
tolerance of float64).  These are conditions on the cases, not measurements: a case that misses one gets another seed."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import common as cm
from tests import heterogeneous_cases as hc


@pytest.mark.parametrize("name", list(hc.CASES))
def test_discrimination(name):
    """Distinct chains' filtered covariances differ by >= 100 tol at t = 0 and t = min(3, T - 1) (the difference decays
    geometrically on these stable models: the early steps are where a slot mix-up shows), and so does the reference with
    every P0 replaced by chain 0's -- the mutation the GPU test must catch."""
    c = hc.CASES[name]
    for t, (pairs, mutation) in hc.discrimination(name).items():
        print(f"{name}: t = {t}: distinct chains differ by >= {pairs:.2e}, same-prior mutation misses by {mutation:.2e} (100 tol = {100 * c['tol']:.0e})")
        cm.record(f"heterogeneous_discrimination[{name}]", t=t, pairs=pairs, mutation=mutation)
        assert pairs >= 100 * c["tol"], (name, t, pairs)
        assert mutation >= 100 * c["tol"], (name, t, mutation)
    # the whole arrays the GPU test compares: the mutation is far outside every asserted tolerance
    ref, mut = hc.reference(name), hc.reference(name, True)
    for k in hc.STREAMS:
        assert cm.rel_err(mut[k], ref[k]) >= 100 * c["tol"], (name, k)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_reference_headroom(name):
    """The fp32 oracle against the float64 recursion on the same inputs: within one fifth of the case's GPU tolerance on
    every stream (weights absolutely, as the GPU test measures them)."""
    c = hc.CASES[name]
    h = hc.headroom(name)
    print(f"{name}: fp32 oracle vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in h.items()))
    cm.record(f"heterogeneous_headroom[{name}]", **h)
    for k in hc.STREAMS + ("carry_means", "carry_covariances"):
        assert h[k] <= c["tol"] / 5, (name, k, h[k])
    assert h["loglik"] <= c["tol_ll"] / 5, (name, h["loglik"])
    assert h["weights"] <= c["tol_w"] / 5, (name, h["weights"])


@pytest.mark.parametrize("name", list(hc.CHUNK_CUTS))
def test_carry_at_the_cut_tells_chains_apart(name):
    """The chunk test is bit for bit, so any difference would do; the cuts are chosen where every pair of chains still differs
    by 100 tolerances, like everywhere else."""
    d = hc.carry_discrimination(name)
    print(f"{name}: carried covariances of distinct chains after step {hc.CHUNK_CUTS[name] - 1} differ by >= {d:.2e}")
    assert 0 < hc.CHUNK_CUTS[name] < hc.CASES[name]["T"]
    assert d >= 100 * hc.CASES[name]["tol"], (name, d)


def test_carry_comparison_is_shortened_on_the_constant_velocity_case_only():
    """carry_T = T everywhere but on kf-cv, and there for the stated reason: after all T steps the fp32 oracle's last
    prediction is more than tol / 5 from float64 on its own scale."""
    assert [n for n, c in hc.CASES.items() if c["carry_T"] != c["T"]] == ["kf-cv"]
    ref, r64 = hc.reference("kf-cv"), hc.reference_f64("kf-cv")
    e = cm.rel_err(ref["predicted_covariances"][:, :, -1], r64["predicted_covariances"][:, :, -1])
    print(f"kf-cv: fp32 oracle vs float64, predicted covariance after the last step, own scale: {e:.2e}")
    assert e > hc.CASES["kf-cv"]["tol"] / 5


@pytest.mark.parametrize("name", list(hc.SMOOTHER_CASES))
def test_smoother_input_headroom(name):
    """A plain fp32 evaluation of the RTS recursion against float64 on each smoother input: within a fifth of the smoother
    test's 1e-5 where the table says so, and NOT on kf-cv, the one input the issue fixes (hc.SMOOTHER_CASES says what follows)."""
    e = hc.smoother_fp32_error(name)
    print(f"{name}: fp32 RTS recursion vs float64, smoothed covariances: {e:.2e}")
    cm.record(f"heterogeneous_smoother_headroom[{name}]", fp32_vs_f64=e)
    if hc.SMOOTHER_CASES[name]:
        assert e <= hc.TOL_SMOOTHER / 5, (name, e)
    else:
        assert e > hc.TOL_SMOOTHER / 5, (name, e)


def test_float64_recursion_is_the_smoother_tests_plus_jitter():
    """hc.kalman_f64 without the + 1e-6 in the gain's solve is tests/test_smoother_cpu.py::kalman_f64 to float64 rounding:
    the jitter is the only difference between the two (and it is what the engine and the oracle compute)."""
    from tests.test_smoother_cpu import kalman_f64
    name = "kf-7-4"
    a = hc.model(name)
    ys, m0s, P0s = hc.data(name)
    with_jitter = hc.reference_f64(name)
    worst = 0.0
    for b in (0, 1, ys.shape[0] - 1):
        r = kalman_f64(a, ys[b].astype(np.float64), m0s[b, 0], P0s[b, 0])
        for k, s in (("m", "means"), ("P", "covariances"), ("pm", "predicted_means"), ("pP", "predicted_covariances")):
            e = cm.rel_err(with_jitter[s][b, 0], r[k])
            worst = max(worst, e)
            assert e < 1e-4, (b, k, e)     # the jitter itself: ~1e-5 relative at R ~ 0.1 (tests/test_oracle_filters.py)
    assert worst > 1e-9                    # ... and it is there


@pytest.mark.parametrize("name", ["kf-3-2", "kf-16-8"])
def test_c_port_with_per_trajectory_covariances(name):
    """c_oracle.kalman_filter(init_covs=) == the NumPy oracle looped per trajectory, at the tolerance
    tests/test_oracle_filters.py::test_c_port_matches_numpy_oracle asserts: the C port is the checker from n = 16."""
    a = hc.model(name)
    ys, m0s, P0s = hc.data(name)
    B = min(ys.shape[0], 6)
    ys, m0s, P0s = ys[:B], m0s[:B, 0], P0s[:B, 0]
    ref = hc.kalman_numpy(a, ys, m0s, P0s)
    got = c_oracle.kalman_filter(a, ys, m0s, init_covs=P0s)
    assert set(got) == set(ref)
    for k in got:
        e = cm.rel_err(got[k], ref[k])
        print(f"{name}: C port vs NumPy oracle, {k}: {e:.2e}")
        assert got[k].shape == ref[k].shape and e < hc.TOL_C_PORT, (k, e)
    # it did read the covariances it was given: with trajectory 0's for all, it is far away
    same = c_oracle.kalman_filter(a, ys, m0s, init_covs=np.broadcast_to(P0s[0], P0s.shape))
    assert cm.rel_err(same["covariances"], ref["covariances"]) > 1e-2


def test_priors_follow_the_recipe():
    a = hc.model("kf-3-2")
    m0s, P0s = hc.priors(a, 4)
    rng = np.random.default_rng(1002)
    L = 0.5 * rng.normal(size=(3, 3))
    assert np.array_equal(P0s[2], (L @ L.T + 0.5 * np.eye(3)).astype(np.float32))
    assert np.array_equal(m0s[2], (a["m0"] + 0.3 * rng.normal(size=3)).astype(np.float32))
    assert np.all(np.linalg.eigvalsh(P0s.astype(np.float64)) >= 0.49)
    ys, im, iP = hc.data("gsf-3-3-K5")
    assert im.shape == (3, 5, 3) and iP.shape == (3, 5, 3, 3) and ys.shape == (3, 10, 3)
    assert not ys.flags.writeable and not hc.reference("gsf-3-3-K5")["covariances"].flags.writeable


def test_first_step_of_a_gaussian_sum_is_the_free_running_reference():
    """hc.gsf_first_step (what the GPU test holds step 0 against) equals step 0 of the chain-wise reference."""
    name = "gsf-3-3-K5"
    ref = hc.reference(name)
    for b in range(hc.CASES[name]["B"]):
        s0 = hc.gsf_first_step(name, b)
        for k in hc.FIELDS + ("loglik",):
            assert np.array_equal(s0[k], ref[k][b, :, 0]), (b, k)
