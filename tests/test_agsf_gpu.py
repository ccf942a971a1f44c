"""GPU parity of the "speedy" augmented Gaussian-sum filter (bf_agsf_ekf_f32; gaussfiltax/inference.py:
621-812) against the NumPy oracle: bit-exact leaf indices of the per-step jr.choice draw, means and
covariances within 2e-5 relative."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import common as cm

pytestmark = pytest.mark.gpu
F32 = np.float32


def _nl():
    import bayesianfiltering_amd as bfa
    return bfa, bfa.nonlinearities


def _compare(post, aux, ref, ref_idx, tol=2e-5):
    got_idx = aux["leaf_indices"].cpu().numpy()
    assert np.array_equal(got_idx, ref_idx), "resampled leaves differ"
    for k in ("means", "covariances"):
        assert cm.rel_err(getattr(post, k).cpu().numpy(), getattr(ref, k)) < tol, (k, cm.rel_err(getattr(post, k).cpu().numpy(), getattr(ref, k)))
    assert np.allclose(post.weights.cpu().numpy(), ref.weights)
    assert post.predicted_means is None and post.predicted_covariances is None


def _oracle_leaf_indices(aux_pre, N0):
    return np.stack([np.minimum(otf.choice_indices(otf.cumsum_assoc(w), otf.uniform(otf.PRNGKey(0), N0)), w.size - 1)
                     for w in aux_pre]).astype(np.int32)


@pytest.mark.parametrize("nc", [(2, 2, 2), (3, 2, 2), (4, 4, 4), (5, 1, 3)])
def test_linear_model(nc):
    bfa, nl = _nl()
    a = cm.cv_model_arrays()
    po, pp = cm.oracle_params(a), cm.product_params(a)
    T = 25
    ys = go.sample_ssm(po, otf.PRNGKey(1), T)[1]
    init = np.random.default_rng(0).normal(size=(nc[0], 4)).astype(F32)
    ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys, nc, initial_means=init, debug=True)
    post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, initial_means=init, return_leaf_indices=True)
    assert tuple(post.means.shape) == (nc[0], T, 4) and tuple(post.covariances.shape) == (nc[0], T, 4, 4)
    _compare(post, aux, ref, _oracle_leaf_indices(raux["pre_weights"], nc[0]))


def test_bearings_only_batch_keys_and_chunks():
    """Manoeuvring target with inputs, a batch of trajectories, a non-default rng_key and opt_args;
    two chunks through the carry reproduce the single scan."""
    bfa, nl = _nl()
    T, B, nc = 24, 5, (3, 2, 2)
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    S0 = np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)
    inputs = np.array([1] * 8 + [0] * 8 + [2] * 8, F32)
    po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Q, om.BearingRange(), np.zeros(2, F32), R)
    pp = bfa.ParamsNLSSM(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Q, nl.bearing_range(), np.zeros(2, F32), R)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(10 + b), T, inputs.reshape(T, 1))[1] for b in range(B)])
    init = (mu0 + 0.05 * np.random.default_rng(0).normal(size=(B, nc[0], 4))).astype(F32)
    key = otf.PRNGKey(7)
    post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, key, 1, (0.2, 0.3), inputs, initial_means=init,
                                                         return_leaf_indices=True)
    assert tuple(post.means.shape) == (B, nc[0], T, 4)
    for b in range(B):
        ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys[b], nc, key, 1, (0.2, 0.3), inputs.reshape(T, 1),
                                                            initial_means=init[b], debug=True)
        idx = _oracle_leaf_indices(raux["pre_weights"], nc[0])
        assert np.array_equal(aux["leaf_indices"][b].cpu().numpy(), idx), b
        for k in ("means", "covariances"):
            assert cm.rel_err(getattr(post, k)[b].cpu().numpy(), getattr(ref, k)) < 2e-5, (b, k)
    p1, a1 = bfa.speedy_augmented_gaussian_sum_filter(pp, ys[:, :10], nc, key, 1, (0.2, 0.3), inputs[:10], initial_means=init,
                                                      return_carry=True)
    p2, _ = bfa.speedy_augmented_gaussian_sum_filter(pp, ys[:, 10:], nc, key, 1, (0.2, 0.3), inputs[10:], carry=a1["carry"])
    for k in ("means", "covariances", "weights"):
        cat = np.concatenate([getattr(p1, k).cpu().numpy(), getattr(p2, k).cpu().numpy()], axis=2)
        assert np.array_equal(cat, getattr(post, k).cpu().numpy()), k


def test_lorenz96_and_errors():
    bfa, nl = _nl()
    T, nc = 10, (2, 2, 2)
    po = go.ParamsNLSSM(np.zeros(8, F32), np.eye(8, dtype=F32), om.Lorenz96(8), np.zeros(8, F32),
                        1e-2 * np.eye(8, dtype=F32), om.PickEven(8), np.zeros(4, F32), 1e-1 * np.eye(4, dtype=F32))
    pp = bfa.ParamsNLSSM(np.zeros(8, F32), np.eye(8, dtype=F32), nl.lorenz96(8), np.zeros(8, F32),
                         1e-2 * np.eye(8, dtype=F32), nl.pick_even(8), np.zeros(4, F32), 1e-1 * np.eye(4, dtype=F32))
    ys = go.sample_ssm(po, otf.PRNGKey(2), T)[1]
    init = np.random.default_rng(1).normal(size=(2, 8)).astype(F32)
    ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys, nc, initial_means=init, debug=True)
    post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, initial_means=init, return_leaf_indices=True)
    _compare(post, aux, ref, _oracle_leaf_indices(raux["pre_weights"], 2))
    with pytest.raises(bfa.BayesFiltError):     # more leaves than one wave
        bfa.speedy_augmented_gaussian_sum_filter(pp, ys, (5, 5, 5))
    with pytest.raises(ValueError):
        bfa.speedy_augmented_gaussian_sum_filter(pp, ys, (2, 2))


def test_golden_bearings_only_fixture(golden_dir):
    bfa, nl = _nl()
    d = np.load(f"{golden_dir}/agsf_bot_322_T24.npz")
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    pp = bfa.ParamsNLSSM(mu0, np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32), nl.maneuver_bot(), np.zeros(2, F32),
                         1e-3 * np.eye(2, dtype=F32), nl.bearing_range(), np.zeros(2, F32), np.diag([1e-3, 1e-2]).astype(F32))
    post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, d["emissions"], (3, 2, 2), d["key"], 1, tuple(d["opt_args"]),
                                                         d["inputs"], initial_means=d["initial_means"], return_leaf_indices=True)
    assert np.array_equal(aux["leaf_indices"].cpu().numpy(), _oracle_leaf_indices(d["pre_weights"], 3))
    for k in ("means", "covariances"):
        assert cm.rel_err(getattr(post, k).cpu().numpy(), d[k]) < 2e-5, k


@pytest.mark.parametrize("nc", [(2, 5, 5), (3, 2, 2)])
def test_container_branch_variant(nc):
    """augmented_gaussian_sum_filter (inference.py:458-620): per-node keys and jr.multivariate_normal draws
    (containers.py:63-140); (2, 5, 5) is the reference's own test size (docs/tests/test_inference.py:85)."""
    bfa, nl = _nl()
    a = cm.cv_model_arrays()
    po, pp = cm.oracle_params(a), cm.product_params(a)
    T = 20
    ys = go.sample_ssm(po, otf.PRNGKey(3), T)[1]
    init = np.random.default_rng(1).normal(size=(nc[0], 4)).astype(F32)
    key = otf.PRNGKey(11)
    ref, raux = go.augmented_gaussian_sum_filter(po, ys, nc, key, initial_means=init, debug=True)
    post, aux = bfa.augmented_gaussian_sum_filter(pp, ys, nc, key, initial_means=init, return_leaf_indices=True)
    _compare(post, aux, ref, _oracle_leaf_indices(raux["pre_weights"], nc[0]))
    # and it is a different stream from the speedy variant
    sp, _ = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, key, initial_means=init)
    assert not np.allclose(sp.means.cpu().numpy(), post.means.cpu().numpy())


@pytest.mark.parametrize("which", ["speedy_unscented_agsf", "unscented_agsf"])
def test_unscented_nodes(which):
    """speedy_unscented_agsf (inference.py:966-1156) and unscented_agsf (:813-965): the same trees with
    _ukf_predict_nonadditive / _ukf_condition_on_nonadditive at the nodes, on the manoeuvring-target model."""
    bfa, nl = _nl()
    T, nc = 18, (2, 5, 5)
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    S0 = np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)
    inputs = np.array([1] * 6 + [0] * 6 + [2] * 6, F32)
    po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Q, om.BearingRange(), np.zeros(2, F32), R)
    pp = bfa.ParamsNLSSM(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Q, nl.bearing_range(), np.zeros(2, F32), R)
    ys = go.sample_ssm(po, otf.PRNGKey(4), T, inputs.reshape(T, 1))[1]
    init = (mu0 + 0.05 * np.random.default_rng(2).normal(size=(nc[0], 4))).astype(F32)
    ref, raux = getattr(go, which)(po, go.ParamsUKF(1, 0, 0), ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs.reshape(T, 1),
                                   initial_means=init, debug=True)
    post, aux = getattr(bfa, which)(pp, bfa.ParamsUKF(1, 0, 0), ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs,
                                    initial_means=init, return_leaf_indices=True)
    _compare(post, aux, ref, _oracle_leaf_indices(raux["pre_weights"], nc[0]), tol=3e-5)


@pytest.mark.parametrize("M,N", [(8, 3), (12, 4), (50, 2), (30, 5), (64, 8), (5, 5), (7, 1),
                                 (65, 64), (125, 5), (100, 10), (256, 3), (257, 17), (1000, 20), (1024, 1024)])
def test_optimal_resampling_matches_oracle(M, N):
    """utils.optimal_resampling (utils.py:216-244) on the device: indices bit-exact, weights to fp32 rounding,
    for flat, peaked and tied weight vectors.  More than 64 weights: one workgroup per vector (sort exchanges,
    running sums and look-ups through LDS)."""
    bfa, nl = _nl()
    rng = np.random.default_rng(M * 100 + N)
    ws = [rng.dirichlet(np.ones(M)), rng.dirichlet(0.05 * np.ones(M)), np.ones(M) / M,
          np.r_[np.zeros(M - 2), [0.5, 0.5]] if M > 2 else np.ones(M) / M]
    W = np.stack(ws).astype(F32)
    key = otf.PRNGKey(M + N)
    idx, wo = bfa.optimal_resampling(W, N, key)
    for b in range(W.shape[0]):
        ri, rw = go.optimal_resampling(W[b], N, key)
        assert np.array_equal(idx[b].cpu().numpy(), ri), (b, idx[b].cpu().numpy(), ri)
        assert np.allclose(wo[b].cpu().numpy(), rw, rtol=1e-6, atol=1e-7, equal_nan=True), b
    i1, w1 = bfa.optimal_resampling(W[0], N, key)
    assert tuple(i1.shape) == (N,) and np.array_equal(i1.cpu().numpy(), idx[0].cpu().numpy())


@pytest.mark.parametrize("nc", [(2, 5, 5), (4, 2, 3), (5, 5, 5), (3, 10, 10)])
def test_optimal_variant(nc):
    """augmented_gaussian_sum_filter_optimal (inference.py:1157-1300): unequal carried weights.  [5, 5, 5] is the tree
    of the reference's own test (docs/tests/test_inference.py:89-92): 125 leaves, one 256-thread workgroup per
    trajectory; [3, 10, 10] needs 1024 threads."""
    bfa, nl = _nl()
    a = cm.cv_model_arrays()
    po, pp = cm.oracle_params(a), cm.product_params(a)
    T = 20
    ys = go.sample_ssm(po, otf.PRNGKey(5), T)[1]
    init = np.random.default_rng(4).normal(size=(nc[0], 4)).astype(F32)
    key = otf.PRNGKey(13)
    ref, raux = go.augmented_gaussian_sum_filter_optimal(po, ys, nc, key, initial_means=init, debug=True)
    post, aux = bfa.augmented_gaussian_sum_filter_optimal(pp, ys, nc, key, initial_means=init, return_leaf_indices=True,
                                                          return_carry=True)
    assert np.array_equal(aux["leaf_indices"].cpu().numpy(), raux["leaf_indices"])
    for k in ("means", "covariances"):
        assert cm.rel_err(getattr(post, k).cpu().numpy(), getattr(ref, k)) < 2e-5, k
    # the weights are exponentials of log-likelihood differences: a 1e-5 error in ll is a 1e-5 * |ll| error here
    assert np.allclose(post.weights.cpu().numpy(), ref.weights, rtol=3e-4, atol=1e-7)
    assert not np.allclose(ref.weights, 1.0 / nc[0])                    # the point of the variant
    assert np.allclose(aux["carry"].weights.cpu().numpy()[0], ref.weights[:, -1], rtol=3e-4, atol=1e-7)


@pytest.mark.parametrize("nc,unscented", [((100, 2, 2), False), ((3, 5, 7), False), ((20, 3, 3), True), ((70, 1, 1), False),
                                          ((100, 2, 2), True), ((130, 2, 3), False)])
def test_trees_wider_than_a_wave(nc, unscented):
    """num_components = [100, 2, 2] is what BOT_Experiment_script.py:118 runs: 400 leaves = one 512-thread workgroup
    per trajectory (reductions and the cumulative sum continue across waves); 70 and 105 leaves use 128 threads, 180 leaves 256, 780 leaves 1024."""
    bfa, nl = _nl()
    T, B = 8, 2
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    S0 = np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)
    inputs = np.array([1] * 3 + [0] * 3 + [2] * 2, F32)
    po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Q, om.BearingRange(), np.zeros(2, F32), R)
    pp = bfa.ParamsNLSSM(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Q, nl.bearing_range(), np.zeros(2, F32), R)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(20 + b), T, inputs.reshape(T, 1))[1] for b in range(B)])
    init = (mu0 + 0.05 * np.random.default_rng(7).normal(size=(B, nc[0], 4))).astype(F32)
    key = otf.PRNGKey(9)
    if unscented:
        post, aux = bfa.speedy_unscented_agsf(pp, bfa.ParamsUKF(1, 0, 0), ys, nc, key, 1, (0.1, 0.1), inputs, initial_means=init,
                                              return_leaf_indices=True)
    else:
        post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, key, 1, (0.1, 0.1), inputs, initial_means=init,
                                                             return_leaf_indices=True)
    assert tuple(post.means.shape) == (B, nc[0], T, 4)
    for b in range(B):
        if unscented:
            ref, raux = go.speedy_unscented_agsf(po, go.ParamsUKF(1, 0, 0), ys[b], nc, key, 1, (0.1, 0.1), inputs.reshape(T, 1),
                                                 initial_means=init[b], debug=True)
        else:
            ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys[b], nc, key, 1, (0.1, 0.1), inputs.reshape(T, 1),
                                                                initial_means=init[b], debug=True)
        assert np.array_equal(aux["leaf_indices"][b].cpu().numpy(), raux["leaf_indices"]), b
        for k in ("means", "covariances"):
            assert cm.rel_err(getattr(post, k)[b].cpu().numpy(), getattr(ref, k)) < 3e-5, (b, k)


@pytest.mark.parametrize("nodes", ["extended", "unscented"])
def test_time_varying_covariances(nodes):
    """(T, d, d) noise covariances in the augmented filters (inference.py:658-661, :1004-1007): per-step Q_t / R_t at
    every node of the tree, extended-Kalman and unscented nodes; the drawn leaves stay bit-exact."""
    bfa, nl = _nl()
    rng = np.random.default_rng(9)
    T, nc = 20, (3, 2, 3)
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    S0 = np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)

    def table(base):
        out = []
        for t in range(T):
            w = rng.normal(size=base.shape) * 0.3
            out.append(base * (0.5 + rng.uniform()) + 0.2 * np.mean(np.diag(base)) * (w @ w.T))
        return np.stack(out).astype(F32)

    Qt, Rt = table(Q), table(R)
    inputs = np.array([1] * 7 + [0] * 6 + [2] * 7, F32)
    po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Qt, om.BearingRange(), np.zeros(2, F32), Rt)
    pp = bfa.ParamsNLSSM(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Qt, nl.bearing_range(), np.zeros(2, F32), Rt)
    ys = go.sample_ssm(po._replace(dynamics_noise_covariance=Q, emission_noise_covariance=R), otf.PRNGKey(4), T,
                       inputs.reshape(T, 1))[1]
    init = (mu0 + 0.05 * rng.normal(size=(nc[0], 4))).astype(F32)
    if nodes == "extended":
        ref, raux = go.speedy_augmented_gaussian_sum_filter(po, ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs.reshape(T, 1),
                                                            initial_means=init, debug=True)
        post, aux = bfa.speedy_augmented_gaussian_sum_filter(pp, ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs,
                                                             initial_means=init, return_leaf_indices=True)
        const, _ = bfa.speedy_augmented_gaussian_sum_filter(pp._replace(dynamics_noise_covariance=Q, emission_noise_covariance=R),
                                                            ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs, initial_means=init,
                                                            return_leaf_indices=True)
    else:
        ref, raux = go.speedy_unscented_agsf(po, go.ParamsUKF(1, 0, 0), ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs.reshape(T, 1),
                                             initial_means=init, debug=True)
        post, aux = bfa.speedy_unscented_agsf(pp, bfa.ParamsUKF(1, 0, 0), ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs,
                                              initial_means=init, return_leaf_indices=True)
        const, _ = bfa.speedy_unscented_agsf(pp._replace(dynamics_noise_covariance=Q, emission_noise_covariance=R),
                                             bfa.ParamsUKF(1, 0, 0), ys, nc, otf.PRNGKey(3), 1, (0.1, 0.1), inputs,
                                             initial_means=init, return_leaf_indices=True)
    _compare(post, aux, ref, _oracle_leaf_indices(raux["pre_weights"], nc[0]), tol=3e-5)
    assert cm.rel_err(const.covariances.cpu().numpy(), ref.covariances) > 1e-3  # the tables are not ignored
    with pytest.raises(bfa.BayesFiltError):  # one matrix per step
        bfa.speedy_augmented_gaussian_sum_filter(pp._replace(dynamics_noise_covariance=Qt[:5]), ys, nc, otf.PRNGKey(3), 1,
                                                 (0.1, 0.1), inputs, initial_means=init)
