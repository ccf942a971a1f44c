"""The oracle's per-step log-evidence (dbg["logz"], dbg["logz64"]) and posterior mean (dbg["mean64"]) of the bootstrap
particle filter, pinned WITHOUT the engine -- the reference of tests/test_bpf_routes_gpu.py must be right before it judges a
kernel.  logz_t = log sum_i w_{t-1,i} p(y_t | x_{t,i}); its additive constant -m/2 log 2 pi - 1/2 log det R_lp cancels in
the normalised weights, so no weight comparison can see it (test 3)."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go, models as om, threefry as otf
from tests import common as cm
from tests import particle_route_cases as prc

F32 = np.float32


def _model(n, m, dq, dr, seed, scale_rlp=1.0):
    """Linear-Gaussian, full Q / R / P0, non-square noise maps, biases; the density's covariance is D R D^T (times `scale_rlp`)."""
    a = cm.random_stable_lgssm(n, m, seed=seed, dq=dq, dr=dr, bias=True)
    a["Rlp"] = (scale_rlp * (a["D"] @ a["R"] @ a["D"].T)).astype(F32)
    fo, ho = om.Linear(a["A"], a["G"]), om.Linear(a["H"], a["D"])
    po = go.ParamsBPF(a["m0"], a["P0"], fo, a["q0"], a["Q"], ho, a["r0"], a["R"], go.GaussianEmissionLogProb(ho, a["Rlp"], a["r0"]))
    return a, po


# The fp32 gap |logz - logz_f64| / (1 + |logz_f64|), logz_f64 the inverse / log-determinant formula on the oracle's own particles:
# measured 1.0e-7, 1.1e-7, 9.5e-8, 3.2e-7 for the canonical oracle on the four shapes below, 1.2e-7 and 5.7e-7 for the libm loop.
# The bound: the dominant particles' fp32 log-densities carry ~m (m + 1) / 2 + 3 roundings of |ll| eps each (forward substitution,
# quadratic form, constant), |ll| up to a few |logz| once the unresampled weights have collapsed, and mx + log(tot) adds two
# roundings of |logz|: some 30 eps = 2e-6 relative.  That is 3e5 times below the m log 2 by which a wrong constant moves logz.
FP32_GAP = 2e-6


# (the libm loop goes particle by particle: the two small shapes cover it)
@pytest.mark.parametrize("dims,N,T,arith", [((4, 2, 2, 2), 300, 20, "canonical"), ((3, 3, 3, 3), 1000, 12, "canonical"),
                                            ((6, 3, 6, 3), 4100, 6, "canonical"), ((2, 2, 2, 2), 50, 30, "canonical"),
                                            ((4, 2, 2, 2), 300, 20, "libm"), ((2, 2, 2, 2), 50, 30, "libm")])
def test_oracle_logz_equals_an_independent_float64_formula(dims, N, T, arith):
    n, m, dq, dr = dims
    a, po = _model(n, m, dq, dr, seed=3)
    ys = cm.simulate_batch(a, 1, T, seed=9)[0]
    ref, dbg = go.bootstrap_particle_filter(po, ys, N, key=otf.PRNGKey(21), ess_threshold=0.0, debug=True, arith=arith)
    assert not dbg["resampled"].any()
    x, w = ref["particles"], ref["weights"]
    lz, wn, mean = prc.recompute_f64(a, x, w, ys)
    # logz64 takes the oracle's fp32 log-densities: against the float64 density of the same particles it differs by their rounding
    # only, and given the SAME log-densities it is the float64 log-sum-exp to 1e-12
    for t in range(T):
        wprev = (np.full(N, F32(1.0) / F32(N)) if t == 0 else w[:, t - 1]).astype(np.float64)      # (the oracle's fp32 1 / N)
        ll32 = np.array(po.emission_distribution_log_prob.logprob_c(x[:, t], ys[t], None) if arith == "canonical" else
                        [po.emission_distribution_log_prob(x[i, t], ys[t], None) for i in range(N)], dtype=np.float64)
        direct = np.log(np.sum(wprev * np.exp(ll32 - ll32.max()))) + ll32.max()
        assert abs(dbg["logz64"][t] - direct) <= 1e-12 * (1 + abs(direct)), t
    assert prc.logz_gap(dbg["logz64"], lz) < FP32_GAP
    gap = prc.logz_gap(dbg["logz"], lz)
    print(f"logz fp32 gap {dims} N={N} T={T} {arith}: {gap:.2e}")
    assert gap < FP32_GAP
    assert dbg["logz"].dtype == F32 and dbg["logz"].shape == (T,) and dbg["logz64"].shape == (T,) and dbg["mean64"].shape == (T, n)
    # mean64 is the weighted mean of what is emitted, and the weights are the float64 ones to the teacher-forced bound
    assert np.max(np.abs(dbg["mean64"] - mean)) <= 1e-12 * np.max(np.abs(mean))
    assert np.max(np.abs(wn - w)) < 2e-5 * max(1.0, w.max() * N) / N + 1e-7


def test_mean64_is_taken_after_resampling():
    a, po = _model(4, 2, 2, 2, seed=3)
    ys = cm.simulate_batch(a, 1, 20, seed=9)[0]
    ref, dbg = go.bootstrap_particle_filter(po, ys, 300, key=otf.PRNGKey(21), debug=True, arith="canonical")
    assert dbg["resampled"].any() and not dbg["resampled"].all()
    mean = np.einsum("itd,it->td", ref["particles"].astype(np.float64), ref["weights"].astype(np.float64))
    assert np.max(np.abs(dbg["mean64"] - mean)) <= 1e-12 * np.max(np.abs(mean))


def _kalman_loglik(a, ys):
    """Exact log p(y_{1:T}) of the model the particle filter sees: biases as a constant extra state, the filter's first step a
    prediction from (m0, P0) (the particle filter propagates before it weights)."""
    n = a["A"].shape[0]
    A = np.zeros((n + 1, n + 1))
    A[:n, :n], A[:n, n], A[n, n] = a["A"], a["G"].astype(np.float64) @ a["q0"], 1.0
    H = np.concatenate([a["H"].astype(np.float64), (a["D"].astype(np.float64) @ a["r0"])[:, None]], axis=1)
    GQGt = np.zeros((n + 1, n + 1))
    GQGt[:n, :n] = a["G"].astype(np.float64) @ a["Q"] @ a["G"].T
    m0 = A @ np.concatenate([a["m0"], [1.0]])
    P0 = np.zeros((n + 1, n + 1))
    P0[:n, :n] = a["P0"]
    P0 = A @ P0 @ A.T + GQGt
    return go.textbook_kalman_f64(A, GQGt, H, a["Rlp"], m0, P0, ys.astype(np.float64))[4].sum()


def test_summed_logz_estimates_the_kalman_log_likelihood():
    """sum_t logz64_t is the log of the particle filter's unbiased likelihood estimate: over K = 16 fixed keys its mean sits
    within 4 s / sqrt(K) (Monte-Carlo error) + s^2 / 2 (the bias of a log of an unbiased estimate, second order) of the exact
    answer, s the spread over the keys -- a bound from the reference's own spread, no number by hand."""
    K, N, T = 16, 2000, 20
    a, po = _model(4, 2, 2, 2, seed=3)
    ys = cm.simulate_batch(a, 1, T, seed=9)[0]
    exact = _kalman_loglik(a, ys)
    est = np.array([go.bootstrap_particle_filter(po, ys, N, key=otf.PRNGKey(100 + k), debug=True, arith="canonical")[1]["logz64"].sum()
                    for k in range(K)])
    s = est.std(ddof=1)
    print(f"exact {exact:.4f} mean {est.mean():.4f} s {s:.4f} bound {4 * s / np.sqrt(K) + s * s / 2:.4f}")
    assert 0 < s < 1.0                  # (a spread of order one would make the bound empty)
    assert abs(est.mean() - exact) <= 4 * s / np.sqrt(K) + s * s / 2


def test_the_density_constant_shows_in_logz_and_not_in_the_weights():
    """Why the weight tests cannot see the density's constant, and that logz does.  On the particles of step 0 (same key; the
    density does not enter the propagation): the float64 weights with and without the constant are the same numbers and the
    oracle's are those; a run whose density has the covariance 4 R_lp has the logz of THAT density -- quadratic form divided by
    4, constant moved by -m log 2 -- and a density that kept the old constant would sit m log 2 = 1.39 away."""
    N, T, m = 300, 4, 2
    a, po = _model(4, m, 2, 2, seed=3)
    a4, po4 = _model(4, m, 2, 2, seed=3, scale_rlp=4.0)
    ys = cm.simulate_batch(a, 1, T, seed=9)[0]
    key = otf.PRNGKey(21)
    ref, dbg = go.bootstrap_particle_filter(po, ys, N, key=key, ess_threshold=0.0, debug=True, arith="canonical")
    ref4, dbg4 = go.bootstrap_particle_filter(po4, ys, N, key=key, ess_threshold=0.0, debug=True, arith="canonical")
    x0 = ref["particles"][:, 0]
    assert np.array_equal(ref4["particles"][:, 0], x0)
    ll = prc.log_density_f64(a, x0, ys[0])
    const = -0.5 * (np.linalg.slogdet(a["Rlp"].astype(np.float64))[1] + m * np.log(2 * np.pi))
    quad = ll - const
    w_with = np.exp(ll - ll.max())
    w_with /= w_with.sum()
    w_without = np.exp(quad - quad.max())
    w_without /= w_without.sum()
    assert np.max(np.abs(w_with - w_without)) < 1e-15                       # the constant cancels in the weights ...
    w0 = ref["weights"][:, 0]
    assert np.max(np.abs(w_with - w0)) < 2e-5 * max(1.0, w0.max() * N) / N + 1e-7
    want = np.log(np.mean(np.exp(quad / 4))) + const - m * np.log(2.0)      # ... and is all of logz's offset
    assert abs(dbg4["logz64"][0] - want) < FP32_GAP * (1 + abs(want))
    assert abs(float(dbg4["logz"][0]) - want) < FP32_GAP * (1 + abs(want))
    assert abs((dbg4["logz64"][0] + m * np.log(2.0)) - want) > 1.0
    # the step-0 weights of the two runs differ only by the tempering of the quadratic form, not by any constant
    w4 = np.exp(quad / 4 - (quad / 4).max())
    w4 /= w4.sum()
    assert np.max(np.abs(w4 - ref4["weights"][:, 0])) < 2e-5 * max(1.0, ref4["weights"][:, 0].max() * N) / N + 1e-7



def test_ambiguous_draws_flags_positions_inside_cdf_inversions():
    """dbg["ambiguous"]: the positions of a resampling step for which {i: c_i < r} is not a prefix of the (non-monotone) fp32
    CDF -- only there can two bisections disagree.  draw_positions reproduces the run's own lookups."""
    cdf = np.array([0.1, 0.3, 0.29999998, 0.5, 0.5, 1.0], F32)
    r = np.array([0.05, 0.29999998, 0.3, 0.31, 0.5, 1.0], F32)     # (0.3: c_1 reaches it, the later c_2 is below it again)
    assert go.ambiguous_draws(cdf, r).tolist() == [False, False, True, False, False, False]
    a, po = _model(4, 2, 2, 2, seed=3)
    ys = cm.simulate_batch(a, 1, 20, seed=9)[0]
    for resampler in ("multinomial", "systematic"):
        ref, dbg = go.bootstrap_particle_filter(po, ys, 300, key=otf.PRNGKey(21), resampler=resampler, debug=True, arith="canonical")
        assert dbg["resampled"].any() and dbg["ambiguous"].shape == (20, 300) and not dbg["ambiguous"][~dbg["resampled"]].any()
    # the lookups of the first resampling step, rebuilt from the run's key chain (split per step, :1342)
    N, key = 300, otf.PRNGKey(21)
    next_key = otf.split(key, N + 1)[0]
    for t in range(20):
        next_key = otf.split(next_key, N + 1)[0]
        if dbg["resampled"][t]:
            cdf, r = go.draw_positions(dbg["pre_weights"][t], next_key, "systematic")
            assert np.array_equal(np.minimum(np.searchsorted(cdf, r, side="left"), N - 1), dbg["ancestors"][t])
            break
