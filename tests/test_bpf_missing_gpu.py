"""The bootstrap particle filter with missing observations (``missing="nan"`` / ``observed=``, bf_bpf_missing_f32) on EVERY
kernel route of tests/particle_route_cases.py, on the gap pattern of tests/particle_missing_cases.py (partial gaps at steps 1
and 4, a wholly missing step 2, a forecast step at the end of the last trajectory):

  1. bits of the masked oracle (the existing oracle's own log-density on the compacted problem) at the default ESS threshold:
     resampling decisions, ancestors, weights, particles, ESS, logz; mean to 1e-5 of the oracle's float64 mean;
  2. with nothing missing the new route is the plain route, bit for bit, in every stream and in the carry;
  3. float64, teacher-forced (ess_threshold = 0), canonical and hardware-arithmetic rows, against the masked recompute_f64;
  4. the stochastic-volatility density (scale of the observed rows only) with single, double and whole gaps;
  5. functions from source: a Gaussian density around a source emission against its registry twin, a density from source that
     treats NaN per component against float64, one that does not (poisoned by its first partial gap, not by a whole one);
  6. the contract: ``observed=`` in its four shapes, chunks cut inside the gap, summary == both, +-Inf poisons, the plain
     route still poisons on NaN, the posterior-sample wrapper.

Bounds.  logz against float64: canonical rows 10 x the worst gap of the masked fp32 ORACLE against float64 measured on the CPU on
these rows and this pattern (particle_missing_cases.ORACLE_LOGZ_GAP, 4.7e-8 ... 2.1e-7 -> 2.1e-6); hardware arithmetic the
standing 2e-5; mean 1e-5."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import particle_missing_cases as pmc
from tests import particle_route_cases as prc

pytestmark = pytest.mark.gpu
F32 = np.float32
SUMMARY = ("mean", "ess", "logz", "resampled")


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def _same(x, y):
    return _bits_equal(x, y) if x.dtype == F32 else np.array_equal(x, y)


def _run(case, pp, ys, ess_threshold=0.5, output="both", carry=None, return_carry=False, keyed=True, missing="nan", inputs=None, **kw):
    """One call on the row's route (per-call options; bpf_spec set and restored around it), NumPy arrays back."""
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import _lib
    lib = _lib.require_gpu()
    if case.spec is not None:
        _lib.check(lib.bf_set_option(b"bpf_spec", case.spec))
    try:
        got = bfa.bootstrap_particle_filter(pp, ys, case.N, prc.key_of(case) if keyed else None, inputs, ess_threshold,
                                            resampler=case.resampler, output=output, carry=carry, return_carry=return_carry,
                                            return_ancestors=output != "summary", options=case.options, missing=missing, **kw)
    finally:
        if case.spec is not None:
            _lib.check(lib.bf_set_option(b"bpf_spec", 1))
    out, c = got if return_carry else (got, None)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return (out, c) if return_carry else out


def _setup(case):
    a = prc.arrays(case)
    ys = prc.observations(case, a)
    return a, prc.engine_params(case, a), ys, pmc.gapped(ys)


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_route_gives_the_masked_oracles_bits(case):
    a, pp, _, ys = _setup(case)
    out = _run(case, pp, ys, output=case.output)
    for b in prc.oracle_trajectories(case):
        ref, dbg = pmc.oracle_run(case, b)
        assert np.array_equal(out["resampled"][b] > 0.5, dbg["resampled"]), (b, out["resampled"][b], dbg["resampled"])
        if case.output == "both":
            assert np.array_equal(out["ancestors"][b].T, dbg["ancestors"]), b
            assert _bits_equal(out["weights"][b], ref["weights"]), b
            assert _bits_equal(out["particles"][b], ref["particles"]), b
        assert _bits_equal(out["ess"][b], dbg["ess"]), (b, out["ess"][b], dbg["ess"])
        err = cm.rel_err(out["mean"][b], dbg["mean64"])
        print(f"{case.id} b={b}: logz {out['logz'][b]} mean rel_err {err:.2e}")
        assert _bits_equal(out["logz"][b], dbg["logz"]), (b, out["logz"][b], dbg["logz"])
        assert err <= prc.MEAN_BOUND, (b, err)


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_nothing_missing_is_the_plain_route_bit_for_bit(case):
    a, pp, ys, _ = _setup(case)
    plain, cp = _run(case, pp, ys, output=case.output, return_carry=True, missing=None)
    new, cn = _run(case, pp, ys, output=case.output, return_carry=True)
    assert set(plain) == set(new)
    for k in plain:
        assert _same(plain[k], new[k]), k
    assert _bits_equal(cp.weights.cpu().numpy(), cn.weights.cpu().numpy())
    assert _bits_equal(cp.particles.cpu().numpy(), cn.particles.cpu().numpy())
    assert np.array_equal(np.asarray(cp.key), np.asarray(cn.key))
    assert np.isfinite(plain["logz"]).all() and plain["resampled"].any()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def _against_float64(case):
    a, pp, _, ys = _setup(case)
    out = _run(case, pp, ys, ess_threshold=0.0, output="both")
    assert not out["resampled"].any()
    bound = pmc.LOGZ_BOUND_HARDWARE if case.arith else pmc.LOGZ_BOUND_CANONICAL
    checks = []
    for b in prc.oracle_trajectories(case):
        x, w = out["particles"][b], out["weights"][b]
        assert np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(out["logz"][b]).all(), b
        lz, wn, mean = pmc.recompute_f64(a, x, w, ys[b])
        gz, gm = prc.logz_gap(out["logz"][b], lz), cm.rel_err(out["mean"][b], mean)
        print(f"{case.id} b={b}: logz gap {gz:.2e} (bound {bound:.1e}), mean rel_err {gm:.2e}")
        checks.append((b, gz, gm))
    cm.record(f"bpf_missing_float64[{case.id}]", logz_gap=max(c[1] for c in checks), mean_rel_err=max(c[2] for c in checks))
    for b, gz, gm in checks:
        assert gz <= bound, (case.id, b, gz)
        assert gm <= pmc.MEAN_BOUND_F64, (case.id, b, gm)


@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_route_against_float64_from_its_own_particles(case):
    _against_float64(case)


def test_hardware_arithmetic_routes_against_float64_from_their_own_particles():
    for case in prc.HARDWARE:
        _against_float64(case)


# ---- 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 300])
def test_stochastic_volatility_with_gaps(N):
    import bayesianfiltering_amd as bfa
    po, arr, ys, u, key = pmc.sv_setup()
    pp = pmc.sv_engine_params(arr)
    ref, dbg = go.bootstrap_particle_filter(po, ys, N, key=key, inputs=u.reshape(-1, 1), debug=True, arith="canonical")
    assert tuple(np.flatnonzero(dbg["resampled"])) == pmc.SV_RESAMPLES[N] and not dbg["ambiguous"].any()
    out = bfa.bootstrap_particle_filter(pp, ys, N, key, u, output="both", return_ancestors=True, missing="nan")
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(out["resampled"] > 0.5, dbg["resampled"]), (out["resampled"], dbg["resampled"])
    assert np.array_equal(out["ancestors"].T, dbg["ancestors"])
    assert _bits_equal(out["particles"], ref["particles"]) and _bits_equal(out["weights"], ref["weights"])
    assert _bits_equal(out["ess"], dbg["ess"]) and _bits_equal(out["logz"], dbg["logz"]), (out["logz"], dbg["logz"])


# ---- 5 -------------------------------------------------------------------------------------------------------------------
BOT_EMI_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  out[0] = atan2(x[2], x[0]) + r[0];
  out[1] = sqrt(x[0] * x[0] + x[2] * x[2]) + r[1];
}
"""


def test_gaussian_density_around_a_source_emission_is_its_registry_twin():
    """The bearing-range emission as source (the run-time build) against the registry function (the compiled (4, 2, 2) instance),
    full R, on a series with single and whole gaps: every stream bit for bit."""
    import bayesianfiltering_amd as bfa
    from oracle import models as om, threefry as otf
    nl = bfa.nonlinearities
    T, B, N = 12, 2, 500
    mu0 = np.array([2.0, 0.3, 3.0, -0.2], F32)
    S0 = np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.array([[1e-3, 2e-4], [2e-4, 1e-2]], F32)
    r0 = np.array([0.01, -0.02], F32)
    inputs = np.array([1] * 4 + [0] * 4 + [2] * 4, F32)
    po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Q, om.BearingRange(), r0, R)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(10 + b), T, inputs.reshape(T, 1))[1] for b in range(B)]).astype(F32)
    ys[:, 2, :] = np.nan
    ys[0, 1, 0] = ys[1, 1, 1] = ys[0, 5, 1] = ys[1, 7, 0] = np.nan
    ys[1, T - 1, :] = np.nan
    g_reg, g_usr = nl.bearing_range(), nl.user_emission(BOT_EMI_SRC, 4, 2)
    reg = bfa.ParamsBPF(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Q, g_reg, r0, R, nl.gaussian_log_prob(g_reg, R, r0))
    usr = reg._replace(emission_function=g_usr, emission_distribution_log_prob=nl.gaussian_log_prob(g_usr, R, r0))
    key = np.array([0, 5], np.uint32)
    kw = dict(output="both", return_ancestors=True, missing="nan")
    a = bfa.bootstrap_particle_filter(reg, ys, N, key, inputs, **kw)
    b_ = bfa.bootstrap_particle_filter(usr, ys, N, key, inputs, **kw)
    assert np.isfinite(a["logz"].cpu().numpy()).all() and 0 < float(a["resampled"].mean()) < 1
    for k in a:
        assert _same(a[k].cpu().numpy(), b_[k].cpu().numpy()), k


LP_SRC = """
template <class T> __device__ T log_prob(const T* x, const float* y, T u, const float* th) {   // th: H (M x N), bias (M), variances (M)
  T s = 0.0f;
  for (int a = 0; a < BF_M; ++a) {
    if (NAN_AWARE && y[a] != y[a]) continue;
    T mu = th[BF_M * BF_N + a];
    for (int j = 0; j < BF_N; ++j) mu = fma(th[a * BF_N + j], x[j], mu);
    const T v = y[a] - mu;
    const float var = th[BF_M * BF_N + BF_M + a];
    s = s - 0.5f * (v * v / var + log(6.283185307179586f * var));
  }
  return s;
}
"""


def _diag_density_model(nan_aware):
    """The 1x4 row's model with a diagonal density written as source (independent components: what a per-component NaN test
    can marginalise)."""
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    case = prc.BY_ID["1x4"]
    a = dict(prc.arrays(case))
    var = np.diag(a["Rlp"]).astype(F32)
    a["Rlp"] = np.diag(var).astype(F32)
    bias = (a["D"].astype(np.float64) @ a["r0"].astype(np.float64)).astype(F32)
    theta = np.concatenate([a["H"].reshape(-1), bias, var]).astype(F32)
    lp = nl.user_log_prob(LP_SRC.replace("NAN_AWARE", "true" if nan_aware else "false"), theta=theta)
    pp = prc.engine_params(case, a)._replace(emission_distribution_log_prob=lp)
    return case, a, pp


def test_log_density_from_source_that_treats_nan_takes_partial_gaps():
    case, a, pp = _diag_density_model(True)
    ys = pmc.gapped(prc.observations(case, a))
    out = _run(case, pp, ys, ess_threshold=0.0, output="both")
    assert not out["resampled"].any()
    for b in range(case.B):
        x, w = out["particles"][b], out["weights"][b]
        assert np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(out["logz"][b]).all(), b
        lz, wn, mean = pmc.recompute_f64(a, x, w, ys[b])
        gz, gm = prc.logz_gap(out["logz"][b], lz), cm.rel_err(out["mean"][b], mean)
        print(f"b={b}: logz gap {gz:.2e} (bound {pmc.LOGZ_BOUND_CANONICAL:.1e}), mean rel_err {gm:.2e}")
        assert gz <= pmc.LOGZ_BOUND_CANONICAL, (b, gz)
        assert gm <= pmc.MEAN_BOUND_F64, (b, gm)
        assert abs(float(out["logz"][b, 2])) <= 2 * np.finfo(F32).eps           # the wholly missing step: the function is not called


def test_log_density_from_source_that_does_not_is_poisoned_by_a_partial_gap_only():
    case, a, pp = _diag_density_model(False)
    case = case._replace(B=3)
    ys = prc.observations(case, a, B=3)
    clean = _run(case, pp, ys, output="both")
    ys[1, 2, :] = np.nan                      # a whole gap alone: the function is not called
    ys[2, 2, :] = np.nan
    ys[2, 3, 1] = np.nan                      # ... and a partial one after it: handed to the function as it is
    out = _run(case, pp, ys, output="both")
    for k in ("weights", "particles", "logz", "ess"):
        assert _bits_equal(out[k][0], clean[k][0]), k
        assert np.isfinite(out[k][1]).all(), k
    assert _bits_equal(out["weights"][1][:, :2], clean["weights"][1][:, :2])
    assert np.isfinite(out["weights"][2][:, :3]).all() and np.isfinite(out["logz"][2, :3]).all()
    assert np.isnan(out["weights"][2][:, 3:]).all() and np.isnan(out["logz"][2, 3:]).all() and np.isnan(out["ess"][2, 3:]).all()
    assert (out["resampled"][2, 3:] == 0).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_observed_mask_in_its_four_shapes_is_the_nan_form():
    import torch
    case = prc.BY_ID["1x4"]
    a, pp, ys, _ = _setup(case)
    B, T, m = ys.shape
    rng = np.random.default_rng(5)
    for shape in ((T,), (B, T), (T, m), (B, T, m)):
        mask = rng.random(shape) > 0.35
        mask.reshape(-1)[0] = False
        full = {(T,): lambda: mask[None, :, None], (B, T): lambda: mask[:, :, None], (T, m): lambda: mask[None]}.get(shape, lambda: mask)()
        as_nan = np.where(np.broadcast_to(full, ys.shape), ys, np.nan).astype(F32)
        want = _run(case, pp, as_nan, output="both")
        for given in (ys.copy(), torch.as_tensor(ys.copy(), device="cuda")):
            before = given.clone() if isinstance(given, torch.Tensor) else given.copy()
            got = _run(case, pp, given, output="both", missing=None, observed=mask)
            for k in want:
                assert _same(want[k], got[k]), (shape, k)
            assert (torch.equal(given, before) if isinstance(given, torch.Tensor) else np.array_equal(given, before)), shape
        assert np.isfinite(want["logz"]).all()


@pytest.mark.parametrize("cid", ["1x4", "big", "wide-five-chunks-B3"])
def test_chunks_cut_inside_the_gap_and_summary_output(cid):
    """Two chunks through the carry, cut before and after the wholly missing step 2, equal the single call bit for bit;
    output="summary" equals output="both"."""
    case = prc.BY_ID[cid]
    a, pp, _, ys = _setup(case)
    both = _run(case, pp, ys, output="both")
    assert np.isfinite(both["logz"]).all()
    summ = _run(case, pp, ys, output="summary")
    assert set(summ) == set(SUMMARY)
    for k in SUMMARY:
        assert _bits_equal(summ[k], both[k]), k
    for cut in (2, 3):
        h1, c1 = _run(case, pp, ys[:, :cut], output="both", return_carry=True)
        h2, c2 = _run(case, pp, ys[:, cut:], output="both", carry=c1, keyed=False, return_carry=True)
        for k in h1:
            if k == "ancestors":
                assert np.array_equal(np.concatenate([h1[k], h2[k]], axis=2), both[k]), (cut, k)
                continue
            axis = 2 if k in ("weights", "particles") else 1
            assert _bits_equal(np.concatenate([h1[k], h2[k]], axis=axis), both[k]), (cut, k)


@pytest.mark.parametrize("cid", ["1x16", "wide-five-chunks-B3"])
def test_infinity_is_not_missing_and_plain_route_still_poisons(cid):
    """B = 3: +Inf (then -Inf) in an OBSERVED entry of trajectory 1 at step 3, next to a missing one, poisons trajectory 1 from
    step 3 on and nothing else; without the keyword the NaN of the gap pattern poisons from its first step."""
    case = prc.BY_ID[cid]._replace(B=3)
    a = prc.arrays(case)
    pp = prc.engine_params(case, a)
    ys = pmc.gapped(prc.observations(case, a, B=3))
    clean = _run(case, pp, ys, output="both")
    assert np.isfinite(clean["logz"]).all() and np.isfinite(clean["weights"]).all()
    m = ys.shape[2]
    for inf in (np.inf, -np.inf):
        bad_ys = ys.copy()
        bad_ys[1, 3, 0] = inf
        if m > 1:
            bad_ys[1, 3, 1] = np.nan
        bad = _run(case, pp, bad_ys, output="both")
        for k in clean:
            t_axis = 1 if k in ("weights", "particles", "ancestors") else 0
            for b in (0, 2):
                assert _same(clean[k][b], bad[k][b]), (k, b)
            assert _same(np.take(clean[k][1], range(3), axis=t_axis), np.take(bad[k][1], range(3), axis=t_axis)), k
        assert not np.isfinite(bad["logz"][1, 3:]).any() and not np.isfinite(bad["ess"][1, 3:]).any(), (bad["logz"][1], bad["ess"][1])
        assert np.isnan(bad["weights"][1][:, 3:]).all()
        assert (bad["resampled"][1, 3:] == 0).all()
    plain = _run(case, pp, ys, output="both", missing=None)
    assert not np.isfinite(plain["logz"][:, 1:]).any() and np.isfinite(plain["logz"][:, 0]).all(), plain["logz"]
    assert np.isnan(plain["weights"][:, :, 1:]).all()


@pytest.mark.parametrize("method", ["backward", "genealogy"])
def test_posterior_sample_wrapper_takes_the_keywords(method):
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import random as bfr
    case = prc.BY_ID["1x4"]
    a, pp, _, ys = _setup(case)
    key = np.array([3, 11], np.uint32)
    S = 5
    xs = bfa.bootstrap_particle_posterior_sample(pp, ys, case.N, S, key, missing="nan", method=method).cpu().numpy()
    assert xs.shape == (case.B, S, case.T, case.dims[0]) and np.isfinite(xs).all()
    kf, _ = bfr.split(key, 2)
    filt = bfa.bootstrap_particle_filter(pp, ys, case.N, kf, missing="nan")["particles"].cpu().numpy()      # (B, N, T, n)
    for b in range(case.B):
        for t in range(case.T):
            stored = {row.tobytes() for row in filt[b, :, t]}
            assert all(xs[b, s, t].tobytes() in stored for s in range(S)), (b, t)
    mask = ~np.isnan(ys)
    ys0 = np.where(mask, ys, 0.0).astype(F32)
    xo = bfa.bootstrap_particle_posterior_sample(pp, ys0, case.N, S, key, observed=mask, method=method).cpu().numpy()
    assert _bits_equal(xo, xs)
