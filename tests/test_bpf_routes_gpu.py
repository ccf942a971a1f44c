"""The bootstrap particle filter on EVERY kernel route (tests/particle_route_cases.py: five one-particle-per-thread capacities,
4x16 with the model structure at run time and at compile time, the 8x8 geometry, 16x16, particles in HBM per trajectory and
per chunk, the run-time build with and without the hardware's transcendentals), with the two quantities that no other test
compares with anything but another kernel: the per-step log-evidence `logz` and the weighted `mean`.

  1. bits of the oracle (arith="canonical"; dbg["logz"] is defined to the bit like the ESS) at the default ESS threshold, on
     seeds for which some steps resample and some do not;
  2. float64 from the engine's OWN emitted particles and weights at ess_threshold = 0 (teacher-forced: nothing compounds, no
     bit-exact ancestry needed, so it also judges the hardware-arithmetic build), the density written with inv / slogdet;
  3. the contract of the summary streams (summary == both, chunked through the carry == one shot, a trajectory alone == its row);
  4. a NaN observation stays in its trajectory;
  5. two calls that the dispatch sends to different kernels agree in every weight and differ in the bits of `mean` (the one
     witness of the route that the outputs offer);
  6. what holds when a draw falls inside an inversion of the non-monotone fp32 CDF, where the in-register kernels' probe
     sequence and the oracle's bisection may take different, equally valid ancestors (found by row 16x16-upper-end).

The rows of the run-time build (jit-*, hw-*) pay one hiprtc compile each on a cold kernel cache (seconds); everything else
is a few launches.  The two hardware-arithmetic rows of dimensions (8, 8, 4) run one right after the other in one test: they
share dimensions and capacity and differ in the model-structure spec only, which the kernel cache must key on.

Bounds.  logz against float64: canonical rows 10 x the worst fp32-ORACLE-against-float64 gap measured on the CPU on these same
rows (particle_route_cases.ORACLE_LOGZ_GAP, 2.4e-8 ... 2.8e-7 -> 2.8e-6), hardware arithmetic the 2e-5 that
test_hardware_arithmetic_option_agrees_to_rounding holds between the two arithmetics; mean: the standing rel_err <= 1e-5;
weights: the teacher-forced bound of test_particle_filter_with_a_log_density_from_source.

Measured on an MI355X (worst over the row's trajectories and steps; logz as |d| / (1 + |ref|), mean as rel_err):
  route                              logz, float64   oracle's gap (CPU)   mean, float64   mean, oracle's mean64
  1x1                                1.2e-07         1.2e-07              7.1e-08         1.2e-07
  1x2                                7.4e-08         7.4e-08              5.6e-08         6.1e-08
  1x4                                1.9e-07         1.8e-07              8.4e-08         9.8e-08
  1x8                                2.5e-07         2.5e-07              1.0e-07         6.0e-08
  1x16                               1.6e-07         1.6e-07              7.4e-08         1.2e-07
  4x16-runtime-nearly-empty-waves    2.4e-08         2.4e-08              1.0e-07         9.0e-08
  4x16-runtime-ragged-last-thread    9.9e-08         9.8e-08              1.6e-07         9.8e-08
  4x16-fixed                         8.4e-08         8.4e-08              1.5e-07         1.2e-07
  4x16-fixed-spec-off                8.4e-08         8.4e-08              1.5e-07         1.2e-07
  8x8-fixed                          1.4e-07         1.4e-07              1.4e-07         1.1e-07
  8x8-spec-off                       1.4e-07         1.4e-07              1.4e-07         1.1e-07
  16x16                              8.7e-08         8.7e-08              9.6e-08         9.4e-08
  16x16-upper-end                    1.6e-07         1.6e-07              1.3e-07         5.7e-08
  big                                6.4e-08         6.4e-08              9.9e-08         4.4e-08
  wide-five-chunks-B1                1.5e-07         1.5e-07              9.2e-08         8.3e-08
  wide-five-chunks-B3                2.8e-07         2.8e-07              7.7e-08         1.2e-07
  wide-by-default                    8.4e-08         8.4e-08              1.3e-07         1.1e-07
  in-register-by-default-B40         1.1e-07         1.1e-07              9.5e-08         9.8e-08
  jit-no-compiled-instance           2.0e-07         2.0e-07              1.3e-07         7.8e-08
  jit-big                            1.1e-07         1.1e-07              7.2e-08         6.1e-08
  hw-4x16-fixed                      6.4e-08         8.4e-08              9.9e-08         -
  hw-big-fixed                       1.1e-07         1.0e-07              1.4e-07         -
  hw-big-runtime-same-dims           8.3e-08         9.0e-08              6.9e-08         -
  (logz bits: all 20 canonical routes equal to the oracle's, every step of every trajectory compared)
"""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import particle_route_cases as prc

pytestmark = pytest.mark.gpu
F32 = np.float32
SUMMARY = ("mean", "ess", "logz", "resampled")


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def _same(x, y):
    """Every bit, whatever the stream's type (ancestors are int32)."""
    return _bits_equal(x, y) if x.dtype == F32 else np.array_equal(x, y)


def _run(case, pp, ys, ess_threshold=0.5, output="both", key=None, carry=None, return_carry=False, options=None, keyed=True):
    """One call on the row's route: per-call options, bpf_spec (not a per-call option) set and restored around it.  Always a
    (B, T, m) batch, so every output keeps its batch axis.  Returns NumPy arrays (and the carry)."""
    import bayesianfiltering_amd as bfa
    from bayesianfiltering_amd import _lib
    lib = _lib.require_gpu()
    assert ys.ndim == 3
    key = prc.key_of(case) if (key is None and keyed) else key
    if case.spec is not None:
        _lib.check(lib.bf_set_option(b"bpf_spec", case.spec))
    try:
        got = bfa.bootstrap_particle_filter(pp, ys, case.N, key, None, ess_threshold, resampler=case.resampler, output=output,
                                            carry=carry, return_carry=return_carry, return_ancestors=output != "summary",
                                            options=case.options if options is None else options)
    finally:
        if case.spec is not None:
            _lib.check(lib.bf_set_option(b"bpf_spec", 1))
    out, c = got if return_carry else (got, None)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return (out, c) if return_carry else out


def _setup(case, B=None):
    a = prc.arrays(case)
    return a, prc.engine_params(case, a), prc.observations(case, a, B)


@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_route_gives_the_oracles_bits(case):
    """Resampling decisions, ancestors, weights, particles, ESS and logz equal to the oracle's bits, mean to 1e-5 of the
    oracle's float64 mean, over steps that do and do not resample."""
    a, pp, ys = _setup(case)
    po = prc.oracle_params(case, a)
    out = _run(case, pp, ys, output=case.output)
    res, worst = [], 0.0
    for b in prc.oracle_trajectories(case):
        ref, dbg = go.bootstrap_particle_filter(po, ys[b], case.N, key=prc.key_of(case), resampler=case.resampler, debug=True,
                                                arith="canonical")
        res.append(dbg["resampled"])
        assert not dbg["ambiguous"].any()         # (the seed's choice: every draw's ancestor is defined by the CDF alone)
        assert np.array_equal(out["resampled"][b] > 0.5, dbg["resampled"]), b
        if case.output == "both":
            assert np.array_equal(out["ancestors"][b].T, dbg["ancestors"]), b
            assert _bits_equal(out["weights"][b], ref["weights"]), b
            assert _bits_equal(out["particles"][b], ref["particles"]), b
        assert _bits_equal(out["ess"][b], dbg["ess"]), b
        nbad = int((out["logz"][b].view(np.uint32) != dbg["logz"].view(np.uint32)).sum())
        err = cm.rel_err(out["mean"][b], dbg["mean64"])
        worst = max(worst, err)
        print(f"{case.id} b={b}: logz words that differ {nbad}/{case.T}, mean rel_err {err:.2e}")
        assert _bits_equal(out["logz"][b], dbg["logz"]), (b, out["logz"][b], dbg["logz"])
        assert err <= prc.MEAN_BOUND, (b, err)
    res = np.array(res)
    assert 0 < res.sum() < res.size, res              # both branches ran (a property of the oracle's run: the seed's choice)
    cm.record(f"bpf_route_oracle_bits[{case.id}]", mean_rel_err=worst)


def _against_float64(case):
    a, pp, ys = _setup(case)
    out = _run(case, pp, ys, ess_threshold=0.0, output="both")
    assert not out["resampled"].any()
    bound = prc.LOGZ_BOUND_HARDWARE if case.arith else prc.LOGZ_BOUND_CANONICAL
    worst_z = worst_m = worst_w = 0.0
    checks = []
    for b in prc.oracle_trajectories(case):
        x, w = out["particles"][b], out["weights"][b]
        assert np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(out["logz"][b]).all()
        lz, wn, mean = prc.recompute_f64(a, x, w, ys[b])
        gz = prc.logz_gap(out["logz"][b], lz)
        gm = cm.rel_err(out["mean"][b], mean)
        wtol = 2e-5 * np.maximum(1.0, w.max(axis=0) * case.N) / case.N + 1e-7           # per step
        gw = float(np.max(np.abs(wn - w) / wtol))
        print(f"{case.id} b={b}: logz gap {gz:.2e} (bound {bound:.1e}), mean rel_err {gm:.2e}, weights {gw:.2f} of their bound")
        worst_z, worst_m, worst_w = max(worst_z, gz), max(worst_m, gm), max(worst_w, gw)
        checks.append((b, gz, gm, gw))
    cm.record(f"bpf_route_float64[{case.id}]", logz_gap=worst_z, mean_rel_err=worst_m, weights_of_bound=worst_w)
    for b, gz, gm, gw in checks:
        assert gz <= bound, (case.id, b, gz)
        assert gm <= prc.MEAN_BOUND, (case.id, b, gm)
        assert gw < 1.0, (case.id, b, gw)


@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_route_against_float64_from_its_own_particles(case):
    """ess_threshold = 0: logz_t, the normalised weights and mean_t recomputed in float64 from the emitted particles of step t
    and the emitted weights of step t - 1."""
    _against_float64(case)


def test_hardware_arithmetic_routes_against_float64_from_their_own_particles():
    """The same for bpf_arith = 1 (in-register SpecFixed; particles in HBM with SpecFixed -- an instance that exists on this
    path only -- and right after it with SpecRuntime at the same dimensions and capacity: a kernel cache that did not key on
    the spec would hand the dense linear model the Lorenz-96 kernel)."""
    for case in prc.HARDWARE:
        _against_float64(case)


CONTRACT = ["1x4", "4x16-fixed", "big", "wide-five-chunks-B3"]


@pytest.mark.parametrize("cid", CONTRACT)
def test_summary_streams_contract(cid):
    """output="summary" gives the bits of output="both"; two chunks through the carry give the one-shot bits of mean, ESS, logz
    and resampled (and of weights and particles); on the workgroup-per-chunk kernels, whose launches and HBM scratch are
    shared between the trajectories, each trajectory filtered alone equals its row."""
    case = prc.BY_ID[cid]
    a, pp, ys = _setup(case)
    both = _run(case, pp, ys, output="both")
    res = both["resampled"]
    assert 0 < res.sum() < res.size, res
    summ = _run(case, pp, ys, output="summary")
    assert set(summ) == set(SUMMARY)
    for k in SUMMARY:
        assert _bits_equal(summ[k], both[k]), k
    cut = case.T // 2
    for output in ("both", "summary"):
        h1, c1 = _run(case, pp, ys[:, :cut], output=output, return_carry=True)
        h2 = _run(case, pp, ys[:, cut:], output=output, carry=c1, keyed=False)
        for k in h1:
            if k == "ancestors":
                continue
            axis = 2 if k in ("weights", "particles") else 1
            assert _bits_equal(np.concatenate([h1[k], h2[k]], axis=axis), both[k]), (output, k)
    if cid.startswith("wide"):
        for b in range(case.B):
            alone = _run(case, pp, ys[b:b + 1], output="both")
            for k in both:
                assert _same(alone[k][0], both[k][b]), (b, k)


@pytest.mark.parametrize("cid", ["1x16", "wide-five-chunks-B3"])
def test_nan_observation_stays_in_its_trajectory(cid):
    """B = 3, a NaN in trajectory 1's observation of step 3: trajectories 0 and 2 keep every bit of the clean run, trajectory 1
    keeps them before step 3; from step 3 on its logz and mean are not finite and it never resamples (its ESS is NaN, and
    NaN < threshold N is false) -- what VERDICT.md describes for the non-finite trajectories of the benchmark."""
    case = prc.BY_ID[cid]._replace(B=3)
    a, pp, ys = _setup(case, B=3)
    clean = _run(case, pp, ys, output="both")
    bad_ys = ys.copy()
    bad_ys[1, 3, 0] = np.nan
    bad = _run(case, pp, bad_ys, output="both")
    for k in clean:
        t_axis = 1 if k in ("weights", "particles", "ancestors") else 0
        for b in (0, 2):
            assert _same(clean[k][b], bad[k][b]), (k, b)
        assert _same(np.take(clean[k][1], range(3), axis=t_axis), np.take(bad[k][1], range(3), axis=t_axis)), k
    assert not np.isfinite(bad["logz"][1, 3:]).any(), bad["logz"][1]
    assert not np.isfinite(bad["mean"][1, 3:]).any(), bad["mean"][1]
    assert not np.isfinite(bad["ess"][1, 3:]).any(), bad["ess"][1]
    assert (bad["resampled"][1, 3:] == 0).all(), bad["resampled"][1]
    assert np.isfinite(clean["logz"]).all() and np.isfinite(clean["mean"]).all()


# The one witness of the route that the outputs offer: two calls that the dispatch sends to different kernels agree in every
# weight and differ in the bits of `mean`, whose sum order belongs to the kernel.  (row, options of one call, of the other)
WITNESS = [
    ("wide-by-default", {}, prc.M1),                                                  # wide | 4x16 SpecFixed
    ("in-register-by-default-B40", {}, None),                                         # 4x16 | its first two trajectories alone: wide
    ("16x16", prc.M1, prc.M2),                                                        # 16x16 | wide
    ("big", prc.M1, prc.M2),                                                          # big | wide
    ("8x8-fixed", {"bpf_hbm_mode": 1, "bpf_variant": 1}, {"bpf_hbm_mode": 1, "bpf_variant": 0}),    # 8x8 | 4x16
]


@pytest.mark.parametrize("cid,opt_a,opt_b", WITNESS, ids=[w[0] for w in WITNESS])
def test_the_options_reach_different_kernels(cid, opt_a, opt_b):
    case = prc.BY_ID[cid]
    a, pp, ys = _setup(case)
    ra = _run(case, pp, ys, output="both", options=opt_a)
    if opt_b is None:      # (B = 40 > 32 stays in the registers whatever bpf_hbm_mode says; two of its trajectories alone are spread)
        rb = _run(case, pp, ys[:2], output="both", options={})
        ra_all, ra = ra, {k: v[:2] for k, v in ra.items()}
    else:
        rb = _run(case, pp, ys, output="both", options=opt_b)
    for k in ("weights", "particles", "ess", "logz", "resampled"):
        assert _bits_equal(ra[k], rb[k]), k
    assert np.array_equal(ra["ancestors"], rb["ancestors"])
    assert cm.rel_err(ra["mean"], rb["mean"]) <= prc.MEAN_BOUND
    assert not _bits_equal(ra["mean"], rb["mean"])
    if cid == "in-register-by-default-B40":          # ... and B = 40 > 32 by the default rule IS the workgroup-per-trajectory instance
        r1 = _run(case, pp, ys, output="both", options=prc.M1)
        for k in ra_all:
            assert _same(ra_all[k], r1[k]), k


def test_draw_inside_a_cdf_inversion():
    """The fp32 CDF in associative-scan order is not monotone, and a draw that falls inside an inversion has no ancestor that
    the CDF alone defines: the oracle and the particles-in-HBM kernels bisect like NumPy (lo = 0, hi = N), the in-register
    kernels probe power-of-two strides, and the two can return different, equally valid indices.  On this seed the oracle
    flags one such draw in the first resampling of trajectory 0 (CPU emulation of the in-register probe sequence: ancestor
    13040 where NumPy's bisection gives 13038, c[13038] == r > c[13039]).  What holds and is asserted: the workgroup-per-chunk
    route equals the oracle bit for bit throughout; the in-register route equals it up to the first step with a flagged draw,
    differs there in flagged draws only, and each of its answers has the CDF at or above the oracle's answer within one
    inversion (no mass in between)."""
    case = prc.INVERSION
    a, pp, ys = _setup(case)
    po = prc.oracle_params(case, a)
    reg = _run(case, pp, ys, output="both", options=prc.M1)
    wide = _run(case, pp, ys, output="both", options=prc.M2)
    flagged = 0
    for b in range(case.B):
        ref, dbg = go.bootstrap_particle_filter(po, ys[b], case.N, key=prc.key_of(case), resampler=case.resampler, debug=True,
                                                arith="canonical")
        assert np.array_equal(wide["ancestors"][b].T, dbg["ancestors"]), b
        assert _bits_equal(wide["weights"][b], ref["weights"]) and _bits_equal(wide["particles"][b], ref["particles"]), b
        assert _bits_equal(wide["logz"][b], dbg["logz"]) and _bits_equal(wide["ess"][b], dbg["ess"]), b
        amb = dbg["ambiguous"]
        flagged += int(amb.sum())
        t_ok = int(np.argmax(amb.any(axis=1))) if amb.any() else case.T          # the first step with a flagged draw
        assert np.array_equal(reg["ancestors"][b].T[:t_ok], dbg["ancestors"][:t_ok]), b
        assert _bits_equal(reg["weights"][b][:, :t_ok], ref["weights"][:, :t_ok]), b
        assert _bits_equal(reg["particles"][b][:, :t_ok], ref["particles"][:, :t_ok]), b
        assert _bits_equal(reg["logz"][b][:t_ok + 1], dbg["logz"][:t_ok + 1]), b         # (logz of a step precedes its resampling)
        if t_ok < case.T:
            got, want = reg["ancestors"][b].T[t_ok], dbg["ancestors"][t_ok]
            diff = np.flatnonzero(got != want)
            print(f"b={b} step {t_ok}: flagged draws {np.flatnonzero(amb[t_ok])}, differing {diff}, {got[diff]} for {want[diff]}")
            assert np.isin(diff, np.flatnonzero(amb[t_ok])).all(), diff
            from oracle import threefry as otf
            cdf = otf.cumsum_assoc(dbg["pre_weights"][t_ok]).astype(np.float64)
            for i in diff:
                lo, hi = min(got[i], want[i]), max(got[i], want[i])
                assert cdf[lo:hi].min() <= cdf[lo] and cdf[hi - 1] - cdf[lo] <= 0.0, (i, cdf[lo - 1:hi + 1])
    assert flagged > 0                                  # (the seed's choice: a property of the oracle's run)
