"""The cases of tests/test_missing_instances_gpu.py, no GPU: the case lists are the compiled tables as the missing-observation
build of the slices takes them (a row added later fails here until it has a case), the vectorised float64 Kalman recursion is the
per-trajectory one of kalman_missing_cases.py, every gap pattern occurs, the list of rows without staged tiles is what the
headers' formulas give, and on every case the float32 reference is within a fraction of the asserted tolerance of float64 (the
project's rule: the tolerance never moves, the inputs do)."""

import numpy as np
import pytest

from tests import common as cm
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc
from tests import kalman_staged_cases as ks
from tests import missing_instance_cases as mi

KIDS = [mi.pair_id(p) for p in mi.KALMAN]
GIDS = [mi.gsf_id(r) for r in mi.GSF_REACHABLE]
CPU_NREF = 8          # trajectories of a Gaussian-sum case whose headroom is checked here (the fixed patterns among them)


# ---- the instance tables ------------------------------------------------------------------------------------------------
def test_kalman_cases_are_the_compiled_instances():
    plain = [r for g in "abcd" for r in cm.instance_rows(f"kf_group_{g}.hip")]
    compiled = [r for g in "abcd" for r in cm.instance_rows(f"kf_group_{g}.hip", missing=True)]
    assert len(plain) == len(set(plain)) == 28 and len(compiled) == len(set(compiled)) == 26
    assert set(plain) - set(compiled) == {(4, 2, 1), (4, 2, 4)}      # the rows marked plain-only: the other lanes of (4, 2)
    assert [r for r in plain if r in compiled] == compiled
    cm.assert_slices_are_built_twice("kf", "abcd", "launch_nml<N_, M_, NL_, BF_MISSING>", "kf_scan_group.hip")
    assert set(compiled) == {(n, m, ks.default_lanes(n)) for n, m in mi.KALMAN}
    assert len(mi.KALMAN) == len(set(mi.KALMAN)) == 26
    assert all(mi.geometry(n, m)["lanes"] == ks.default_lanes(n) for n, m in mi.KALMAN)


def test_gaussian_sum_cases_are_the_compiled_instances():
    compiled = [(mi.GENERIC,) + r for g in "abcd" for r in cm.instance_rows(f"gsf_group_{g}.hip", missing=True)]
    compiled += [(mi.L96,) + r for r in cm.instance_rows("gsf_group_e.hip", missing=True)]
    assert len(compiled) == len(set(compiled)) == 33
    cm.assert_slices_are_built_twice("gsf", "abcd", "SPEC_GENERIC, BF_MISSING>", "gsf_scan.hip")
    cm.assert_slices_are_built_twice("gsf", "e", "SPEC_L96_PICK, BF_MISSING>", "gsf_scan.hip")
    assert len(mi.GSF_REACHABLE) == len(set(mi.GSF_REACHABLE)) == 29 and len(mi.GSF_UNREACHABLE) == 4
    assert set(compiled) == set(mi.GSF_REACHABLE) | set(mi.GSF_UNREACHABLE)
    # unreachable = the rows whose lanes are not the default of their n, which is all the entry point passes on
    src = cm.read_csrc("gsf_scan.hip")
    assert "static const int kGsfDefaultLanes[9] = {0, 1, 1, 1, 2, 1, 2, 1, 2};" in src
    assert "if (lanes == 0) lanes = gsf_default_lanes(p->n);" in src
    assert "if (lanes != 0 && lanes != bf::gsf_default_lanes(model->n))" in cm.read_csrc("bf_api.hip")
    assert mi.GSF_DEFAULT_LANES == (0, 1, 1, 1, 2, 1, 2, 1, 2)
    assert set(mi.GSF_UNREACHABLE) == {r for r in compiled if r[3] != mi.GSF_DEFAULT_LANES[r[1]]}
    # every generic pair of the Kalman table has its row, and the structured rows are Lorenz-96 shapes (m = n / 2)
    assert {r[1:3] for r in mi.GSF_REACHABLE if r[0] == mi.GENERIC} == set(mi.KALMAN)
    assert all(2 * r[2] == r[1] for r in compiled if r[0] == mi.L96)


def test_unscented_cases_are_the_compiled_instances():
    compiled = cm.instance_rows("ugsf_group_u.hip", missing=True) + cm.instance_rows("ugsf_group_v.hip", missing=True)
    cm.assert_slices_are_built_twice("ugsf", "uv", "launch_ugsf<N_, DQ_, M_, DR_, BF_MISSING>", "ugsf_scan.hip")
    assert len(compiled) == len(set(compiled)) == 9
    assert set(compiled) == set(mi.UKF_SHAPES) | set(mi.UKF_COVERED_ELSEWHERE)
    assert len(mi.UKF_SHAPES) == 6 and not set(mi.UKF_SHAPES) & set(mi.UKF_COVERED_ELSEWHERE)


# ---- rows without staged tiles: GsfCfg / Tile (csrc/gsf_scan.hpp, csrc/scan_common.hpp) restated ----------------------------
def _gsf_staged_ok(n, nl, wsm=16):
    cpw, ep, wmin = 64 // nl, n * n, 4 * nl
    wp = max(max(ep, 32), wmin)
    wm = max(max(n, wsm), wmin)
    ww = max(wsm, wmin)

    def ok(e, w, pad):
        ch, nchunk = w // 4, cpw * (w // 4)
        pow2 = (ch & (ch - 1)) == 0 and nchunk >= 64 and nchunk % 64 == 0
        return w % e == 0 and w % 4 == 0 and pad % 4 == 0 and pow2
    return ok(ep, wp, 4) and ok(n, wm, 4) and ok(1, ww, 0)


def test_rows_without_staged_tiles():
    hpp, common = cm.read_csrc("gsf_scan.hpp"), cm.read_csrc("scan_common.hpp")
    for line in ("static constexpr int CPW = 64 / NL;  // chains per wave", "static constexpr int EP = NS * NS;",
                 "static constexpr int WMIN = 4 * NL;",
                 "static constexpr int WP = (EP >= 32 ? EP : 32) > WMIN ? (EP >= 32 ? EP : 32) : WMIN;",
                 "static constexpr int WSM = 16;",
                 "static constexpr int WM = (NS >= WSM ? NS : WSM) > WMIN ? (NS >= WSM ? NS : WSM) : WMIN;",
                 "static constexpr int WW = WSM > WMIN ? WSM : WMIN;",
                 "using TP = Tile<EP, WP, CPW, 4>;", "using TM = Tile<NS, WM, CPW, 4>;", "using TW = Tile<1, WW, CPW, 0>;",
                 "static constexpr bool STAGED_OK = TP::OK && TM::OK && TW::OK;"):
        assert line in hpp, line
    for line in ("static constexpr int CH = W / 4;", "static constexpr int NCHUNK = CPW * CH;",
                 "static constexpr bool POW2 = ((CH & (CH - 1)) == 0) && (NCHUNK >= 64) && (NCHUNK % 64 == 0);",
                 "static constexpr bool GOK = (W % E == 0) && (W % 4 == 0) && (PAD % 4 == 0);",
                 "static constexpr bool OK = GOK && POW2;"):
        assert line in common, line
    for spec, n, m, lanes in mi.GSF_REACHABLE + mi.GSF_UNREACHABLE:
        assert _gsf_staged_ok(n, lanes) == (n not in mi.GSF_NO_STAGED_N), (spec, n, m, lanes)


def test_staged_runs_meet_the_launch_conditions():
    """launch_gsf: K == KP, B % tpb == 0, (B K) % CPW == 0, rows of T n and T n^2 floats 16-byte aligned, at every row."""
    r = mi.GSF_RUNS["staged"]
    for row in mi.GSF_REACHABLE:
        _, n, _, lanes = row
        K = mi.gsf_K(row, "staged")
        tpb = 256 // (K * lanes)
        assert K & (K - 1) == 0 and r["B"] % tpb == 0 and (r["B"] * K) % (64 // lanes) == 0
        assert (r["T"] * n) % 4 == 0 and (r["T"] * n * n) % 4 == 0
    assert mi.GSF_RUNS["strided"]["T"] % 4 and mi.GSF_RUNS["strided"]["B"] % 4     # and the strided run is ragged in both


# ---- the vectorised float64 Kalman recursion ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["const", "QR"])
@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_batched_float64_recursion_is_the_per_trajectory_one(pair, variant):
    n, m = pair
    d, a = mi.kalman_data(n, m), dict(mi.model(n, m))
    Qt, Rt = mi.variant_tables(n, m, variant)
    if Qt is not None:
        a["Q"], a["R"] = Qt, Rt
    ref = mi.kalman_reference(n, m, variant)
    B = d["gapped"].shape[0]
    for b in list(range(mi.HEADROOM_B)) + [B - 1]:
        one = kc.kalman_missing_f64(a, d["gapped"][b], d["m0s"][b], d["P0s"][b])
        for k in kc.STREAMS + ("loglik",):
            assert ref[k].dtype == np.float64 and ref[k][b, 0].shape == one[k].shape
            assert cm.rel_err(ref[k][b, 0], one[k]) < 1e-12, (b, k)


@pytest.mark.parametrize("pair", [(3, 2), (6, 4), (8, 1)], ids=mi.pair_id)
def test_batched_float64_recursion_on_complete_data_is_the_plain_one(pair):
    n, m = pair
    d, a = mi.kalman_data(n, m), mi.model(n, m)
    for tables in ((None, None), mi.kalman_tables(n, m)):
        got = mi.kalman_missing_f64_batched(a, d["ys"][:9], d["m0s"][:9], d["P0s"][:9], *tables)
        want = ks.kalman_f64_batched(a, d["ys"][:9], d["m0s"][:9], d["P0s"][:9], *tables)
        assert set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape and cm.rel_err(got[k], want[k]) < 1e-12, k


# ---- patterns --------------------------------------------------------------------------------------------------------------
def _patterns(mask):
    m = mask.shape[-1]
    return set(np.unique(mask.reshape(-1, m) @ (1 << np.arange(m))))


def _assert_fixed_trajectories(mask):
    B, T, m = mask.shape
    assert mask[kc.FULL].all() and not mask[kc.NONE].any()
    c = min(1, m - 1)
    assert not mask[kc.NO_COMP1, :, c].any() and np.delete(mask[kc.NO_COMP1], c, axis=1).all()
    rest = np.delete(mask, [kc.FULL, kc.NO_COMP1], axis=0)
    assert not rest[:, 0].any() and not rest[:, T - kc.FORECAST:].any()


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_masks(pair):
    n, m = pair
    g, mask = mi.geometry(n, m), mi.kalman_data(n, m)["mask"]
    assert mask.shape == (g["B"], g["t_max"], m)
    assert _patterns(mask[:mi.HEADROOM_B]) == set(range(2 ** m))       # every pattern, among the trajectories with headroom
    _assert_fixed_trajectories(mask)
    rest = np.delete(mask, [kc.FULL, kc.NO_COMP1], axis=0)
    assert not rest[:, g["cut"]].any()                                  # the second chunk opens inside a gap
    assert np.array_equal(np.isnan(mi.kalman_data(n, m)["gapped"]), ~mask)
    # the causality horizons: eligible for the staged emitter, below T_max, ragged against the observation block where an
    # eligible horizon can be
    assert all(ks.eligible(n, T) and T < g["t_max"] for T in g["causal"]) and g["t_min"] in g["causal"]
    assert any(T % g["ys"] for T in g["causal"]) == any(T % g["ys"] for T in g["horizons"][:-1])


def test_default_mask_is_unchanged_by_the_new_argument():
    for B, T, m in ((37, 19, 2), (5, 64, 4)):
        assert np.array_equal(kc.observed_mask(B, T, m), kc.observed_mask(B, T, m, wholly_missing_at=T // 2))
    assert not kc.observed_mask(6, 19, 2, wholly_missing_at=7)[0, 7].any()


@pytest.mark.parametrize("row", mi.GSF_REACHABLE, ids=GIDS)
def test_gaussian_sum_masks(row):
    for run in mi.GSF_RUNS:
        if run == "tv" and row[0] != mi.GENERIC:
            continue
        c = mi.gsf_case(row, run)
        r = mi.GSF_RUNS[run]
        assert c["mask"].shape == (r["B"], r["T"], row[2]) and c["init"].shape == (r["B"], c["K"], row[1])
        assert _patterns(c["mask"]) == set(range(2 ** row[2])), run
        _assert_fixed_trajectories(c["mask"])


@pytest.mark.parametrize("shape", mi.UKF_SHAPES, ids=mi.ukf_id)
def test_unscented_masks(shape):
    c = mi.ukf_case(shape, 3, False)
    assert _patterns(c["mask"]) == set(range(2 ** shape[2]))
    _assert_fixed_trajectories(c["mask"])
    po = c["po"]
    assert (po.dynamics_noise_covariance.shape[-1], po.emission_noise_covariance.shape[-1]) == (shape[1], shape[3])


# ---- headroom ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["const", "QR"])
@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_kalman_headroom(pair, variant):
    """The float32 oracle on the row-compacted model on trajectories 0-15 over T_max steps is within tol / 5 = 2e-6 of
    float64 on the four streams, the carry and the log-likelihood."""
    h = mi.kalman_headroom(*pair, variant)
    print(f"{mi.pair_id(pair)} {variant}: fp32 oracle vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in h.items()))
    for k, v in h.items():
        assert v <= mi.TOL / 5, (k, v)


def _assert_quarter(h, what):
    print(what, {k: f"{v:.2e}" for k, v in h.items()})
    for k, v in h.items():
        assert v <= mi.STANDARD[k] / 4, (what, k, v)


@pytest.mark.parametrize("row", mi.GSF_REACHABLE, ids=GIDS)
def test_gaussian_sum_headroom(row):
    """Every run of a row, on its first trajectories: the float32 reference within a quarter of the standard bound of float64,
    so that gsf_missing_cases.bounds hands out the standard bounds."""
    for run in mi.GSF_RUNS:
        if run == "tv" and row[0] != mi.GENERIC:
            continue
        bound, h = mi.gsf_bounds(row, run, CPU_NREF)
        _assert_quarter(h, f"{mi.gsf_id(row)} {run}")
        assert bound == mi.STANDARD


@pytest.mark.parametrize("tv", [False, True])
@pytest.mark.parametrize("K", mi.UKF_K)
@pytest.mark.parametrize("shape", mi.UKF_SHAPES, ids=mi.ukf_id)
def test_unscented_headroom(shape, K, tv):
    bound, h = mi.ukf_bounds(shape, K, tv, CPU_NREF)
    _assert_quarter(h, f"{mi.ukf_id(shape)} K={K} tv={tv}")
    assert bound == mi.STANDARD


# ---- what a wrong select would do to the reference ----------------------------------------------------------------------------
def _embedded_f64(a, ys, m0, P0, leak=None):
    """The kernel's m x m embedding of one trajectory's update in float64 (DESIGN.md 4a'): v and the rows of H P of a missing
    component selected to 0, its row and column of S those of the identity.  ``leak``: the component whose row of H P is NOT
    selected away -- one wrong select of one instance.  Returns (means (T, n), covariances (T, n, n))."""
    A, G, H, D = (np.asarray(a[k], np.float64) for k in ("A", "G", "H", "D"))
    Q, R, q0, r0 = (np.asarray(a[k], np.float64) for k in ("Q", "R", "q0", "r0"))
    m = H.shape[0]
    mp, Pp, means, covs = np.asarray(m0, np.float64), np.asarray(P0, np.float64), [], []
    for y in np.asarray(ys, np.float64):
        o = ~np.isnan(y)
        keep = o.copy()
        if leak is not None:
            keep[leak] = True
        X = np.where(keep[:, None], H @ Pp, 0.0)
        both = np.outer(o, o)
        S = np.where(both, D @ R @ D.T + H @ Pp @ H.T, np.eye(m))
        v = np.where(o, np.nan_to_num(y) - H @ mp - D @ r0, 0.0)
        K = np.linalg.solve(np.where(both, S + 1e-6, S), X).T
        mf, Pf = mp + K @ v, Pp - K @ S @ K.T
        means.append(mf)
        covs.append(Pf)
        mp, Pp = A @ mf + G @ q0, A @ Pf @ A.T + G @ Q @ G.T
    return np.stack(means), np.stack(covs)


@pytest.mark.parametrize("pair", mi.KALMAN, ids=KIDS)
def test_one_wrong_select_is_far_outside_the_tolerance(pair):
    """The embedding restated in float64 is the row-selected reference; with the right-hand sides of ONE missing component
    left in place (a select dropped in one instance) the filtered covariances of a gapped trajectory move by >= 100 tol, for
    every component of every pair: the gaps of these cases sit where such a mistake shows."""
    n, m = pair
    d, a = mi.kalman_data(n, m), mi.model(n, m)
    ref = mi.kalman_reference(n, m)
    for b in (0, kc.NO_COMP1):
        mu, P = _embedded_f64(a, d["gapped"][b], d["m0s"][b], d["P0s"][b])
        assert cm.rel_err(mu, ref["means"][b, 0]) < 1e-10 and cm.rel_err(P, ref["covariances"][b, 0]) < 1e-10
    for comp in range(m):
        _, P = _embedded_f64(a, d["gapped"][0], d["m0s"][0], d["P0s"][0], leak=comp)
        assert cm.rel_err(P, ref["covariances"][0, 0]) >= 100 * mi.TOL, comp
