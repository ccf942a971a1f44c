"""The cases of tests/test_kalman_staged_gpu.py, no GPU: the instance list is the compiled table, the geometry the cases rely
on is what the header's formulas give, the horizon sweep reaches every remainder it claims, the batched float64 recursion is
heterogeneous_cases.kalman_f64, and on every instance the fp32 oracle is within a fifth of the asserted tolerance of float64
(the project's rule: the tolerance never moves, the inputs do)."""
import os
import re

import numpy as np
import pytest

from tests import common as cm
from tests import heterogeneous_cases as hc
from tests import kalman_staged_cases as ks

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesianfiltering_amd", "csrc")
IDS = [ks.case_id(i) for i in ks.INSTANCES]


def test_cases_are_the_compiled_instances():
    """One case per BF_CASE(n, m, lanes) of csrc/kf_group_{a,b,c,d}.hip, and the default lanes are launch_kf_group's."""
    compiled = set()
    for f in "abcd":
        with open(os.path.join(CSRC, f"kf_group_{f}.hip")) as fh:
            compiled |= {tuple(int(x) for x in mt.groups()) for mt in re.finditer(r"BF_CASE\((\d+), (\d+), (\d+)\);", fh.read())}
    cases = [(n, m, ks.geometry((n, m, opt))["lanes"]) for n, m, opt in ks.INSTANCES]
    assert len(cases) == len(set(cases)) == 28
    assert set(cases) == compiled
    with open(os.path.join(CSRC, "kf_scan_group.hip")) as fh:
        src = fh.read()
    assert "static int default_lanes(int n) { return n <= 2 ? 1 : (n <= 4 ? 2 : 4); }" in src
    assert "if (lanes == 0 && p->n >= 1 && p->n <= 8) lanes = default_lanes(p->n);" in src
    # per (n, m) the default is the only instance, except (4, 2), which has all three
    by_pair = {}
    for n, m, nl in compiled:
        by_pair.setdefault((n, m), set()).add(nl)
    assert all(v == ({1, 2, 4} if k == (4, 2) else {ks.default_lanes(k[0])}) for k, v in by_pair.items())


# ---- GroupCfg / Tile (csrc/kf_scan_group.hpp, csrc/scan_common.hpp) restated ---------------------------------------------
def _lcm4(e):
    return e if e % 4 == 0 else (2 * e if e % 2 == 0 else 4 * e)


def _row_floats(e, want):
    return -(-want // _lcm4(e)) * _lcm4(e)


def _group_cfg(n, m, nl, wsm_default=32):
    cpw, ep, wmin = 64 // nl, n * n, 4 * nl
    wp = _row_floats(ep, max(max(ep, 32), wmin))
    wsm = wsm_default if (nl >= 2 and n <= 4) else 16
    wm = _row_floats(n, max(max(n, wsm), wmin))
    ww = max(wsm, wmin)

    def tile(e, w, pad):
        ch = w // 4
        nchunk = cpw * ch
        return dict(ts=w // e, ch=ch, floats=cpw * (w + pad), iters=-(-nchunk // 64),
                    pow2=(ch & (ch - 1)) == 0 and nchunk >= 64 and nchunk % 64 == 0, gok=w % e == 0 and w % 4 == 0)
    ys = 1 if m >= 8 else 8 // m
    return dict(cpw=cpw, P=tile(ep, wp, 4), M=tile(n, wm, 4), W=tile(1, ww, 0 if nl == 1 else 4), ys=ys, ytile=cpw * ys * m,
                ybuf=-(-cpw * ys * m // 64) * 64)


def test_header_still_states_the_formulas_restated_here():
    """The lines of GroupCfg and Tile that _group_cfg restates: a change there must come back to this file."""
    with open(os.path.join(CSRC, "kf_scan_group.hpp")) as fh:
        hpp = fh.read()
    with open(os.path.join(CSRC, "scan_common.hpp")) as fh:
        common = fh.read()
    for line in ("static constexpr int CPW = 64 / NL;",
                 "static constexpr int lcm4(int e) { return e % 4 == 0 ? e : (e % 2 == 0 ? 2 * e : 4 * e); }",
                 "static constexpr int row_floats(int e, int want) { return ((want + lcm4(e) - 1) / lcm4(e)) * lcm4(e); }",
                 "static constexpr int WMIN = 4 * NL;",
                 "static constexpr int WP = row_floats(EP, (EP >= 32 ? EP : 32) > WMIN ? (EP >= 32 ? EP : 32) : WMIN);",
                 "#define BF_KF_WSM 32",
                 "static constexpr int WSM = (NL >= 2 && NS <= 4) ? BF_KF_WSM : 16;",
                 "static constexpr int WM = row_floats(NS, (NS >= WSM ? NS : WSM) > WMIN ? (NS >= WSM ? NS : WSM) : WMIN);",
                 "static constexpr int WW = WSM > WMIN ? WSM : WMIN;",
                 "using TP = Tile<EP, WP, CPW, 4>;", "using TM = Tile<NS, WM, CPW, 4>;",
                 "using TW = Tile<1, WW, CPW, (NL == 1 ? 0 : 4)>;",
                 "static constexpr int YS = (M >= 8) ? 1 : 8 / M;",
                 "auto row_ok = [&](const bf_stream& st, long long E) { return st.ptr == nullptr || (T * E) % 4 == 0; };",
                 "const long long b_main = (B / Cfg::CPW) * Cfg::CPW;"):
        assert line in hpp, line
    for line in ("static constexpr int TS = W / E;", "static constexpr int CH = W / 4;",
                 "static constexpr bool POW2 = ((CH & (CH - 1)) == 0) && (NCHUNK >= 64) && (NCHUNK % 64 == 0);"):
        assert line in common, line


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_geometry_table(inst):
    n, m, _ = inst
    g = ks.geometry(inst)
    cfg = _group_cfg(n, m, g["lanes"])
    assert g["cpw"] == cfg["cpw"] and g["B"] == 5 * cfg["cpw"] + 3
    assert g["depths"] == (cfg["P"]["ts"], cfg["M"]["ts"], cfg["W"]["ts"])
    assert g["ys"] == cfg["ys"] == {1: 8, 2: 4, 3: 2, 4: 2}[m]
    assert all(cfg[k]["gok"] for k in "PMW")                    # GroupCfg::STAGED_OK: every instance has staged tiles
    # all streams staged fit the 160 KiB of a workgroup of four waves (launch_nml: lds_ok), so forcing the emitter is not refused
    per_wave = 2 * cfg["ybuf"] + 2 * cfg["P"]["floats"] + 2 * cfg["M"]["floats"] + 2 * cfg["W"]["floats"]
    assert per_wave * 4 * 4 <= 160 * 1024
    # the counted wait: masked tiles (n = 3, 5, 6, 7) claim no younger stores; the masked observation DMA is m = 3 at 4 lanes
    assert all(cfg[k]["pow2"] for k in "PMW") == (n in (1, 2, 4, 8))
    assert (cfg["ytile"] % 64 != 0) == (m == 3 and g["lanes"] == 4)


def test_eligibility_rule():
    for n in range(1, 9):
        for T in range(1, 80):
            want = T % 4 == 0 if n % 2 else (T % 2 == 0 if n in (2, 6) else True)
            assert ks.eligible(n, T) == want, (n, T)


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_horizons_reach_what_the_sweep_claims(inst):
    n, m, _ = inst
    g = ks.geometry(inst)
    D, hz = max(g["depths"]), g["horizons"]
    assert 2 * D + g["ys"] + 1 <= g["t_max"] <= 76 and ks.eligible(n, g["t_max"])
    assert not any(ks.eligible(n, T) for T in range(2 * D + g["ys"] + 1, g["t_max"]))
    assert hz[-1] == g["t_max"] and hz[0] == g["t_min"] == {1: 4, 3: 4, 5: 4, 7: 4, 2: 2, 6: 2, 4: 1, 8: 1}[n]
    # the stream-subset runs: at least three observation blocks each, and one of them with the scalar streams staged
    assert g["subset_horizons"][0] == g["t_max"] and all(T in hz and T >= 3 * g["ys"] for T in g["subset_horizons"])
    assert any(T % 4 == 0 for T in g["subset_horizons"])
    assert len(g["subset_horizons"]) == (2 if g["t_max"] % 4 else 1) and (n % 2 == 0 or g["t_max"] % 4 == 0)
    # every remainder an eligible T can have against each tile depth and against the observation block, each with at least
    # one whole row (block) in front of it
    step = 4 if n % 2 else (2 if n in (2, 6) else 1)
    for period in g["depths"] + (g["ys"],):
        reach = {T % period for T in range(step, 8 * period * step + 1, step)}
        assert {T % period for T in hz if T > period} == reach, period
    if n % 2 == 0:
        assert any(T % 4 for T in hz) and any(T % 4 == 0 for T in hz)      # both routes of the scalar streams
    if n in (4, 8):
        assert hz[:3] == [1, 2, 3]
    # the chunk cut: aligned with nothing; both chunks staged wherever an eligible length can be unaligned (n = 3, 5, 7 have
    # a tile of depth 4, which divides every eligible length; at n = 6 a length is even, hence a multiple of YS = 2 at m = 3, 4)
    c = g["cut"]
    assert 0 < c < g["t_max"] and all(c % d for d in g["depths"] + (g["ys"],) if d > 1)
    assert (ks.eligible(n, c) and ks.eligible(n, g["t_max"] - c)) == (n not in (3, 5, 7) and (n, g["ys"]) != (6, 2))


@pytest.mark.parametrize("inst", [(3, 2, 0), (6, 4, 0), (8, 1, 0)], ids=ks.case_id)
def test_batched_float64_recursion_is_the_per_trajectory_one(inst):
    a = ks.model(inst)
    ys, m0s, P0s = (v[:5] for v in ks.data(inst))
    ref = hc.kalman_f64(a, ys, m0s, P0s)
    got = ks.kalman_f64_batched(a, ys, m0s, P0s)
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float64
        assert cm.rel_err(got[k], ref[k]) < 1e-12, k
    # per-step tables: constant tables change nothing
    T = ys.shape[1]
    const = ks.kalman_f64_batched(a, ys, m0s, P0s, np.broadcast_to(a["Q"], (T,) + a["Q"].shape), np.broadcast_to(a["R"], (T,) + a["R"].shape))
    assert all(np.array_equal(const[k], got[k]) for k in got)


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_a_table_read_one_step_late_is_far_outside_the_tolerance(inst):
    """Staged and strided kernels share the step that reads the per-step tables, so only the float64 comparison can tell a
    table row read at the wrong step: with Q_t (or R_t) taken from step max(t - 1, 0) the reference moves by >= 100 tol on
    every stream, and step 0, which reads row 0 either way, does not move."""
    a = ks.model(inst)
    ys, m0s, P0s = ks.data(inst)
    Qt, Rt = ks.tables(inst)
    tv = ks.reference_f64(inst, "QR")
    for name, late in (("Q", ks.kalman_f64_batched(a, ys, m0s, P0s, np.concatenate([Qt[:1], Qt[:-1]]), Rt)),
                       ("R", ks.kalman_f64_batched(a, ys, m0s, P0s, Qt, np.concatenate([Rt[:1], Rt[:-1]])))):
        for k in ks.STREAMS + ("loglik",):
            assert np.array_equal(late[k][:, :, 0], tv[k][:, :, 0]), (name, k)
            assert cm.rel_err(late[k], tv[k]) >= 100 * ks.TOL, (name, k)
    assert cm.rel_err(tv["covariances"], ks.reference_f64(inst)["covariances"]) >= 100 * ks.TOL     # and the tables are not constant


def test_fp32_oracle_with_constant_tables_is_the_plain_one():
    inst = (5, 3, 0)
    a = dict(ks.model(inst))
    ys, m0s, P0s = (v[:2] for v in ks.data(inst))
    T = ys.shape[1]
    plain = ks.kalman_numpy(a, ys, m0s, P0s)
    const = ks.kalman_numpy(a, ys, m0s, P0s, np.broadcast_to(a["Q"], (T,) + a["Q"].shape), np.broadcast_to(a["R"], (T,) + a["R"].shape))
    assert all(np.array_equal(plain[k], const[k]) for k in plain)


@pytest.mark.parametrize("variant", ("const",) + ks.TABLE_VARIANTS)
@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_reference_headroom(inst, variant):
    """The fp32 oracle on trajectories 0-15 over T_max steps is within tol / 5 = 2e-6 of float64 on the four streams, the carry
    and the log-likelihood, with constant covariances and with each combination of per-step tables the GPU test runs."""
    h = ks.headroom(inst, variant)
    print(f"{ks.case_id(inst)} {variant}: fp32 oracle vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in h.items()))
    cm.record(f"kalman_staged_headroom[{ks.case_id(inst)}-{variant}]", **h)
    for k in ks.STREAMS + ("loglik", "carry_means", "carry_covariances"):
        assert h[k] <= ks.TOL / 5, (k, h[k])


def test_priors_tell_trajectories_apart():
    """Distinct trajectories' filtered covariances differ by >= 100 tol at step 0 and still by >= 10 tol at step 3: a row
    stored in a neighbour's slot is far outside the tolerance (and the bitwise comparisons need no margin at all)."""
    for inst in ((3, 3, 0), (4, 2, 4), (8, 4, 0)):
        n = inst[0]
        P = ks.reference_f64(inst)["covariances"][:32, 0]
        assert hc.pairwise_min_rel_err(P[:, 0].reshape(-1, n, n)) >= 100 * ks.TOL, inst
        assert hc.pairwise_min_rel_err(P[:, 3].reshape(-1, n, n)) >= 10 * ks.TOL, inst
