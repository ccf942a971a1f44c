"""The missing-observation route of the bootstrap particle filter without a GPU: the masked oracle wrappers of
tests/particle_missing_cases.py against the plain oracle and the properties of their runs that the GPU tests rely on, the
device header csrc/bpf_missing.hpp built for the host against the compacted arithmetic, what ``missing=`` / ``observed=``
refuse in Python before the device is asked for, what bf_bpf_missing_f32 refuses before its first HIP call (through ctypes, on
host buffers nothing reads), the header, and the instance lists of the new translation units."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import particle_missing_cases as pmc
from tests import particle_route_cases as prc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianfiltering_amd", "csrc")


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


# ---- the masked oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["1x4", "1x8", "4x16-fixed"])
def test_masked_wrapper_on_complete_data_is_the_plain_oracle(cid):
    case = prc.BY_ID[cid]
    a = prc.arrays(case)
    ys = prc.observations(case, a)
    po = prc.oracle_params(case, a)
    kw = dict(key=prc.key_of(case), resampler=case.resampler, debug=True, arith="canonical")
    ref, dr = go.bootstrap_particle_filter(po, ys[0], case.N, **kw)
    got, dg = go.bootstrap_particle_filter(pmc.masked_oracle_params(po), ys[0], case.N, **kw)
    assert dr["resampled"].any()
    assert _bits_equal(got["weights"], ref["weights"]) and _bits_equal(got["particles"], ref["particles"])
    assert _bits_equal(dg["logz"], dr["logz"]) and _bits_equal(dg["ess"], dr["ess"])
    assert np.array_equal(dg["ancestors"], dr["ancestors"])


def test_masked_stochastic_volatility_wrapper_on_complete_data_is_the_plain_oracle():
    from oracle import models as om, threefry as otf
    po, arr, ys, u, key = pmc.sv_setup()
    n, T = arr["n"], pmc.SV_T
    hn = om.StochVol(n)
    plain = po._replace(emission_distribution_log_prob=go.StochVolEmissionLogProb(hn, arr["R"]))
    full = go.sample_ssm(go.ParamsNLSSM(*plain[:8]), otf.PRNGKey(21), T, u.reshape(T, 1))[1]
    kw = dict(key=key, inputs=u.reshape(T, 1), debug=True, arith="canonical")
    ref, dr = go.bootstrap_particle_filter(plain, full, 64, **kw)
    got, dg = go.bootstrap_particle_filter(po, full, 64, **kw)
    assert _bits_equal(got["weights"], ref["weights"]) and _bits_equal(got["particles"], ref["particles"])
    assert _bits_equal(dg["logz"], dr["logz"]) and np.array_equal(dg["ancestors"], dr["ancestors"])


def test_gap_pattern():
    B, T, m = 3, 6, 2
    ys = np.arange(B * T * m, dtype=F32).reshape(B, T, m)
    g = pmc.gapped(ys)
    miss = np.isnan(g)
    assert not np.isnan(ys).any()                          # a copy
    want = np.zeros((B, T, m), bool)
    want[:, 2, :] = True
    for b in range(B):
        want[b, 1, b % m] = want[b, 4, (b + 1) % m] = True
    want[B - 1, T - 1, :] = True
    assert np.array_equal(miss, want) and np.array_equal(g[~miss], ys[~miss])


@pytest.mark.parametrize("case", prc.CANONICAL, ids=[c.id for c in prc.CANONICAL])
def test_masked_oracle_runs_have_the_properties_the_gpu_tests_rely_on(case):
    """Every run finite; no draw inside a CDF inversion (bit comparison of ancestors is legitimate on the rows' own seeds); every
    row but 1x2 has steps that resample and steps that do not, 1x2 and trajectory 1 of 1x1 and of 16x16 never resample; a wholly
    missing step has logz within 2 ulp of 0, does not resample and leaves the previous weights renormalised."""
    res = []
    for b in prc.oracle_trajectories(case):
        out, dbg = pmc.oracle_run(case, b)
        assert np.isfinite(out["weights"]).all() and np.isfinite(out["particles"]).all() and np.isfinite(dbg["logz"]).all(), b
        assert not dbg["ambiguous"].any(), b
        res.append(dbg["resampled"])
        whole = [2] + ([case.T - 1] if b == case.B - 1 else [])
        for t in whole:
            assert abs(float(dbg["logz"][t])) <= 2 * np.finfo(F32).eps, (b, t, dbg["logz"][t])
            assert not dbg["resampled"][t], (b, t)
            prev = out["weights"][:, t - 1].astype(np.float64)
            assert np.max(np.abs(out["weights"][:, t] - prev / prev.sum())) <= 4 * np.finfo(F32).eps * prev.max(), (b, t)
    res = np.array(res)
    if case.id == "1x2":
        assert not res.any()
    else:
        assert 0 < res.sum() < res.size, res
    if case.id in ("1x1", "16x16"):
        assert not res[1].any() and res[0].any()


def test_masked_oracle_gap_to_float64_is_what_the_cases_module_records():
    """The figures the canonical logz bound of the GPU test is taken from (a cheap row; all of them were measured this way)."""
    case = prc.BY_ID["1x8"]
    a = prc.arrays(case)
    ys = pmc.gapped(prc.observations(case, a))
    worst = 0.0
    for b in prc.oracle_trajectories(case):
        out, dbg = pmc.oracle_run(case, b, 0.0)
        lz, _, _ = pmc.recompute_f64(a, out["particles"], out["weights"], ys[b])
        worst = max(worst, prc.logz_gap(dbg["logz"], lz))
    assert worst <= 1.05 * pmc.ORACLE_LOGZ_GAP[case.id] and pmc.ORACLE_LOGZ_GAP[case.id] <= 1.5 * worst, worst
    assert set(pmc.ORACLE_LOGZ_GAP) == {c.id for c in prc.CANONICAL}
    assert pmc.LOGZ_BOUND_CANONICAL == 10 * max(pmc.ORACLE_LOGZ_GAP.values())


def test_masked_stochastic_volatility_oracle_resamples_where_recorded():
    po, arr, ys, u, key = pmc.sv_setup()
    miss = np.isnan(ys)
    assert miss[list(pmc.SV_WHOLE)].all() and miss.sum() == 3 * len(pmc.SV_WHOLE) + len(pmc.SV_SINGLE) + 2 * len(pmc.SV_DOUBLE)
    for N, steps in pmc.SV_RESAMPLES.items():
        out, dbg = go.bootstrap_particle_filter(po, ys, N, key=key, inputs=u.reshape(-1, 1), debug=True, arith="canonical")
        assert tuple(np.flatnonzero(dbg["resampled"])) == steps, (N, dbg["resampled"])
        assert not dbg["ambiguous"].any() and np.isfinite(out["weights"]).all()


# ---- the device header on the host -------------------------------------------------------------------------------------------
def test_masked_density_is_the_compacted_density_bit_for_bit(tmp_path):
    """csrc/bpf_missing.hpp compiled by the host compiler (tests/c/host_shim stands in for the HIP header): every pattern of
    m <= 8 on random full R_lp, with and without the stochastic-volatility scale, against emission_loglik's arithmetic on the
    compacted problem; the embedded factor's observed block against the compacted factor, its missing rows against e_a."""
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "bpf_missing_density"
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "c", "host_shim"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "bpf_missing_density.cpp"), "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "total mismatches: 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert int(re.search(r"log-densities compared: (\d+)", r.stdout).group(1)) > 30000


def test_header_keeps_clear_of_the_kernels():
    """The header of the masked density includes nothing of the kernels (it is what the host program builds), and the flag
    reaches every body the issue of this change names."""
    text = open(os.path.join(CSRC, "bpf_missing.hpp")).read()
    assert re.findall(r'^#include "([^"]+)"', text, re.M) == ["bf_canon_math.hpp"]
    for word in ("update_dpp", "kernarg", "threadIdx"):
        assert word not in text, word
    for path, names in (("bpf_scan.hpp", ("bpf_scan_body", "bpf_scan_kernel", "launch_bpf_cfg", "launch_bpf_dims")),
                        ("bpf_big.hpp", ("propagate_particle", "bpf_big_body")), ("bpf_wide.hpp", ("wide_propagate_kernel", "launch_bpf_wide_dims"))):
        src = open(os.path.join(CSRC, path)).read()
        for name in names:
            assert re.search(r"template <[^>]*bool MISSING = false>\s*\n[^;{]*\b" + name + r"\(", src), (path, name)


# ---- Python: refused before the device ---------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    import bayesianfiltering_amd as bfa
    case = prc.BY_ID["1x4"]
    pp = prc.engine_params(case)
    B, T, m = 3, 6, 2
    ys = np.zeros((B, T, m), F32)
    with pytest.raises(ValueError, match="missing must be None or 'nan'"):
        bfa.bootstrap_particle_filter(pp, ys, 16, missing="drop")
    with pytest.raises(ValueError, match="observed must be a bool mask"):
        bfa.bootstrap_particle_filter(pp, ys, 16, observed=np.ones((B, T), F32))
    for shape in ((T + 1,), (B, T + 1), (T, m + 1), (B, T, m, 1), (B,)):
        with pytest.raises(ValueError, match="observed must have shape"):
            bfa.bootstrap_particle_filter(pp, ys, 16, observed=np.ones(shape, bool))
    with pytest.raises(ValueError, match="observed must have shape"):      # the batched forms need batched emissions
        bfa.bootstrap_particle_filter(pp, ys[0], 16, observed=np.ones((B, T), bool))
    nlssm = bfa.ParamsNLSSM(*pp[:8])
    for kw in (dict(missing="nan"), dict(observed=np.ones(T, bool)), {}):
        with pytest.raises(TypeError, match="params must be a ParamsBPF"):
            bfa.bootstrap_particle_filter(nlssm, ys, 16, **kw)
    with pytest.raises(ValueError, match="missing must be None or 'nan'"):
        bfa.bootstrap_particle_posterior_sample(pp, ys, 16, 2, np.array([0, 1], np.uint32), missing=1)


# ---- C: refused before the first HIP call ----------------------------------------------------------------------------------
class _Call:
    """A valid call of bf_bpf_missing_f32 (or of bf_bpf_f32) on small host buffers that no refused call reads."""

    def __init__(self, n=2, m=2):
        self.keep = keep = []

        def fp(x):
            keep.append(np.ascontiguousarray(x, F32))
            return keep[-1].ctypes.data_as(_lib._FP)

        self.B, self.T, self.N, self.resampler = 2, 6, 64, 0
        bm = self.model = _lib.bf_bpf_model()
        p = bm.ssm
        p.dyn_id, p.emi_id, p.n, p.dq, p.m, p.dr = 0, 0, n, n, m, m
        th_d, th_e = np.zeros(2 * n * n, F32), np.zeros(m * n + m * m, F32)
        p.dyn_theta, p.n_dyn_theta, p.emi_theta, p.n_emi_theta = fp(th_d), th_d.size, fp(th_e), th_e.size
        p.q0, p.r0, p.Q, p.R = fp(np.zeros(n)), fp(np.zeros(m)), fp(np.eye(n)), fp(np.eye(m))
        p.Q_steps, p.R_steps = 1, 1
        bm.m0, bm.P0, bm.lp_cov, bm.r_eval = fp(np.zeros(n)), fp(np.eye(n)), fp(np.eye(m)), fp(np.zeros(m))
        keep.append(np.zeros(4096, F32))
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = keep[-1].ctypes.data, self.T * m, m, 1
        self.u = _lib.bf_cstream()
        self.carry = _lib.bf_bpf_carry()
        self.out = _lib.bf_bpf_out()
        self.key = (C.c_uint32 * 2)(0, 1)
        self.null = set()

    def run(self, lib, entry="bf_bpf_missing_f32"):
        ref = lambda name: None if name in self.null else C.byref(getattr(self, name))
        code = getattr(lib, entry)(ref("model"), ref("y"), ref("u"), self.B, self.T, self.N, None if "key" in self.null else self.key,
                                   0.5, self.resampler, ref("carry"), ref("out"), None)
        return code, lib.bf_last_error().decode()


def test_c_refusals_precede_the_first_hip_call():
    """Every pre-launch refusal of bf_bpf_f32, word for word the same from bf_bpf_missing_f32."""
    lib = _lib.load()
    EINVAL = _lib.BF_EINVAL
    calls = []
    for name in ("model", "y", "out", "key"):
        calls.append((lambda c, name=name: c.null.add(name), "NULL argument"))
    for field, value in (("B", 0), ("B", -3), ("T", 0), ("T", -1), ("N", 0), ("N", -5)):
        calls.append((lambda c, f=field, v=value: setattr(c, f, v), "B, T and N must be positive"))
    calls.append((lambda c: setattr(c.y, "ptr", None), "observations pointer is NULL"))
    for field in ("m0", "P0", "lp_cov"):
        calls.append((lambda c, f=field: setattr(c.model, f, None), "Q, m0, P0, lp_cov are required"))
    calls.append((lambda c: setattr(c.model.ssm, "Q", None), "Q, m0, P0, lp_cov are required"))
    for r in (2, -1):
        calls.append((lambda c, r=r: setattr(c, "resampler", r), "resampler must be 0 (multinomial) or 1 (systematic)"))
    calls.append((lambda c: setattr(c.carry, "x_in", c.keep[-1].ctypes.data), "carry.x_in needs carry.w_in"))
    for breaker, words in calls:
        got = []
        for entry in ("bf_bpf_missing_f32", "bf_bpf_f32"):
            c = _Call()
            breaker(c)
            got.append(c.run(lib, entry))
        assert got[0] == got[1] and got[0][0] == EINVAL and words in got[0][1], (words, got)


def test_symbol_and_header():
    hdr = open(os.path.join(ROOT, "include", "bayesfilt.h")).read()
    assert re.search(r"\bint bf_bpf_missing_f32\(", hdr)
    assert _lib.SYMBOLS["bf_bpf_missing_f32"] == _lib.SYMBOLS["bf_bpf_f32"]
    assert hasattr(_lib.load(), "bf_bpf_missing_f32")
    assert "#define BF_VERSION 210" in hdr
    assert "this header declares 49 entry points" in hdr
    for earlier in ("declares 48 entry points", "declares 46 entry points"):
        assert earlier in hdr
    assert "bf_bpf_missing_f32" in re.search(r"bf_set_option changes.*?\*/", hdr, re.S).group(0)      # takes per-call options


# ---- the instance lists -----------------------------------------------------------------------------------------------------
def test_instance_lists_equal_the_plain_tables():
    total = 0
    for g in "abc":                                             # slice by slice: the one list of (n, dq, m) rows serves both builds
        plain, miss = cm.instance_rows(f"bpf_group_{g}.hip"), cm.instance_rows(f"bpf_group_{g}.hip", missing=True)
        assert plain and plain == miss, (g, plain, miss)
        total += len(miss)
    assert total == 12
    cm.assert_slices_are_built_twice("bpf", "abc", "launch_bpf_dims<N_, DQ_, M_, BF_MISSING>", "bpf_scan.hip")
    assert "run_groups(missing ? kMissingGroups : kPlainGroups," in cm.read_csrc("bpf_scan.hip")
    assert "bpf_missing.hpp" in cm.read_csrc("jit_embed.py")
