"""The parallel-in-time Kalman filter with missing observations, without a GPU: the algebra of the per-pattern elements in
float64, the jitter gap between the two yardsticks of every GPU case, the pattern coverage of those cases, the host-built
pattern table (csrc/kf_pscan_patterns.hpp through tests/c/pscan_pattern_elements.cpp), what bf_kalman_filter_pscan_missing_f32
refuses before its first HIP call, the symbol, the header, the instance lists and the Python refusals."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import common as cm
from tests import kalman_missing_cases as kc
from tests import parallel_kalman_cases as pk
from tests import parallel_kalman_missing_cases as pm
from tests import test_parallel_kalman_cpu as plain

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "bayesianfiltering_amd", "csrc")
ALGEBRA_TOL = plain.ALGEBRA_TOL
F32 = np.float32


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-30))


# ---- the algebra ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1", "bias", "4x4"])
def test_pattern_elements_are_associative_and_prefixes_are_the_gapped_filter(name):
    T = 48
    a, ys, init, _ = pk.case(name, 1, T)
    m = ys.shape[2]
    yg = kc.gapped(ys, kc.observed_mask(1, T, m, seed=3))[0]
    yg[0] = ys[0, 0]                                     # step 0 observed: the prefixes start from its filtered state
    assert np.isnan(yg).all(axis=1).any() and np.isnan(yg).any(axis=1).sum() > 10
    els = [pm.element(a, yg[t]) for t in range(T)]
    for i in (1, 7, 20, 22, 40):                         # single steps and spans, around the wholly missing step T // 2 and in the tail
        x, y, z = els[i], pk.combine(els[i + 1], els[i + 2]), els[i + 3]
        left, right = pk.combine(pk.combine(x, y), z), pk.combine(x, pk.combine(y, z))
        for l, r in zip(left, right):
            assert _rel(l, r) <= ALGEBRA_TOL
    ms, Ps = pm.gapped_filter_f64(a, yg, init[0], a["P0"])
    prefix = els[1]
    for t in range(1, T):
        if t > 1:
            prefix = pk.combine(prefix, els[t])
        mt, Pt = pk.apply_span(prefix, ms[0], Ps[0])
        assert _rel(mt, ms[t]) <= ALGEBRA_TOL, t
        assert _rel(Pt, Ps[t]) <= ALGEBRA_TOL, t
    # nothing observed: the element is the prediction (A, u, Qb, 0, 0); everything observed: the plain element
    A, H, Qb, Rb, u, d = pk.terms(a)
    e = pm.element(a, np.full(m, np.nan))
    assert np.array_equal(e[0], A) and np.array_equal(e[1], u) and np.array_equal(e[2], Qb) and not e[3].any() and not e[4].any()
    for got, want in zip(pm.element(a, ys[0, 5]), pk.element(a, ys[0, 5])):
        assert _rel(got, want) <= ALGEBRA_TOL


def test_with_one_block_the_scheme_is_the_contract():
    c = pm.case("4x2", 37, 64)
    for key in pm.STREAMS:
        assert np.array_equal(c["scheme"][key], c["contract"][key]), key


# ---- the GPU cases: jitter gap and coverage --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,block", pm.SHAPES)
@pytest.mark.parametrize("name", pm.MODELS)
def test_jitter_gap_of_every_gpu_case(name, T, block):
    """The scheme against the contract in float64: the two differ by the 1e-6 jitter of the folded steps.  The GPU test holds
    the product to (this gap + 1e-5) against the contract, so the gap itself must stay inside the standing tolerance."""
    gap = pm.jitter_gap(name, T, block)
    worst = max(v for g in gap.values() for v in g.values())
    print(f"jitter gap {name} T={T} block={block}: {worst:.2e}")
    assert worst <= pm.TOL, gap
    c = pm.case(name, T, block)
    assert np.all(c["contract"]["weights"] == 1.0) and np.all(c["scheme"]["weights"] == 1.0)
    for key in pm.STREAMS:
        assert np.isfinite(c["contract"][key]).all() and np.isfinite(c["scheme"][key]).all(), key


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_every_pattern_occurs_inside_a_middle_block(m):
    """For each shape with a middle block (blocks 1 ... NB - 2, the ones the fold builds from the table), the observation
    patterns of their steps; over the long shapes every one of the 2^m patterns must occur."""
    for T, block in [(301, 4), (1000, 64)]:
        mask = pm.mask_for(T, m)
        NB = -(-T // block)
        middle = mask[:, block:(NB - 1) * block]
        seen = set(np.unique((middle * (1 << np.arange(m))).sum(axis=2)).tolist())
        assert seen == set(range(1 << m)), (m, T, block, sorted(seen))
    b, t0, t1 = pm.LONG_GAP
    mask = pm.mask_for(301, m)
    assert not mask[b, t0:t1].any() and mask[b, t0 - 8:t0].any() and mask[b, t1:t1 + 8].any()
    rest = np.delete(mask, [kc.FULL, kc.NO_COMP1], axis=0)               # (the two trajectories with a fixed pattern)
    assert not rest[:, 150].any() and not rest[:, 0].any() and not rest[:, -kc.FORECAST:].any()
    assert mask[kc.FULL].all() and not mask[kc.NONE].any()


# ---- the host-built table -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path_factory.mktemp("pscan_patterns") / "pscan_pattern_elements"
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(HERE, "c", "host_shim"), "-I", CSRC,
                    os.path.join(HERE, "c", "pscan_pattern_elements.cpp"), "-o", str(exe)], check=True)
    return exe


def _table(exe, tmp_path, n, m, A, H, Qb, Rb):
    path = tmp_path / f"model_{n}_{m}.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([n, m], np.int32).tobytes())
        for x in (A, H, Qb, Rb):
            fh.write(np.ascontiguousarray(x, F32).tobytes())
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("n", range(1, 7))
@pytest.mark.parametrize("m", range(1, 5))
def test_host_table_matches_the_float64_elements(table_program, tmp_path, n, m):
    """Every entry of the table against the NumPy element of its pattern to fp32 rounding, every entry against the compacted
    model bit for bit (the program's own check, exit status 0), and entry 2^m - 1 against the plain route's constants bit for
    bit."""
    a = cm.random_stable_lgssm(n, m, seed=900 + 10 * n + m, bias=True)
    A, H, Qb, Rb, u, d = pk.terms(a)
    A32, H32, Qb32, Rb32 = (np.asarray(x, F32) for x in (A, H, Qb, Rb))     # what the launcher reads: fp32 model terms
    code, out, err = _table(table_program, tmp_path, n, m, A32, H32, Qb32, Rb32)
    assert code == 0, (code, err[-2000:])
    lines = [ln.split() for ln in out.strip().split("\n")]
    assert [ln[0] for ln in lines] == [str(p) for p in range(1 << m)] + ["plain"]
    rows = {ln[0]: np.array([float(x) for x in ln[1:]], F32) for ln in lines}
    for p in range(1 << m):
        obs = np.array([(p >> i) & 1 for i in range(m)], bool)
        # the float64 element from the same fp32 terms (Qb and Rb as the launcher rounds them)
        want = _element_from_terms(A32, H32, Qb32, Rb32, obs)
        got = rows[str(p)]
        assert got.size == 3 * n * n + 2 * n * m
        off = 0
        for i, w in enumerate(want):
            g = got[off:off + w.size].reshape(w.shape)
            off += w.size
            scale = max(np.max(np.abs(w)), 1e-30)
            assert np.max(np.abs(g - w)) <= 2.0 ** -23 * scale + 1e-12, (p, np.max(np.abs(g - w)), scale)
            if i >= 3:                                                      # K, W: zero columns for the missing components
                assert not g[:, ~obs].any()
    assert rows[str((1 << m) - 1)].tobytes() == rows["plain"].tobytes()


def _element_from_terms(A, H, Qb, Rb, obs):
    A, H, Qb, Rb = (np.asarray(x, np.float64) for x in (A, H, Qb, Rb))
    n, m = A.shape[0], H.shape[0]
    K, W = np.zeros((n, m)), np.zeros((n, m))
    if obs.any():
        Ho = H[obs]
        Si = np.linalg.inv(Ho @ Qb @ Ho.T + Rb[np.ix_(obs, obs)])
        K[:, obs], W[:, obs] = Qb @ Ho.T @ Si, A.T @ Ho.T @ Si
    IKH = np.eye(n) - K @ H
    Ce, Je = IKH @ Qb, W @ H @ A
    return IKH @ A, 0.5 * (Ce + Ce.T), 0.5 * (Je + Je.T), K, W


def test_host_table_refuses_a_singular_submatrix(table_program, tmp_path):
    n, m = 2, 2
    H = np.array([[1, 0], [0, 0]], F32)                   # row 1 observes nothing and has no noise: S_{1} = 0
    code, out, err = _table(table_program, tmp_path, n, m, 0.5 * np.eye(n), H, np.eye(n), np.diag([1.0, 0.0]))
    assert code == 2


# ---- C: refused before the first HIP call -----------------------------------------------------------------------------------
class Call(plain.Call):
    def run(self, lib, entry="bf_kalman_filter_pscan_missing_f32"):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        ws = self.workspace if self.pointers["workspace"] else None
        code = getattr(lib, entry)(ref("model"), ref("y"), self.B, self.T, ref("carry"), ref("out"), ws, self.workspace_bytes, None)
        return code, lib.bf_last_error().decode()


def _singular(c):
    zeros = np.zeros((3, 3), F32)
    c.keep.append(zeros)
    c.model.Q = zeros.ctypes.data_as(_lib._FP)
    c.model.R = zeros.ctypes.data_as(_lib._FP)


SINGULAR = "parallel kalman filter: S = H G Q G^T H^T + D R D^T is singular, the step element does not exist"
ROWS = plain.ROWS + [("singular-S", _singular, _lib.BF_EUNSUPPORTED, SINGULAR)]


@pytest.mark.parametrize("name,breaker,code,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusals_are_the_plain_entry_points_word_for_word(name, breaker, code, message):
    lib = _lib.load()
    got = []
    for entry in ("bf_kalman_filter_pscan_missing_f32", "bf_kalman_filter_pscan_f32"):
        call = Call()
        breaker(call)
        got.append(call.run(lib, entry))
    assert got[0] == got[1] == (code, message)


def test_refusals_come_in_the_same_order():
    """Two faults at once: the earlier check answers, from both entry points."""
    lib = _lib.load()
    for first, second in [(1, 6), (5, 9), (7, 13), (9, 11), (11, 13)]:
        got = []
        for entry in ("bf_kalman_filter_pscan_missing_f32", "bf_kalman_filter_pscan_f32"):
            call = Call()
            plain.ROWS[first][1](call)
            plain.ROWS[second][1](call)
            got.append(call.run(lib, entry))
        assert got[0] == got[1] and got[0][0] != 0, (first, second, got)


def test_block_option_is_honoured():
    """"pkf_block" reaches the new entry point: with block 4 the same call needs two blocks per trajectory."""
    lib = _lib.load()
    call = Call()
    call.workspace_bytes = 720           # enough for one block per trajectory (the default block 16), not for two
    assert lib.bf_set_call_option(b"pkf_block", 4) == 0
    code, text = call.run(lib)
    assert code == _lib.BF_EINVAL and "block=4 need 1440 bytes" in text, text


def test_symbol_and_header():
    hdr = open(os.path.join(ROOT, "include", "bayesfilt.h")).read()
    assert re.search(r"\bint bf_kalman_filter_pscan_missing_f32\(", hdr)
    assert _lib.SYMBOLS["bf_kalman_filter_pscan_missing_f32"] == _lib.SYMBOLS["bf_kalman_filter_pscan_f32"]
    assert hasattr(_lib.load(), "bf_kalman_filter_pscan_missing_f32")
    assert "#define BF_VERSION 210" in hdr
    assert "this header declares 50 entry points" in hdr
    for earlier in ("declares 49 entry points", "declares 48 entry points", "declares 46 entry points"):
        assert earlier in hdr
    assert "bf_kalman_filter_pscan_missing_f32" in re.search(r"bf_set_option changes.*?\*/", hdr, re.S).group(0)
    assert len(re.findall(r"^(?:int|int64_t|const char\*|void) bf_\w+\(", hdr, re.M)) == 50


# ---- the instance lists -----------------------------------------------------------------------------------------------------
def test_instance_lists_equal_the_plain_tables():
    total = []
    for g in "abcdef":                                          # slice by slice: the one list of (n, m) rows serves both builds
        rows, miss = cm.instance_rows(f"kf_pscan_group_{g}.hip"), cm.instance_rows(f"kf_pscan_group_{g}.hip", missing=True)
        assert rows and rows == miss, (g, rows, miss)
        total += miss
    assert sorted(total) == [(n, m) for n in range(1, 7) for m in range(1, 5)]
    cm.assert_slices_are_built_twice("kf_pscan", "abcdef", "launch_pscan_nm<N_, M_, BF_MISSING>", "kf_pscan.hip")
    mk = cm.read_csrc("Makefile")                               # max-ilp: the missing object of slice f, and no other
    assert re.findall(r"^(\S+): CXXFLAGS \+= .*max-ilp", mk, re.M) == ["kf_pscan_group_f.missing.o"]
    hpp = open(os.path.join(CSRC, "kf_pscan.hpp")).read()
    for name in ("ps_update", "ps_fold_body", "ps_emit_body", "kf_pscan_fold_kernel", "kf_pscan_emit_kernel", "launch_pscan_nm"):
        assert re.search(r"template <int N, int M, bool MISSING = false>\s*\n[^;{]*\b" + name + r"\(", hpp), name
    assert "hip" not in open(os.path.join(CSRC, "kf_pscan_patterns.hpp")).read().split("#pragma once")[1].lower()


# ---- Python: refused before the device ---------------------------------------------------------------------------------------
def test_python_refusals_need_no_gpu(monkeypatch):
    import bayesianfiltering_amd as bfa
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("the GPU side was loaded before the refusal"))
    a = pk.model("4x2")
    p = cm.product_params(a)
    Bn, T, m = 3, 6, 2
    ys = np.zeros((Bn, T, m), F32)
    for fn, args in ((bfa.parallel_kalman_filter, ()), (bfa.parallel_kalman_smoother, ()),
                     (bfa.parallel_kalman_posterior_sample, (2, None))):
        extra = dict(workspace=object()) if fn is not bfa.parallel_kalman_filter else {}   # (the wrappers size a workspace first)
        with pytest.raises(ValueError, match="missing must be None or 'nan'"):
            fn(p, ys, *args, missing="drop", **extra)
        with pytest.raises(ValueError, match="observed must be a bool mask"):
            fn(p, ys, *args, observed=np.ones((Bn, T), F32), **extra)
        for shape in ((T + 1,), (Bn, T + 1), (T, m + 1), (Bn, T, m, 1), (Bn,)):
            with pytest.raises(ValueError, match="observed must have shape"):
                fn(p, ys, *args, observed=np.ones(shape, bool), **extra)
        with pytest.raises(ValueError, match="observed must have shape"):      # the batched forms need batched emissions
            fn(p, ys[0], *args, observed=np.ones((Bn, T), bool), **extra)
