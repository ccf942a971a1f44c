"""The missing-observation Kalman route without a GPU: the float64 reference of tests/kalman_missing_cases.py against the
oracle's recursion and against itself on the row-reduced model, what bf_kalman_filter_missing_f32 refuses before its first
HIP call (through ctypes, on host buffers nothing reads), and the Python front: the ``observed=`` mask."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import common as cm
from tests import kalman_missing_cases as kc

F32, F64 = np.float32, np.float64


# ---- the reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", kc.SHAPES)
def test_reference_with_everything_observed_is_the_oracles_recursion(n, m):
    """The oracle runs the reference's float32 arithmetic; 1e-5 (2e-5 for the log-likelihood) is what the product is held to
    against it (tests/test_kalman_gpu.py) and bounds the oracle's own rounding over these 24 steps."""
    a = kc.model(n, m)
    B, T = 3, 24
    ys = cm.simulate_batch(a, B, T, seed=3)
    init = np.tile(a["m0"], (B, 1))
    ref = kc.batch_reference(a, ys, init)
    orc = cm.oracle_kalman_batch(a, ys, init)
    for k in kc.STREAMS:
        assert ref[k].shape == orc[k].shape
        assert cm.rel_err(orc[k], ref[k]) < 1e-5, k
    assert cm.rel_err(orc["loglik"], ref["loglik"]) < 2e-5
    assert np.array_equal(ref["carry"][1][:, 0], ref["predicted_means"][:, 0, -1])


def test_reference_wholly_missing_step_is_predict_only():
    a = kc.model(4, 2)
    T, t0 = 12, 5
    ys = cm.simulate_batch(a, 1, T, seed=3)[0]
    ys[t0] = np.nan
    r = kc.kalman_missing_f64(a, ys, a["m0"], a["P0"])
    assert np.array_equal(r["means"][t0], r["predicted_means"][t0 - 1])
    assert np.array_equal(r["covariances"][t0], r["predicted_covariances"][t0 - 1])
    assert r["loglik"][t0] == 0.0 and r["weights"][t0] == 1.0
    A, G = a["A"].astype(F64), a["G"].astype(F64)
    assert np.allclose(r["predicted_means"][t0], A @ r["means"][t0] + G @ a["q0"], rtol=1e-14, atol=0)
    assert np.isfinite(r["means"]).all() and (r["loglik"][np.arange(T) != t0] != 0.0).all()


@pytest.mark.parametrize("n,m,drop", [(4, 2, 1), (3, 3, 0), (8, 4, 2)])
def test_reference_constant_pattern_is_the_row_reduced_model(n, m, drop):
    """A component that is never observed: the same numbers as the complete-data recursion on the model without that row
    (float64 both ways; only the order of BLAS sums may differ)."""
    a = kc.model(n, m)
    T = 20
    ys = cm.simulate_batch(a, 1, T, seed=3)[0]
    keep = [i for i in range(m) if i != drop]
    yg = ys.copy()
    yg[:, drop] = np.nan
    got = kc.kalman_missing_f64(a, yg, a["m0"], a["P0"])
    red = kc.kalman_missing_f64(kc.row_reduced(a, keep), ys[:, keep], a["m0"], a["P0"])
    for k in kc.STREAMS + ("loglik",):
        assert np.allclose(got[k], red[k], rtol=1e-12, atol=1e-14), k


def test_patterns_hold_what_they_promise():
    B, T, m = 37, 19, 2
    mask = kc.observed_mask(B, T, m)
    assert mask[kc.FULL].all() and not mask[kc.NONE].any()
    assert not mask[kc.NO_COMP1][:, 1].any() and mask[kc.NO_COMP1][:, 0].all()
    rest = np.delete(mask, [kc.FULL, kc.NONE, kc.NO_COMP1], axis=0)
    assert not rest[:, 0].any() and not rest[:, T // 2].any() and not rest[:, T - kc.FORECAST:].any()
    inner = np.delete(rest[:, 1:T - kc.FORECAST], T // 2 - 1, axis=1)
    assert 0.2 < 1.0 - inner.mean() < 0.4
    assert ((inner.sum(axis=2) == 1).any() and (inner.sum(axis=2) == 2).any())     # partly and fully observed steps


# ---- the device arithmetic, built for the host ---------------------------------------------------------------------------------
def test_embedded_step_is_the_reduced_step_bit_for_bit(tmp_path):
    """csrc/kf_math.hpp compiled by the host compiler (tests/c/host_shim stands in for the HIP header): condition_on_masked on
    all 2^m patterns, m <= 4, random models, against condition_on on the compacted model.  Every mean, covariance entry and log-likelihood must have the same bits; nothing observed must leave
    m and P unchanged with log-likelihood 0."""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = shutil.which("g++") or shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = tmp_path / "embedding"
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(here, "c", "host_shim"), "-I", os.path.join(os.path.dirname(here), "bayesianfiltering_amd", "csrc"),
                    os.path.join(here, "c", "kalman_missing_embedding.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "total mismatches: 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- the C entry point's refusals ---------------------------------------------------------------------------------------------
class _Call:
    """A valid call of bf_kalman_filter_missing_f32 on small host buffers that no refused call reads."""

    def __init__(self, n=4, m=2):
        self.keep = keep = []

        def fp(x):
            keep.append(np.ascontiguousarray(x, F32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def buf():
            keep.append(np.zeros(4096, F32))
            return keep[-1].ctypes.data

        B, T = 4, 8
        p = self.model = _lib.bf_lgssm()
        p.n, p.dq, p.m, p.dr = n, n, m, m
        p.A, p.H, p.Q, p.R = fp(0.5 * np.eye(n)), fp(np.eye(m, n)), fp(np.eye(n)), fp(np.eye(m))
        p.Q_steps, p.R_steps = 1, 1
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = buf(), T * m, m, 1
        self.carry = _lib.bf_carry()
        self.carry.m_in, self.carry.P_in = buf(), buf()
        self.out = _lib.bf_out_desc()
        self.out.means.ptr, self.out.means.sB, self.out.means.sK, self.out.means.sT, self.out.means.sE = buf(), T * n, T * n, n, 1
        self.B, self.T = B, T
        self.null = set()

    def run(self, lib):
        ref = lambda name: None if name in self.null else C.byref(getattr(self, name))
        code = lib.bf_kalman_filter_missing_f32(ref("model"), ref("y"), self.B, self.T, ref("carry"), ref("out"), None)
        return code, lib.bf_last_error().decode()


def test_c_refusals_precede_the_first_hip_call():
    lib = _lib.load()
    UNSUP, EINVAL = _lib.BF_EUNSUPPORTED, _lib.BF_EINVAL
    # dimensions beyond the register kernels: the message names the limit
    for n, m in ((9, 2), (12, 4), (8, 5), (64, 32)):
        code, msg = _Call(n, m).run(lib)
        assert code == UNSUP and "n <= 8 and m <= 4" in msg, (n, m, code, msg)
    code, msg = _Call(2, 3).run(lib)                      # within the limits, not in the table (m > n)
    assert code == UNSUP and "not compiled in" in msg, (code, msg)
    # a lane count without a missing-data instance (the plain filter has (4, 2) at 1, 2 and 4 lanes; this route at 2 only)
    for lanes in (1, 4, 8):
        assert lib.bf_set_call_option(b"kf_lanes", lanes) == _lib.BF_OK
        code, msg = _Call(4, 2).run(lib)
        assert code == UNSUP and f"kf_lanes={lanes}" in msg, (lanes, code, msg)
    # collapsed streams
    for name in ("coll_mean", "coll_cov"):
        c = _Call()
        getattr(c.out, name).ptr = c.keep[0].ctypes.data
        code, msg = c.run(lib)
        assert code == UNSUP and "collapsed" in msg, (name, code, msg)
    # NULL arguments and sizes
    for name in ("model", "y", "carry", "out"):
        c = _Call()
        c.null.add(name)
        code, msg = c.run(lib)
        assert code == EINVAL and "NULL argument" in msg, (name, code, msg)
    for field, value in (("B", 0), ("B", -3), ("T", 0), ("T", -1)):
        c = _Call()
        setattr(c, field, value)
        code, msg = c.run(lib)
        assert code == EINVAL and "must be positive" in msg, (field, value, code, msg)
    c = _Call()
    c.y.ptr = None
    assert c.run(lib) == (EINVAL, "observations pointer is NULL")
    c = _Call()
    c.carry.P_in = None
    assert c.run(lib)[0] == EINVAL


def test_symbol_and_header():
    assert "bf_kalman_filter_missing_f32" in _lib.SYMBOLS
    assert _lib.SYMBOLS["bf_kalman_filter_missing_f32"] == _lib.SYMBOLS["bf_kalman_filter_f32"]
    assert hasattr(_lib.load(), "bf_kalman_filter_missing_f32")


# ---- the Python front ---------------------------------------------------------------------------------------------------------
def test_mask_shapes():
    from bayesianfiltering_amd import inference as inf
    B, T, m = 3, 6, 2
    rng = np.random.default_rng(0)
    for shape, as3 in (((T,), (1, T, 1)), ((B, T), (B, T, 1)), ((T, m), (1, T, m)), ((B, T, m), (B, T, m))):
        mk = rng.random(shape) > 0.4
        full = inf._observed_mask(mk, (B, T, m), m)
        assert full.shape == (B, T, m) and full.dtype == np.bool_
        assert np.array_equal(full, np.broadcast_to(mk.reshape(as3), (B, T, m)))
    for shape in ((T,), (T, m)):                                  # one trajectory: emissions (T, m)
        mk = rng.random(shape) > 0.4
        assert np.array_equal(inf._observed_mask(mk, (T, m), m), np.broadcast_to(mk.reshape(T, -1), (T, m)))
    for shape in ((T + 1,), (B,), (m,), (T, m + 1), (B, T + 1), (B + 1, T, m), (B, T, 1), (1, T, m), ()):
        with pytest.raises(ValueError, match="observed must have shape"):
            inf._observed_mask(np.ones(shape, bool), (B, T, m), m)
    with pytest.raises(ValueError, match="observed must have shape"):
        inf._observed_mask(np.ones((B, T), bool), (T, m), m)      # a batched mask for one trajectory
    with pytest.raises(ValueError, match="bool mask"):
        inf._observed_mask(np.ones((T,), np.float32), (B, T, m), m)


def test_python_refusals_need_no_gpu():
    """A mask that does not fit and an unknown ``missing`` are refused before the device is asked for."""
    import bayesianfiltering_amd as bfa
    a = kc.model(4, 2)
    p = cm.product_params(a)
    ys = np.zeros((3, 6, 2), F32)
    with pytest.raises(ValueError, match="observed must have shape"):
        bfa.kalman_filter(p, ys, observed=np.ones((5,), bool))
    with pytest.raises(ValueError, match="missing must be None or 'nan'"):
        bfa.kalman_filter(p, ys, missing="zero")
    with pytest.raises(ValueError, match="observed must have shape"):
        bfa.kalman_smoother(p, ys, observed=np.ones((3, 6, 3), bool))
    with pytest.raises(ValueError, match="observed must have shape"):
        bfa.kalman_posterior_sample(p, ys, 2, bfa.PRNGKey(0), observed=np.ones((2, 6), bool))


def test_mask_to_nan_leaves_the_input_untouched():
    import torch
    from bayesianfiltering_amd import inference as inf
    B, T, m = 3, 6, 2
    rng = np.random.default_rng(1)
    mk = rng.random((B, T)) > 0.4
    mask = inf._observed_mask(mk, (B, T, m), m)
    for ys in (rng.normal(size=(B, T, m)).astype(F32), torch.as_tensor(rng.normal(size=(B, T, m)).astype(F32))):
        before = np.asarray(ys).copy()
        out = inf._masked_emissions(ys, mask, "cpu")
        assert np.array_equal(np.asarray(ys), before)                         # the caller's data, bit for bit
        assert isinstance(out, torch.Tensor) and out.dtype == torch.float32
        if isinstance(ys, torch.Tensor):
            assert out.data_ptr() != ys.data_ptr()
        got = out.numpy()
        assert np.isnan(got[~mask]).all() and np.array_equal(got[mask], before[mask])
    # a mask that hides nothing still copies
    y = torch.zeros((B, T, m))
    assert inf._masked_emissions(y, np.ones((B, T, m), bool), "cpu").data_ptr() != y.data_ptr()
