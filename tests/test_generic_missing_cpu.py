"""Missing observations on the run-time-dimension kernel without a GPU: which entry point a gapped call takes, what
bf_kalman_filter_missing_anydim_f32 / bf_gsf_ekf_missing_anydim_f32 refuse before their first HIP call and in which order (through
ctypes, on host buffers no refused call reads), the companion header, and what the cases of tests/generic_missing_cases.py promise
the GPU tests: masks with every kind of step, benign float64 references, and a float32 reference close enough to its float64 copy
for the standard bounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from bayesianfiltering_amd.inference import _gapped_entry
from tests import generic_missing_cases as xc
from tests import gsf_missing_cases as gc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KF_OLD, KF_NEW = "bf_kalman_filter_missing_f32", "bf_kalman_filter_missing_anydim_f32"
GSF_OLD, GSF_NEW = "bf_gsf_ekf_missing_f32", "bf_gsf_ekf_missing_anydim_f32"


# ---- the entry-point choice -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n,m,dq,dr,source,options,want", [
    # Kalman: the register kernels keep n <= 8 with m <= min(n, 4)
    ("kalman", 1, 1, 1, 1, False, None, KF_OLD), ("kalman", 4, 2, 4, 2, False, None, KF_OLD), ("kalman", 8, 4, 8, 4, False, None, KF_OLD),
    ("kalman", 3, 3, 3, 3, False, {}, KF_OLD), ("kalman", 4, 2, 4, 2, False, {"kf_emit_mode": 2}, KF_OLD),
    ("kalman", 4, 2, 4, 2, False, {"force_generic": 0}, KF_OLD),
    ("kalman", 9, 2, 9, 2, False, None, KF_NEW), ("kalman", 6, 5, 6, 5, False, None, KF_NEW), ("kalman", 3, 6, 3, 6, False, None, KF_NEW),
    ("kalman", 2, 3, 2, 3, False, None, KF_NEW), ("kalman", 12, 4, 12, 4, False, None, KF_NEW), ("kalman", 33, 6, 33, 6, False, None, KF_NEW),
    ("kalman", 64, 32, 64, 32, False, None, KF_NEW), ("kalman", 4, 2, 4, 2, False, {"force_generic": 1}, KF_NEW),
    # Gaussian sum, registry functions: n <= 8 and m <= 4 stay (m > n included: the old entry point names what it lacks)
    ("gsf", 4, 2, 2, 2, False, None, GSF_OLD), ("gsf", 8, 4, 8, 4, False, None, GSF_OLD), ("gsf", 2, 3, 2, 3, False, None, GSF_OLD),
    ("gsf", 2, 2, 2, 2, False, {"gsf_structured": 1}, GSF_OLD),
    ("gsf", 9, 2, 9, 2, False, None, GSF_NEW), ("gsf", 8, 5, 8, 5, False, None, GSF_NEW), ("gsf", 12, 6, 12, 6, False, None, GSF_NEW),
    ("gsf", 9, 9, 9, 9, False, None, GSF_NEW), ("gsf", 4, 2, 2, 2, False, {"force_generic": 1}, GSF_NEW),
    # ... from source or recorded: every dimension <= 8 stays (m up to 8, unlike the registry's 4)
    ("gsf", 4, 2, 2, 2, True, None, GSF_OLD), ("gsf", 8, 8, 8, 8, True, None, GSF_OLD), ("gsf", 3, 5, 3, 5, True, None, GSF_OLD),
    ("gsf", 9, 2, 9, 2, True, None, GSF_NEW), ("gsf", 4, 2, 9, 2, True, None, GSF_NEW), ("gsf", 4, 2, 2, 9, True, None, GSF_NEW),
    ("gsf", 8, 9, 8, 9, True, None, GSF_NEW), ("gsf", 12, 6, 12, 6, True, None, GSF_NEW), ("gsf", 4, 2, 2, 2, True, {"force_generic": 1}, GSF_NEW),
])
def test_entry_point_choice(family, n, m, dq, dr, source, options, want):
    assert _gapped_entry(family, n, m, dq, dr, source, options) == want
    assert want in _lib.SYMBOLS


def test_entry_point_choice_refuses_an_unknown_family():
    with pytest.raises(ValueError, match="unknown filter family"):
        _gapped_entry("ukf", 4, 2, 4, 2)


# ---- C: refused before the first HIP call, and in this order ------------------------------------------------------------------
class _Call:
    """A valid call of one of the two entry points on small host buffers that no refused call reads."""

    def __init__(self, kalman, n=9, m=2):
        self.keep = keep = []
        self.kalman = kalman

        def fp(x):
            keep.append(np.ascontiguousarray(x, F32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def buf():
            keep.append(np.zeros(4096, F32))
            return keep[-1].ctypes.data

        self.B, self.T, self.K = 4, 8, 1 if kalman else 2
        if kalman:
            p = self.model = _lib.bf_lgssm()
            p.n, p.dq, p.m, p.dr = n, n, m, m
            p.A, p.H, p.Q, p.R = fp(np.eye(n)), fp(np.zeros((m, n))), fp(np.eye(n)), fp(np.eye(m))
            p.Q_steps, p.R_steps = 1, 1
        else:
            p = self.model = _lib.bf_model()
            p.dyn_id, p.emi_id, p.n, p.dq, p.m, p.dr = 0, 0, n, n, m, m                  # linear registry functions
            th_d, th_e = np.zeros(2 * n * n, F32), np.zeros(m * n + m * m, F32)
            p.dyn_theta, p.n_dyn_theta, p.emi_theta, p.n_emi_theta = fp(th_d), th_d.size, fp(th_e), th_e.size
            p.q0, p.r0, p.Q, p.R = fp(np.zeros(n)), fp(np.zeros(m)), fp(np.eye(n)), fp(np.eye(m))
            p.Q_steps, p.R_steps = 1, 1
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = buf(), self.T * m, m, 1
        self.u = _lib.bf_cstream()
        self.carry = _lib.bf_carry()
        self.carry.m_in, self.carry.P_in = buf(), buf()
        self.out = _lib.bf_out_desc()
        self.null = set()

    def collapsed(self):
        self.out.coll_mean.ptr = self.keep[0].ctypes.data
        return self

    def run(self, lib):
        ref = lambda name: None if name in self.null else C.byref(getattr(self, name))
        if self.kalman:
            code = lib.bf_kalman_filter_missing_anydim_f32(ref("model"), ref("y"), self.B, self.T, ref("carry"), ref("out"), None)
        else:
            code = lib.bf_gsf_ekf_missing_anydim_f32(ref("model"), ref("y"), ref("u"), self.B, self.T, self.K, ref("carry"), ref("out"), None)
        return code, lib.bf_last_error().decode()


def _lp_only_handle(lib, n, m):
    """A handle that carries only a log-density: nothing is compiled for it before the first particle-filter call."""
    h = C.c_void_p()
    src = b"template <class T> __device__ T log_prob(const T* x, const float* y, T u, const float* theta) { return x[0] * 0.0f; }\n"
    assert lib.bf_user_model_create_lp(None, None, src, n, n, m, m, C.byref(h)) == _lib.BF_OK, lib.bf_last_error().decode()
    return h.value


BIG = (64, 64)      # P and the update's ten tiles at pitch 68: 191 KiB of LDS


@pytest.mark.parametrize("kalman", [True, False])
def test_c_refusals_and_their_order(kalman):
    lib = _lib.load()
    UNSUP, EINVAL = _lib.BF_EUNSUPPORTED, _lib.BF_EINVAL
    # 1. NULL arguments and non-positive sizes, before anything else that is wrong with the call
    for name in ("model", "y", "carry", "out"):
        c = _Call(kalman, *BIG).collapsed() if name != "out" else _Call(kalman, *BIG)
        c.null.add(name)
        code, msg = c.run(lib)
        assert code == EINVAL and "NULL argument" in msg, (name, code, msg)
    for field, value in (("B", 0), ("B", -3), ("T", 0), ("T", -1)) + (() if kalman else (("K", 0), ("K", -2))):
        c = _Call(kalman, *BIG).collapsed()
        setattr(c, field, value)
        code, msg = c.run(lib)
        assert code == EINVAL and "must be positive" in msg, (field, value, code, msg)
    c = _Call(kalman).collapsed()
    c.y.ptr = None
    assert c.run(lib) == (EINVAL, "observations pointer is NULL")
    # 2. collapsed streams, before the flags, the handle and the capacity
    c = _Call(kalman, *BIG).collapsed()
    if not kalman:
        c.model.flags = 1
        c.model.user = _lp_only_handle(lib, *BIG)
    code, msg = c.run(lib)
    assert code == UNSUP and "collapsed streams" in msg, (code, msg)
    if not kalman:
        # 3. the legacy flags, before the handle and the capacity
        for flags in (1, 2, 4):
            c = _Call(kalman, *BIG)
            c.model.flags = flags
            c.model.user = _lp_only_handle(lib, *BIG)
            code, msg = c.run(lib)
            assert code == UNSUP and "flags != 0" in msg, (flags, code, msg)
        # 4. a handle that carries only a log-density, before the capacity
        c = _Call(kalman, *BIG)
        c.model.user = _lp_only_handle(lib, *BIG)
        code, msg = c.run(lib)
        assert code == EINVAL and "only a log-density" in msg, (code, msg)
    # 5. the LDS capacity, by name
    code, msg = _Call(kalman, *BIG).run(lib)
    assert code == UNSUP and "bytes of LDS" in msg and "160 KiB" in msg and "n = 64, m = 64" in msg, (code, msg)
    # "force_generic" is what these entry points are: armed or not, the same answer; and the override is consumed by the call
    assert lib.bf_set_call_option(b"force_generic", 1) == _lib.BF_OK
    code, msg = _Call(kalman, *BIG).run(lib)
    assert code == UNSUP and "bytes of LDS" in msg, (code, msg)


def test_the_old_entry_points_refuse_what_they_refused():
    """(9, 2), (12, 4), (8, 5), (64, 32) on bf_kalman_filter_missing_f32: word for word as before."""
    lib = _lib.load()
    for n, m in ((9, 2), (12, 4), (8, 5), (64, 32)):
        c = _Call(True, n, m)
        code = lib.bf_kalman_filter_missing_f32(C.byref(c.model), C.byref(c.y), c.B, c.T, C.byref(c.carry), C.byref(c.out), None)
        assert code == _lib.BF_EUNSUPPORTED
        assert lib.bf_last_error().decode() == f"kalman filter with missing observations: n <= 8 and m <= 4 only (n={n}, m={m})"


# ---- the companion header ---------------------------------------------------------------------------------------------------
def test_symbols_and_headers():
    ext = open(os.path.join(ROOT, "include", "bayesfilt_ext.h")).read()
    hdr = open(os.path.join(ROOT, "include", "bayesfilt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext, flags=re.S)
    assert sorted(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", code))) == sorted([KF_NEW, GSF_NEW])
    assert '#include "bayesfilt.h"' in code and "BF_VERSION" not in code and "extern \"C\"" in code
    assert "Why a second header" in ext
    for name, twin in ((KF_NEW, "bf_kalman_filter_f32"), (GSF_NEW, "bf_gsf_ekf_f32")):
        assert re.search(rf"\bint {name}\(", code), name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[twin]
        assert hasattr(_lib.load(), name)
        assert name not in hdr
    # bayesfilt.h is as it was: version, its count of declarations, the two register entry points
    assert "#define BF_VERSION 210" in hdr and _lib.HEADER_VERSION == 210 and _lib.load().bf_version() == 210
    assert "this header declares 50 entry points" in hdr and "declares 51" not in hdr
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert len(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", plain))) == 50
    assert "bayesfilt_ext" not in hdr


def test_the_headers_compile_as_c99(tmp_path):
    import subprocess
    src = tmp_path / "ext.c"
    src.write_text('#include "bayesfilt_ext.h"\n'
                   "typedef int (*kf_fn)(const bf_lgssm*, const bf_cstream*, int64_t, int64_t, const bf_carry*, const bf_out_desc*, void*);\n"
                   "typedef int (*gsf_fn)(const bf_model*, const bf_cstream*, const bf_cstream*, int64_t, int64_t, int32_t, const bf_carry*,\n"
                   "                      const bf_out_desc*, void*);\n"
                   "kf_fn new_kf = bf_kalman_filter_missing_anydim_f32, old_kf = bf_kalman_filter_missing_f32;\n"
                   "gsf_fn new_gsf = bf_gsf_ekf_missing_anydim_f32, old_gsf = bf_gsf_ekf_missing_f32;\n"
                   "int version = BF_VERSION;\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "ext.o")], check=True)


def test_the_plain_kernels_keep_their_translation_unit():
    """The MISSING = true instances are built in a file of their own; generic_scan.hip names none."""
    from tests import common as cm
    assert "gsf_generic_kernel<NT, true>" in cm.read_csrc("generic_scan_missing.hip")
    plain = cm.read_csrc("generic_scan.hip")
    assert "gsf_generic_kernel<64>" in plain and "gsf_generic_kernel<256>" in plain and ", true>" not in plain
    assert "generic_scan_missing.hip" in cm.read_csrc("Makefile")


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("n,m", xc.KALMAN_SHAPES)
def test_kalman_cases_are_benign_and_hold_every_kind_of_step(n, m, B):
    c = xc.kalman_case(n, m, B, xc.T)
    assert xc.mask_has_every_kind_of_step(c["mask"]), (n, m, B)
    ref = c["ref"]
    for k in ("means", "covariances", "predicted_means", "predicted_covariances", "loglik", "smoothed_means", "smoothed_covariances"):
        assert np.isfinite(ref[k]).all(), k
    biggest = max(float(np.abs(ref[k]).max()) for k in ("covariances", "predicted_covariances"))
    print((n, m, B), f"max |P| = {biggest:.2f}")
    assert biggest <= 16.0


@pytest.mark.parametrize("name", ["l96", "sv"])
def test_gsf_cases_keep_the_standard_bounds(name):
    """Four times the float32 reference's distance from its float64 copy stays below the standard tolerances: the bounds of the
    GPU tests are 1e-5 (streams) and 2e-5 (weights), and the cap of 2e-4 is not touched."""
    c = xc.gsf_case(name)
    assert xc.mask_has_every_kind_of_step(c["mask"]), name
    bound, h = xc.gsf_bounds(name)
    print(name, {k: f"{v:.2e}" for k, v in h.items()})
    assert all(np.isfinite(c["ref"][k]).all() for k in gc.STREAMS + ("loglik",))
    for k, v in bound.items():
        assert v == (gc.WTOL if k == "weights" else gc.TOL), (k, v, h[k])


def test_the_leak_case_really_holds_a_non_finite_missing_row():
    """svleak: the last component starts at 1e3, exp(x / sigma) overflows in float32, and that row's value and Jacobians are not
    finite while every other row's are; the component is coupled to nothing, so nothing finite depends on it."""
    po, _, u, _ = xc.gsf_model("svleak")
    n = 9
    x = np.zeros(n, F32)
    x[n - 1] = 1e3
    with np.errstate(all="ignore"):
        for u0 in (0.0, 1.0):
            uu = np.array([u0], F32)
            val = np.asarray(po.emission_function.value(x, np.asarray(po.emission_noise_bias, F32), uu))
            assert not np.isfinite(val[n - 1]) and np.isfinite(val[:n - 1]).all(), (u0, val)
    Phi = np.asarray(po.dynamics_function.value(np.eye(n, dtype=F32)[n - 1], np.zeros(n, F32), np.zeros(1, F32)))
    assert Phi[n - 1] == 1.0 and (Phi[:n - 1] == 0).all()
    R = np.asarray(po.emission_noise_covariance)
    assert (R[n - 1, :n - 1] == 0).all() and (R[:n - 1, n - 1] == 0).all()
