"""Missing observations on the one-wave matrix-core kernel without a GPU: which entry point a gapped call takes
(``_gapped_route`` over ``_gapped_entry``), the third header, what bf_kalman_filter_missing_tiles_f32 /
bf_gsf_ekf_missing_tiles_f32 refuse before their first HIP call -- code for code and word for word what their anydim twins
refuse, in the same order --, where the MISSING instances are built, the float64 identity between the kernel's 32 x 32 embedding
and the reduced model of the contract, and what the cases of tests/matrix_missing_cases.py promise the GPU tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from bayesianfiltering_amd.inference import _gapped_entry, _gapped_route
from tests import common as cm
from tests import generic_missing_cases as xc
from tests import gsf_missing_cases as gc
from tests import kalman_missing_cases as kc
from tests import matrix_missing_cases as mc
from tests.test_generic_missing_cpu import _Call, _lp_only_handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KF_REG, KF_ANY, KF_TILES = "bf_kalman_filter_missing_f32", "bf_kalman_filter_missing_anydim_f32", "bf_kalman_filter_missing_tiles_f32"
GSF_REG, GSF_ANY, GSF_TILES = "bf_gsf_ekf_missing_f32", "bf_gsf_ekf_missing_anydim_f32", "bf_gsf_ekf_missing_tiles_f32"


# ---- the entry-point choice -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,options,want", [
    (KF_ANY, None, KF_TILES), (KF_ANY, {}, KF_TILES), (KF_ANY, {"force_generic": 0}, KF_TILES), (KF_ANY, {"kf_emit_mode": 2}, KF_TILES),
    (KF_ANY, {"force_generic": 1}, KF_ANY), (KF_ANY, {"force_generic": 1, "kf_lanes": 2}, KF_ANY),
    (GSF_ANY, None, GSF_TILES), (GSF_ANY, {"gsf_structured": 1}, GSF_TILES), (GSF_ANY, {"force_generic": 1}, GSF_ANY),
    # the register entry points, and anything else, pass through
    (KF_REG, None, KF_REG), (KF_REG, {"force_generic": 0}, KF_REG), (GSF_REG, None, GSF_REG), ("bf_ugsf_ukf_missing_f32", None, "bf_ugsf_ukf_missing_f32"),
])
def test_gapped_route(name, options, want):
    assert _gapped_route(name, options) == want
    assert want in _lib.SYMBOLS


@pytest.mark.parametrize("family,n,m,options,entry,route", [
    ("kalman", 16, 8, None, KF_ANY, KF_TILES), ("kalman", 32, 16, None, KF_ANY, KF_TILES), ("kalman", 9, 9, None, KF_ANY, KF_TILES),
    ("kalman", 33, 6, None, KF_ANY, KF_TILES),            # (the C entry point sends it on: tests/test_matrix_missing_gpu.py, test 7)
    ("kalman", 32, 16, {"force_generic": 1}, KF_ANY, KF_ANY), ("kalman", 4, 2, {"force_generic": 1}, KF_ANY, KF_ANY),
    ("kalman", 4, 2, None, KF_REG, KF_REG), ("kalman", 8, 4, None, KF_REG, KF_REG),
    ("gsf", 16, 8, None, GSF_ANY, GSF_TILES), ("gsf", 16, 8, {"force_generic": 1}, GSF_ANY, GSF_ANY), ("gsf", 4, 2, None, GSF_REG, GSF_REG),
])
def test_the_two_functions_together(family, n, m, options, entry, route):
    """``_gapped_entry`` is what it was (its own table: tests/test_generic_missing_cpu.py); the route is taken from its answer."""
    assert _gapped_entry(family, n, m, n, m, False, options) == entry
    assert _gapped_route(entry, options) == route


# ---- the third header ---------------------------------------------------------------------------------------------------------
def _declared(text):
    return sorted(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def test_symbols_and_headers():
    ext2 = open(os.path.join(ROOT, "include", "bayesfilt_ext2.h")).read()
    ext = open(os.path.join(ROOT, "include", "bayesfilt_ext.h")).read()
    hdr = open(os.path.join(ROOT, "include", "bayesfilt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", ext2, flags=re.S)
    assert _declared(ext2) == sorted([KF_TILES, GSF_TILES])
    assert '#include "bayesfilt_ext.h"' in code and "BF_VERSION" not in code and 'extern "C"' in code
    lib = _lib.load()
    for name, twin in ((KF_TILES, "bf_kalman_filter_f32"), (GSF_TILES, "bf_gsf_ekf_f32")):
        assert re.search(rf"\bint {name}\(", code), name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[twin]
        assert hasattr(lib, name)
        assert name not in hdr and name not in ext
    # the two older headers declare what they declared, and the version is what it was
    assert _declared(ext) == sorted([KF_ANY, GSF_ANY]) and "bayesfilt_ext2" not in ext and "bayesfilt_ext" not in hdr
    assert len(_declared(hdr)) == 50 and "this header declares 50 entry points" in hdr
    assert "#define BF_VERSION 210" in hdr and _lib.HEADER_VERSION == 210 and lib.bf_version() == 210
    assert len(_lib.SYMBOLS) == 54 and sorted(_lib.SYMBOLS) == sorted(_declared(hdr) + _declared(ext) + _declared(ext2))


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "ext2.c"
    src.write_text('#include "bayesfilt_ext2.h"\n'
                   "typedef int (*kf_fn)(const bf_lgssm*, const bf_cstream*, int64_t, int64_t, const bf_carry*, const bf_out_desc*, void*);\n"
                   "typedef int (*gsf_fn)(const bf_model*, const bf_cstream*, const bf_cstream*, int64_t, int64_t, int32_t, const bf_carry*,\n"
                   "                      const bf_out_desc*, void*);\n"
                   "kf_fn tiles_kf = bf_kalman_filter_missing_tiles_f32, any_kf = bf_kalman_filter_missing_anydim_f32, plain_kf = bf_kalman_filter_f32;\n"
                   "gsf_fn tiles_gsf = bf_gsf_ekf_missing_tiles_f32, any_gsf = bf_gsf_ekf_missing_anydim_f32, plain_gsf = bf_gsf_ekf_f32;\n"
                   "int version = BF_VERSION;\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "ext2.o")], check=True)


def test_the_plain_kernels_keep_their_translation_unit():
    """The MISSING = true instances are built in a file of their own; kf_scan_bf32.hip names none."""
    twins, plain, body = cm.read_csrc("kf_scan_bf32_missing.hip"), cm.read_csrc("kf_scan_bf32.hip"), cm.read_csrc("kf_scan_bf32.hpp")
    assert "bf32_launch_instance<true>" in twins and "bf32_launch_instance<false>" in plain
    assert "true>" not in plain and "MISSING" not in plain.replace("MISSING = true twins", "")
    assert "template <bool MULTI, bool TV, int DYN = 0, bool MISSING = false>" in body and "__global__" not in plain + twins
    assert len(re.findall(r"kf_scan_bf32_kernel<(?:true|false), (?:true|false), [012], MISSING>", body)) == 8
    mk = cm.read_csrc("Makefile")
    assert " kf_scan_bf32_missing.hip " in mk and " kf_scan_bf32.hpp " in mk and "../../include/bayesfilt_ext2.h" in mk
    assert "chol_w_rows_impl<32, true>" in body and "MISSING" not in cm.read_csrc("mfma_tiles.hpp")   # the factorization is untouched


# ---- C: refused before the first HIP call, like the anydim twins ------------------------------------------------------------------
def _both(lib, call):
    """The same call on the anydim entry point and on the tiles one: (code, text) of each."""
    ref = lambda name: None if name in call.null else C.byref(getattr(call, name))
    out = []
    for kf, gsf in ((KF_ANY, GSF_ANY), (KF_TILES, GSF_TILES)):
        if call.kalman:
            code = getattr(lib, kf)(ref("model"), ref("y"), call.B, call.T, ref("carry"), ref("out"), None)
        else:
            code = getattr(lib, gsf)(ref("model"), ref("y"), ref("u"), call.B, call.T, call.K, ref("carry"), ref("out"), None)
        out.append((code, lib.bf_last_error().decode()))
    return out


# shapes: beyond the LDS of the run-time-dimension kernel (no launch either way); the one-wave kernel's own (32, 16) and (16, 8)
BIG, TILES = (64, 64), ((32, 16), (16, 8))


@pytest.mark.parametrize("kalman", [True, False])
def test_c_refusals_are_the_anydim_twins(kalman):
    lib = _lib.load()
    UNSUP, EINVAL = _lib.BF_EUNSUPPORTED, _lib.BF_EINVAL
    calls = []                                                       # (label, call, code, text the message holds)
    for shape in (BIG,) + TILES:
        # 1. NULL arguments and non-positive sizes, before anything else that is wrong with the call
        for name in ("model", "y", "carry", "out"):
            c = _Call(kalman, *shape).collapsed() if name != "out" else _Call(kalman, *shape)
            c.null.add(name)
            calls.append((("null", name, shape), c, EINVAL, "NULL argument"))
        for field, value in (("B", 0), ("B", -3), ("T", 0), ("T", -1)) + (() if kalman else (("K", 0), ("K", -2))):
            c = _Call(kalman, *shape).collapsed()
            setattr(c, field, value)
            calls.append(((field, value, shape), c, EINVAL, "must be positive"))
        # 2. the model and the streams
        c = _Call(kalman, *shape).collapsed()
        c.y.ptr = None
        calls.append((("y.ptr", shape), c, EINVAL, "observations pointer is NULL"))
        c = _Call(kalman, *shape).collapsed()
        c.model.R = None
        calls.append((("R", shape), c, EINVAL, "R are required"))
        c = _Call(kalman, *shape).collapsed()
        c.carry.m_in = None
        calls.append((("carry.m_in", shape), c, EINVAL, "carry.m_in and carry.P_in are required"))
        # 3. collapsed streams, before the flags and the handle
        c = _Call(kalman, *shape).collapsed()
        if not kalman:
            c.model.flags = 1
            c.model.user = _lp_only_handle(lib, *shape)
        calls.append((("collapsed", shape), c, UNSUP, "collapsed streams"))
        if not kalman:
            # 4. the legacy flags, before the handle; 5. a handle that carries only a log-density
            for flags in (1, 2, 4):
                c = _Call(kalman, *shape)
                c.model.flags = flags
                c.model.user = _lp_only_handle(lib, *shape)
                calls.append((("flags", flags, shape), c, UNSUP, "flags != 0"))
            c = _Call(kalman, *shape)
            c.model.user = _lp_only_handle(lib, *shape)
            calls.append((("lp only", shape), c, EINVAL, "only a log-density"))
    # 6. outside the one-wave kernel: the LDS capacity of the run-time-dimension kernel, by name
    calls.append((("capacity",), _Call(kalman, *BIG), UNSUP, "bytes of LDS"))
    for label, c, code, text in calls:
        (ca, ma), (ct, mt) = _both(lib, c)
        assert (ca, ma) == (ct, mt), (label, (ca, ma), (ct, mt))
        assert ct == code and text in mt, (label, ct, mt)
    # "force_generic": the call is the anydim one, armed or not, and the override is consumed by the call
    assert lib.bf_set_call_option(b"force_generic", 1) == _lib.BF_OK
    assert _both(lib, _Call(kalman, *BIG))[1][0] == UNSUP


def test_a_table_count_the_one_wave_kernel_refuses_is_refused_before_any_hip_call():
    """Q_steps that is neither 1 nor T at (32, 16): BF_EINVAL from the launcher's own check, which stands before its first HIP
    call (the plain twin's answer to the same model)."""
    lib = _lib.load()
    c = _Call(True, 32, 16)
    c.model.Q_steps = 3
    plain = lib.bf_kalman_filter_f32(C.byref(c.model), C.byref(c.y), c.B, c.T, C.byref(c.carry), C.byref(c.out), None)
    text = lib.bf_last_error().decode()
    ct = lib.bf_kalman_filter_missing_tiles_f32(C.byref(c.model), C.byref(c.y), c.B, c.T, C.byref(c.carry), C.byref(c.out), None)
    mt = lib.bf_last_error().decode()
    assert ct == plain == _lib.BF_EINVAL and mt == text and "one matrix per step" in mt, (ct, mt)


# ---- the float64 identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", mc.KALMAN_SHAPES)
def test_the_embedding_is_the_reduced_model_in_float64(n, m):
    """The kernel's step restated in NumPy (unit rows for missing and padded components, the jitter on every entry of the 32 x 32
    system, W / g / z, the determinant-lemma log-likelihood, the 32 - |o| correction, the empty-step rule) against the contract
    reference, which really reduces the model: measured <= 1.7e-10 over means, covariances and log-likelihood at these shapes
    (the jitter between padded and observed rows changes the effective jitter by a relative ~1e-5 of 1e-6); the bound leaves
    50 x over that."""
    c = mc.kalman_case(n, m, 5)
    got, ref = mc.embedded_batch(c), c["ref"]
    e = {k: cm.rel_err(got[k], ref[k]) for k in kc.STREAMS + ("loglik",)}
    e.update({f"carry {i}": cm.rel_err(x, y) for i, (x, y) in enumerate(zip(got["carry"], ref["carry"]))})
    print((n, m), {k: f"{v:.1e}" for k, v in e.items()})
    assert max(e.values()) < 1e-8, e
    empty = ~c["mask"].any(axis=2)
    assert (got["loglik"][:, 0][empty] == 0.0).all() and (got["loglik"][:, 0][~empty] != 0.0).all()


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("n,m", mc.KALMAN_SHAPES)
def test_kalman_cases_are_benign_and_hold_every_kind_of_step(n, m, B):
    c = mc.kalman_case(n, m, B)
    assert xc.mask_has_every_kind_of_step(c["mask"]), (n, m, B)
    assert c["mask"][0, 2].all() and not c["mask"][0, mc.T // 2].any()
    for k in kc.STREAMS + ("loglik", "smoothed_means", "smoothed_covariances"):
        assert np.isfinite(c["ref"][k]).all(), k


@pytest.mark.parametrize("name", mc.GSF_CASES)
def test_gsf_cases_are_benign_and_hold_every_kind_of_step(name):
    c = mc.gsf_case(name)
    assert xc.mask_has_every_kind_of_step(c["mask"]), name
    assert all(np.isfinite(c["ref"][k]).all() for k in gc.STREAMS + ("loglik",))
    bound, h = mc.gsf_bounds(name)
    print(name, {k: f"{v:.2e}" for k, v in h.items()}, {k: f"{v:.1e}" for k, v in bound.items()})
    for k, v in bound.items():
        assert v <= gc.CAP and (name not in mc.LINEAR_GSF or v == (gc.WTOL if k in ("weights", "loglik") else gc.TOL)), (k, v)
