"""The missing-observation route of the Gaussian-sum filters without a GPU: the reference of tests/gsf_missing_cases.py against
the oracle and against its float64 copy, what ``missing=`` / ``observed=`` refuse in Python before the device is asked for, what
bf_gsf_ekf_missing_f32 / bf_ugsf_ukf_missing_f32 refuse before their first HIP call (through ctypes, on host buffers nothing
reads), the header, and the instance lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from oracle import gaussfilt_oracle as go
from tests import common as cm
from tests import gsf_missing_cases as gc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianfiltering_amd", "csrc")


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unscented", [False, True])
@pytest.mark.parametrize("name", ["bot", "l63", "sv", "l96"])
def test_reference_on_complete_data_is_the_oracle(name, unscented):
    """Every step observed: the wrapped emission returns all rows and the loop is the oracle's filter, bit for bit."""
    T, K = 12, 3
    po, _, u = gc.model(name, T)
    ys = gc.simulate(po, 1, T, u)[0]
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(1).normal(size=(K, po.initial_mean.size))).astype(F32)
    iu = None if u is None else u.reshape(T, 1)
    up = go.ParamsUKF(1.0, 0.0, 0.0) if unscented else None
    ref = gc.reference(po, ys, K, init, iu, up)
    if unscented:
        post, ll = go.unscented_gaussian_sum_filter(po, up, ys, K, inputs=iu, initial_means=init, return_ll=True)
    else:
        post, ll = go.gaussian_sum_filter(po, ys, K, inputs=iu, initial_means=init, return_ll=True)
    for k in gc.STREAMS:
        assert np.array_equal(ref[k], getattr(post, k)), k
    assert np.array_equal(ref["loglik"], ll)


@pytest.mark.parametrize("unscented", [False, True])
def test_reference_step_with_nothing_observed(unscented):
    """ll = 0, means and covariances pass untouched, the weights are renormalised only (K = 1: exactly 1); the predict runs."""
    T, K, t0 = 10, 3, 4
    po, _, u = gc.model("bot", T)
    ys = gc.simulate(po, 1, T, u)[0]
    ys[t0] = np.nan
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(1).normal(size=(K, 4))).astype(F32)
    up = go.ParamsUKF(1.0, 0.0, 0.0) if unscented else None
    r = gc.reference(po, ys, K, init, u.reshape(T, 1), up)
    assert np.array_equal(r["means"][:, t0], r["predicted_means"][:, t0 - 1])
    assert np.array_equal(r["covariances"][:, t0], r["predicted_covariances"][:, t0 - 1])
    assert (r["loglik"][:, t0] == 0).all() and (r["loglik"][:, np.arange(T) != t0] != 0).all()
    assert np.allclose(r["weights"][:, t0], r["weights"][:, t0 - 1], rtol=3e-7, atol=0)
    assert not np.array_equal(r["predicted_means"][:, t0], r["means"][:, t0])
    r1 = gc.reference(po, ys, 1, init[:1], u.reshape(T, 1), up)
    assert (r1["weights"] == 1).all()


def test_reference_fixed_pattern_is_the_reduced_model():
    """Bearing / range with the range never observed = the oracle's filter of the bearing-only model (R[0, 0] the same)."""
    T, K = 15, 3
    po, _, u = gc.model("bot", T)
    p1 = gc.model("bot1", T)[0]
    ys = gc.simulate(po, 1, T, u)[0]
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(1).normal(size=(K, 4))).astype(F32)
    yg = ys.copy()
    yg[:, 1] = np.nan
    ref = gc.reference(po, yg, K, init, u.reshape(T, 1))
    red, ll = go.gaussian_sum_filter(p1, ys[:, :1], K, inputs=u.reshape(T, 1), initial_means=init, return_ll=True)
    for k in gc.STREAMS:
        assert np.array_equal(ref[k], getattr(red, k)), k
    assert np.array_equal(ref["loglik"], ll)


@pytest.mark.parametrize("name,B,T,K,unscented", [("l63", 3, 64, 1, False), ("l96", 3, 64, 1, False), ("bot", 3, 64, 1, False),
                                                  ("sv", 3, 64, 1, False), ("l96", 3, 19, 3, True), ("bot", 3, 19, 3, True)])
def test_headroom_stays_under_the_cap(name, B, T, K, unscented):
    """The float32 reference against its float64 copy on gapped series, forecast steps included: four times that distance is
    what a case may add to the standard bounds, and it must stay under 2e-4 at the horizons the GPU tests use."""
    c = gc.case(name, B, T, K, unscented=unscented)
    bound, h = gc.bounds(c, K)
    print(name, T, K, unscented, {k: f"{v:.2e}" for k, v in h.items()})
    assert max(bound.values()) <= gc.CAP, (bound, h)


# ---- Python: refused before the device is asked for ---------------------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    import bayesianfiltering_amd as bfa
    T = 6
    _, pp, u = gc.model("bot", T)
    ys = np.zeros((3, T, 2), F32)
    up = bfa.ParamsUKF(1.0, 0.0, 0.0)
    key = bfa.PRNGKey(0)
    calls = {
        "gsf": lambda **kw: bfa.gaussian_sum_filter(pp, ys, 2, 1, u, **kw),
        "ugsf": lambda **kw: bfa.unscented_gaussian_sum_filter(pp, up, ys, 2, 1, u, **kw),
        "eks": lambda **kw: bfa.extended_kalman_smoother(pp, ys, u, **kw),
        "uks": lambda **kw: bfa.unscented_kalman_smoother(pp, up, ys, u, **kw),
        "egs": lambda **kw: bfa.extended_gaussian_sum_smoother(pp, ys, 2, u, **kw),
        "ugs": lambda **kw: bfa.unscented_gaussian_sum_smoother(pp, up, ys, 2, u, **kw),
        "eps": lambda **kw: bfa.extended_kalman_posterior_sample(pp, ys, 2, key, u, **kw),
        "ups": lambda **kw: bfa.unscented_kalman_posterior_sample(pp, up, ys, 2, key, u, **kw),
        "egps": lambda **kw: bfa.extended_gaussian_sum_posterior_sample(pp, ys, 2, 2, key, u, **kw),
        "ugps": lambda **kw: bfa.unscented_gaussian_sum_posterior_sample(pp, up, ys, 2, 2, key, u, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="missing must be None or 'nan'"):
            call(missing="zero")
        with pytest.raises(ValueError, match="bool mask"):
            call(observed=np.ones((T,), F32))
        for shape in ((T + 1,), (3, T, 3), (2, T), (T, 1)):
            with pytest.raises(ValueError, match="observed must have shape"):
                call(observed=np.ones(shape, bool))
    # the augmented and the particle filters do not take the keywords
    with pytest.raises(TypeError):
        bfa.augmented_gaussian_sum_filter(pp, ys, (2, 2, 2), missing="nan")
    with pytest.raises(TypeError):
        bfa.bootstrap_particle_filter(pp, ys, 16, missing="nan")


# ---- C: refused before the first HIP call ----------------------------------------------------------------------------------
class _Call:
    """A valid call of one of the two entry points on small host buffers that no refused call reads."""

    def __init__(self, n=4, m=2, dq=None, dr=None, unscented=False):
        self.keep = keep = []
        self.unscented = unscented

        def fp(x):
            keep.append(np.ascontiguousarray(x, F32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def buf():
            keep.append(np.zeros(4096, F32))
            return keep[-1].ctypes.data

        dq = n if dq is None else dq
        dr = m if dr is None else dr
        self.B, self.T, self.K = 4, 8, 2
        p = self.model = _lib.bf_model()
        p.dyn_id, p.emi_id, p.n, p.dq, p.m, p.dr = 0, 0, n, dq, m, dr          # linear registry functions
        th_d, th_e = np.zeros(n * n + n * dq, F32), np.zeros(m * n + m * dr, F32)
        p.dyn_theta, p.n_dyn_theta, p.emi_theta, p.n_emi_theta = fp(th_d), th_d.size, fp(th_e), th_e.size
        p.q0, p.r0, p.Q, p.R = fp(np.zeros(dq)), fp(np.zeros(dr)), fp(np.eye(dq)), fp(np.eye(dr))
        p.Q_steps, p.R_steps = 1, 1
        self.up = _lib.bf_ukf_params(1.0, 0.0, 0.0)
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = buf(), self.T * m, m, 1
        self.u = _lib.bf_cstream()
        self.carry = _lib.bf_carry()
        self.carry.m_in, self.carry.P_in = buf(), buf()
        self.out = _lib.bf_out_desc()
        o = self.out.means
        o.ptr, o.sB, o.sK, o.sT, o.sE = buf(), self.K * self.T * n, self.T * n, n, 1
        self.null = set()

    def run(self, lib):
        ref = lambda name: None if name in self.null else C.byref(getattr(self, name))
        if self.unscented:
            code = lib.bf_ugsf_ukf_missing_f32(ref("model"), ref("up"), ref("y"), ref("u"), self.B, self.T, self.K, ref("carry"),
                                               ref("out"), None)
        else:
            code = lib.bf_gsf_ekf_missing_f32(ref("model"), ref("y"), ref("u"), self.B, self.T, self.K, ref("carry"), ref("out"), None)
        return code, lib.bf_last_error().decode()


@pytest.mark.parametrize("unscented", [False, True])
def test_c_refusals_common(unscented):
    lib = _lib.load()
    UNSUP, EINVAL = _lib.BF_EUNSUPPORTED, _lib.BF_EINVAL
    for name in ("model", "y", "carry", "out") + (("up",) if unscented else ()):
        c = _Call(unscented=unscented)
        c.null.add(name)
        code, msg = c.run(lib)
        assert code == EINVAL and "NULL argument" in msg, (name, code, msg)
    for field, value in (("B", 0), ("B", -3), ("T", 0), ("T", -1), ("K", 0), ("K", -2)):
        c = _Call(unscented=unscented)
        setattr(c, field, value)
        code, msg = c.run(lib)
        assert code == EINVAL and "must be positive" in msg, (field, value, code, msg)
    c = _Call(unscented=unscented)
    c.y.ptr = None
    assert c.run(lib) == (EINVAL, "observations pointer is NULL")
    for flags in (1, 2, 4):                                   # the legacy classes
        c = _Call(unscented=unscented)
        c.model.flags = flags
        code, msg = c.run(lib)
        assert code == UNSUP and "flags != 0" in msg, (flags, code, msg)
    opt = b"ugsf_force_generic" if unscented else b"force_generic"
    assert lib.bf_set_call_option(opt, 1) == _lib.BF_OK
    code, msg = _Call(unscented=unscented).run(lib)
    assert code == UNSUP and opt.decode() in msg and "no gaps" in msg, (code, msg)


def test_c_refusals_extended():
    lib = _lib.load()
    UNSUP = _lib.BF_EUNSUPPORTED
    # registry models beyond the register kernels: the message names the limit
    for n, m in ((9, 2), (12, 4), (8, 5), (64, 32)):
        code, msg = _Call(n, m).run(lib)
        assert code == UNSUP and "n <= 8 and m <= 4" in msg, (n, m, code, msg)
    code, msg = _Call(2, 3).run(lib)                          # within the limits, not in the table (m > n)
    assert code == UNSUP and "not compiled in" in msg, (code, msg)
    # a lane count other than the compiled default (n = 4: two lanes per chain)
    for lanes in (1, 4, 8):
        assert lib.bf_set_call_option(b"kf_lanes", lanes) == _lib.BF_OK
        code, msg = _Call(4, 2).run(lib)
        assert code == UNSUP and f"kf_lanes={lanes}" in msg and "default is 2" in msg, (lanes, code, msg)
    # models from source the register kernel does not take: the handle is never read (a pointer to nothing)
    for kw, field, value, words in ((dict(n=9, m=2), None, None, "every dimension <= 8"), (dict(n=4, m=2, dr=9), None, None, "every dimension <= 8"),
                                    ({}, "K", 257, "at most 256 components"), ({}, "coll", None, "collapsed")):
        c = _Call(**kw)
        c.model.user = 0x10
        if field == "K":
            c.K = value
        if field == "coll":
            c.out.coll_mean.ptr = c.keep[0].ctypes.data
        code, msg = c.run(lib)
        assert code == UNSUP and words in msg and "from source" in msg, (kw, field, code, msg)


def test_c_refusals_unscented():
    lib = _lib.load()
    UNSUP = _lib.BF_EUNSUPPORTED
    for kw in (dict(n=9, m=2), dict(n=4, m=2, dq=9), dict(n=8, m=9), dict(n=4, m=2, dr=12)):
        code, msg = _Call(unscented=True, **kw).run(lib)
        assert code == UNSUP and "every dimension <= 8" in msg, (kw, code, msg)
    c = _Call(unscented=True)
    c.K = 257
    code, msg = c.run(lib)
    assert code == UNSUP and "at most 256 components" in msg, (code, msg)
    c = _Call(unscented=True)
    c.out.coll_cov.ptr = c.keep[0].ctypes.data
    code, msg = c.run(lib)
    assert code == UNSUP and "collapsed" in msg, (code, msg)
    c = _Call(unscented=True)
    c.up = _lib.bf_ukf_params(0.0, 0.0, 0.0)
    assert c.run(lib)[0] == _lib.BF_EINVAL


def test_symbols_and_header():
    hdr = open(os.path.join(ROOT, "include", "bayesfilt.h")).read()
    for name, twin in (("bf_gsf_ekf_missing_f32", "bf_gsf_ekf_f32"), ("bf_ugsf_ukf_missing_f32", "bf_ugsf_ukf_f32")):
        assert re.search(rf"\bint {name}\(", hdr), name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[twin]
        assert hasattr(_lib.load(), name)
    assert "#define BF_VERSION 210" in hdr
    assert "this header declares 48 entry points" in hdr


# ---- the instance lists -----------------------------------------------------------------------------------------------------
def test_instance_lists_equal_the_plain_tables():
    for g in "abcde":                                           # slice by slice: the one list of (n, m, lanes) rows serves both builds
        plain, miss = cm.instance_rows(f"gsf_group_{g}.hip"), cm.instance_rows(f"gsf_group_{g}.hip", missing=True)
        assert plain and plain == miss, (g, plain, miss)
    cm.assert_slices_are_built_twice("gsf", "abcd", "launch_gsf<N_, M_, NL_, SPEC_GENERIC, BF_MISSING>", "gsf_scan.hip")
    cm.assert_slices_are_built_twice("gsf", "e", "launch_gsf<N_, M_, NL_, SPEC_L96_PICK, BF_MISSING>", "gsf_scan.hip")
    plain = cm.instance_rows("ugsf_group_u.hip") + cm.instance_rows("ugsf_group_v.hip")
    miss = cm.instance_rows("ugsf_group_u.hip", missing=True) + cm.instance_rows("ugsf_group_v.hip", missing=True)
    assert len(plain) == 9 and plain == miss, (plain, miss)
    assert "BF_CASE" not in cm.read_csrc("ugsf_scan.hip")       # the table left the dispatcher: it calls the groups
    cm.assert_slices_are_built_twice("ugsf", "uv", "launch_ugsf<N_, DQ_, M_, DR_, BF_MISSING>", "ugsf_scan.hip")
