"""What the five five-stream entry points of the forward family refuse before their first HIP call, word for word:
bf_kalman_filter_f32, bf_gsf_ekf_f32, bf_ugsf_ukf_f32, bf_agsf_ekf_f32 and bf_agsf_ukf_f32, called through ctypes with host
buffers.  No GPU is needed: every row returns before anything is uploaded or launched.  (The sixth,
bf_kalman_filter_pscan_f32, has its table in test_parallel_kalman_cpu.py.)

A row is (name, what to break, code, message).  A row breaks one check of an otherwise valid call; the rows named
``a+b`` break two, where the order of the checks decides which message the caller reads -- the entry points do not all
order them alike, and the order is part of what they promise.  The expected strings were recorded from the library as it
was before the entry points' shared checks moved into csrc/forward_host.hpp.

The second table holds every name bf_set_option / bf_set_call_option know: one accepted value, one refused value with its
message, and the message for a name they do not know."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib

EINVAL = _lib.BF_EINVAL
B, T, K = 4, 8, 3
ENTRIES = ("bf_kalman_filter_f32", "bf_gsf_ekf_f32", "bf_ugsf_ukf_f32", "bf_agsf_ekf_f32", "bf_agsf_ukf_f32")
KALMAN, GSF, UGSF, AGSF, UAGSF = ENTRIES
UNSCENTED, AUGMENTED = (UGSF, UAGSF), (AGSF, UAGSF)


class Call:
    """A valid call of one entry point on small host buffers that no row lets the library read."""

    def __init__(self, entry, n=3, m=2):
        self.entry = entry
        self.keep = keep = []

        def fp(a):
            keep.append(np.ascontiguousarray(a, np.float32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def buf():
            keep.append(np.zeros(1024, np.float32))
            return keep[-1].ctypes.data

        if entry == KALMAN:
            p = self.model = _lib.bf_lgssm()
            p.n, p.dq, p.m, p.dr = n, n, m, m
            p.A, p.H, p.Q, p.R = fp(0.5 * np.eye(n)), fp(np.eye(m, n)), fp(np.eye(n)), fp(np.eye(m))
        else:   # a linear registry model: dyn_id = emi_id = 0, theta = (A | G), (H | D)
            p = self.model = _lib.bf_model()
            p.n, p.dq, p.m, p.dr = n, n, m, m
            p.dyn_theta, p.n_dyn_theta = fp(np.concatenate([0.5 * np.eye(n).ravel(), np.eye(n).ravel()])), 2 * n * n
            p.emi_theta, p.n_emi_theta = fp(np.concatenate([np.eye(m, n).ravel(), np.eye(m).ravel()])), m * n + m * m
            p.Q, p.R = fp(np.eye(n)), fp(np.eye(m))
        p.Q_steps, p.R_steps = 1, 1
        self.uparams = _lib.bf_ukf_params(1.0, 2.0, 0.0)
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = buf(), T * m, m, 1
        self.u = _lib.bf_cstream()
        self.carry = _lib.bf_carry()
        self.carry.m_in, self.carry.P_in = buf(), buf()
        self.out = _lib.bf_out_desc()
        self.out.means.ptr, self.out.means.sB, self.out.means.sK, self.out.means.sT, self.out.means.sE = buf(), K * T * n, T * n, n, 1
        self.nc = (C.c_int32 * 3)(2, 2, 2)
        self.key = (C.c_uint32 * 2)(0, 0)
        self.opt = (C.c_float * 2)(0.1, 0.1)
        self.B, self.T, self.K, self.variant = B, T, K, 0
        self.pointers = dict.fromkeys(("model", "uparams", "y", "carry", "out", "nc", "key", "opt"), True)

    def host_ptr(self):
        return self.keep[0].ctypes.data

    def run(self, lib):
        on = self.pointers
        ref = lambda name: C.byref(getattr(self, name)) if on[name] else None
        arr = lambda name: getattr(self, name) if on[name] else None
        e = self.entry
        head = (ref("model"),) + ((ref("uparams"),) if e in UNSCENTED else ())
        if e == KALMAN:
            args = head + (ref("y"), self.B, self.T, ref("carry"), ref("out"), None)
        elif e in (GSF, UGSF):
            args = head + (ref("y"), C.byref(self.u), self.B, self.T, self.K, ref("carry"), ref("out"), None)
        else:
            args = head + (ref("y"), C.byref(self.u), self.B, self.T, arr("nc"), arr("key"), arr("opt"), ref("carry"), ref("out"),
                           None, self.variant, None)
        code = getattr(lib, e)(*args)
        return code, lib.bf_last_error().decode()


def null(name):
    return lambda c: c.pointers.__setitem__(name, False)


def size(name, value):
    return lambda c: setattr(c, name, value)


def model(**fields):
    def go(c):
        for k, v in fields.items():
            setattr(c.model, k, v)
    return go


def collapsed(name):
    return lambda c: setattr(getattr(c.out, name), "ptr", c.host_ptr())


def no_y(c):
    c.y.ptr = None


def no_carry(name):
    return lambda c: setattr(c.carry, name, None)


def alpha(value):
    return lambda c: setattr(c.uparams, "alpha", value)


def components(i, value):
    return lambda c: c.nc.__setitem__(i, value)


def both(*steps):
    def go(c):
        for s in steps:
            s(c)
    return go


NULL_ARGUMENT = (EINVAL, "NULL argument")
DIMENSION = (EINVAL, "non-positive model dimension")
NO_Y = (EINVAL, "observations pointer is NULL")
NO_CARRY = (EINVAL, "carry.m_in and carry.P_in are required")
STEPS = (EINVAL, "Q_steps / R_steps must be >= 1")
ALPHA = (EINVAL, "ParamsUKF.alpha must be positive")

# ---- what every entry point refuses, in the words they share --------------------------------------------------------------
SHARED = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-y", null("y")) + NULL_ARGUMENT,
    ("null-carry", null("carry")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("null-model+B-zero", both(null("model"), size("B", 0))) + NULL_ARGUMENT,
    ("n-zero", model(n=0)) + DIMENSION,
    ("m-negative", model(m=-1)) + DIMENSION,
    ("dq-zero", model(dq=0)) + DIMENSION,
    ("dr-zero", model(dr=0)) + DIMENSION,
    ("no-observations", no_y) + NO_Y,
    ("no-carry-m-in", no_carry("m_in")) + NO_CARRY,
    ("no-carry-P-in", no_carry("P_in")) + NO_CARRY,
    ("no-observations+no-carry-m-in", both(no_y, no_carry("m_in"))) + NO_Y,
]

# ---- bf_kalman_filter_f32 ---------------------------------------------------------------------------------------------------
COLLAPSED = (EINVAL, "collapsed streams are produced by bf_gsf_ekf_f32 (with one component they equal means / covs)")
BT = "B and T must be positive (B=%d, T=%d)"
REQUIRED = (EINVAL, "A, H, Q, R are required")
NO_G = (EINVAL, "G == NULL requires dq == n")
NO_D = (EINVAL, "D == NULL requires dr == m")
KALMAN_ROWS = SHARED + [
    ("collapsed-mean", collapsed("coll_mean")) + COLLAPSED,
    ("collapsed-cov", collapsed("coll_cov")) + COLLAPSED,
    ("collapsed-mean+null-model", both(collapsed("coll_mean"), null("model"))) + COLLAPSED,   # before the NULL pointers
    ("collapsed-cov+B-zero", both(collapsed("coll_cov"), size("B", 0))) + COLLAPSED,
    ("B-zero", size("B", 0), EINVAL, BT % (0, T)),
    ("T-negative", size("T", -1), EINVAL, BT % (B, -1)),
    ("B-zero+n-zero", both(size("B", 0), model(n=0)), EINVAL, BT % (0, T)),
    ("no-A", model(A=None)) + REQUIRED,
    ("no-H", model(H=None)) + REQUIRED,
    ("no-Q", model(Q=None)) + REQUIRED,
    ("no-R", model(R=None)) + REQUIRED,
    ("no-G-dq-differs", model(dq=2)) + NO_G,
    ("no-D-dr-differs", model(dr=1)) + NO_D,
    ("Q-steps-zero", model(Q_steps=0)) + STEPS,
    ("R-steps-negative", model(R_steps=-1)) + STEPS,
    ("n-zero+no-A", both(model(n=0), model(A=None))) + DIMENSION,
    ("no-A+no-G-dq-differs", both(model(A=None), model(dq=2))) + REQUIRED,
    ("no-G-dq-differs+no-D-dr-differs", model(dq=2, dr=1)) + NO_G,
    ("no-D-dr-differs+Q-steps-zero", model(dr=1, Q_steps=0)) + NO_D,
    ("Q-steps-zero+no-observations", both(model(Q_steps=0), no_y)) + STEPS,
]

# ---- the Gaussian-sum entry points (bf_model) -----------------------------------------------------------------------------------
NO_QR = (EINVAL, "Q and R are required")
MODEL = SHARED + [
    ("no-Q", model(Q=None)) + NO_QR,
    ("no-R", model(R=None)) + NO_QR,
    ("n-zero+no-Q", model(n=0, Q=None)) + DIMENSION,
    ("no-Q+no-observations", both(model(Q=None), no_y)) + NO_QR,
]
BTK = (EINVAL, "B, T and K must be positive")
BANK = MODEL + [   # bf_gsf_ekf_f32, bf_ugsf_ukf_f32
    ("B-zero", size("B", 0)) + BTK,
    ("T-negative", size("T", -1)) + BTK,
    ("K-zero", size("K", 0)) + BTK,
    ("K-zero+n-zero", both(size("K", 0), model(n=0))) + BTK,
]
UKF = [
    ("null-uparams", null("uparams")) + NULL_ARGUMENT,
    ("alpha-zero", alpha(0.0)) + ALPHA,
    ("alpha-negative", alpha(-1.0)) + ALPHA,
    ("alpha-nan", alpha(float("nan"))) + ALPHA,
    ("no-carry-P-in+alpha-zero", both(no_carry("P_in"), alpha(0.0))) + NO_CARRY,   # alpha is looked at last
]
BT_PLAIN = (EINVAL, "B and T must be positive")
COUNTS = (EINVAL, "num_components must be three positive counts")
TREE = MODEL + [   # bf_agsf_ekf_f32, bf_agsf_ukf_f32
    ("null-num-components", null("nc")) + NULL_ARGUMENT,
    ("null-key", null("key")) + NULL_ARGUMENT,
    ("null-opt-args", null("opt")) + NULL_ARGUMENT,
    ("B-zero", size("B", 0)) + BT_PLAIN,
    ("T-negative", size("T", -1)) + BT_PLAIN,
    ("N0-zero", components(0, 0)) + COUNTS,
    ("N1-negative", components(1, -2)) + COUNTS,
    ("N2-zero", components(2, 0)) + COUNTS,
    ("B-zero+N0-zero", both(size("B", 0), components(0, 0))) + BT_PLAIN,
    ("N0-zero+n-zero", both(components(0, 0), model(n=0))) + COUNTS,
]
VARIANT3 = (EINVAL, "variant must be 0 (speedy), 1 (container branches) or 2 (container branches + optimal resampling)")
VARIANT2 = (EINVAL, "variant must be 0 (speedy) or 1 (container branches)")
ROWS = {
    KALMAN: KALMAN_ROWS,
    GSF: BANK,
    UGSF: BANK + UKF,
    AGSF: TREE + [
        ("variant-negative", size("variant", -1)) + VARIANT3,
        ("variant-three", size("variant", 3)) + VARIANT3,
        ("variant-three+null-model", both(size("variant", 3), null("model"))) + VARIANT3,   # before the NULL pointers
        ("Q-steps-zero", model(Q_steps=0)) + STEPS,
        ("R-steps-negative", model(R_steps=-1)) + STEPS,
        ("no-Q+Q-steps-zero", model(Q=None, Q_steps=0)) + NO_QR,
        ("Q-steps-zero+no-observations", both(model(Q_steps=0), no_y)) + STEPS,
    ],
    UAGSF: TREE + UKF + [
        ("variant-negative", size("variant", -1)) + VARIANT2,
        ("variant-two", size("variant", 2)) + VARIANT2,     # optimal resampling is the extended tree's alone
        ("variant-two+null-uparams", both(size("variant", 2), null("uparams"))) + VARIANT2,
        # bf_agsf_ukf_f32 has no Q_steps / R_steps check where its extended twin refuses them (the row above it in AGSF): the
        # call goes on to the next refusal.  Recorded as it is; whether it should refuse them is a question of its own.
        ("Q-steps-zero+no-observations", both(model(Q_steps=0), no_y)) + NO_Y,
        ("Q-steps-zero+alpha-zero", both(model(Q_steps=0), alpha(0.0))) + ALPHA,
    ],
}


def _cases():
    for entry in ENTRIES:
        for row in ROWS[entry]:
            yield pytest.param(entry, row, id=f"{entry}-{row[0]}")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("entry, row", _cases())
def test_refusal_code_and_message(lib, entry, row):
    _, break_it, code, message = row
    call = Call(entry)
    break_it(call)
    assert call.run(lib) == (code, message)


# ---- the tuning options: (name, the default -- accepted --, another accepted value, a refused value, its message) ---------------
OPTIONS = [
    ("kf_emit_mode", -1, 2, 3, "kf_emit_mode must be -1..2"),
    ("kf_lanes", 0, 64, 3, "kf_lanes must be 0 or a power of two <= 64"),
    ("kf_small_mode", 1, 0, 2, "kf_small_mode must be 0 or 1"),
    ("force_generic", 0, 1, -1, "force_generic must be 0 or 1"),
    ("ugsf_force_generic", 0, 1, 2, "ugsf_force_generic must be 0 or 1"),
    ("agsf_force_generic", 0, 1, 2, "agsf_force_generic must be 0 or 1"),
    ("rts_load_mode", -1, 2, 1, "rts_load_mode must be -1, 0 or 2"),
    ("ffbs_spl", 0, 8, 3, "ffbs_spl must be 0, 1, 2, 4 or 8"),
    ("pkf_block", 0, 4096, 3, "pkf_block must be 0 or 4..4096"),
    ("gsf_structured", 1, 0, 2, "gsf_structured must be 0 or 1"),
    ("bpf_variant", 0, 1, 2, "bpf_variant must be 0 or 1"),
    ("bpf_hbm_mode", 0, 2, 3, "bpf_hbm_mode must be 0, 1 or 2"),
    ("bpf_arith", 0, 1, -1, "bpf_arith must be 0 or 1"),
    ("bpf_spec", 1, 0, 2, "bpf_spec must be 0 or 1"),
]


@pytest.mark.parametrize("name, default, other, refused, message", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_option_values(lib, name, default, other, refused, message):
    key = name.encode()
    for setter in (lib.bf_set_option, lib.bf_set_call_option):
        assert setter(key, refused) == EINVAL
        assert lib.bf_last_error().decode() == message
    # (the process-wide setter is given the default only: other tests of this process read these options)
    assert lib.bf_set_option(key, default) == _lib.BF_OK
    assert lib.bf_set_call_option(key, other) == _lib.BF_OK
    assert lib.bf_set_call_option(key, default) == _lib.BF_OK
    # (an entry point disarms this thread's call options when it returns, a refusal included: nothing stays armed)
    call = Call(GSF)
    null("model")(call)
    assert call.run(lib) == NULL_ARGUMENT


def test_unknown_option_name(lib):
    for setter in (lib.bf_set_option, lib.bf_set_call_option):
        assert setter(b"kf_lane", 0) == EINVAL
        assert lib.bf_last_error().decode() == "unknown option 'kf_lane'"
        assert setter(None, 0) == EINVAL
        assert lib.bf_last_error().decode() == "unknown option '(null)'"
