"""What the six C entry points of the backward family refuse before their first HIP call, word for word: the RTS smoother
(bf_rts_smoother_f32, bf_eks_smoother_f32, bf_uks_smoother_f32) and the posterior sampler (bf_ffbs_sample_f32,
bf_effbs_sample_f32, bf_uffbs_sample_f32), called through ctypes with host buffers.  No GPU is needed: every row returns
before anything is uploaded or launched.

A row is (name, what to break, code, message).  Each row breaks exactly one check of an otherwise valid call.  The rows
of a route family (linear, extended, unscented) run against both products from one table: the model validation and the
route resolution behind them are shared (csrc/backward_host.hpp), and ``{product}`` in a message is the only word that
differs.  Refusals only one product has are listed per product.  The expected strings were recorded from the library as
it was before the two products' host sides were folded into one."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib

EINVAL, EUNSUPPORTED = _lib.BF_EINVAL, _lib.BF_EUNSUPPORTED
B, T, S = 4, 8, 2
LORENZ63, LINEAR_EMISSION = 2, 0


class Call:
    """A valid call of one entry point: ``family`` in ("linear", "extended", "unscented"), ``product`` in ("smoother",
    "sampler").  The streams point at small host buffers that no row lets the library read."""

    def __init__(self, family, product, n=3):
        self.family, self.product, self.n = family, product, n
        self.keep = keep = []

        def fp(a):
            keep.append(np.ascontiguousarray(a, np.float32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def stream(s):
            keep.append(np.zeros(64, np.float32))
            s.ptr, s.sB, s.sT, s.sE = keep[-1].ctypes.data, 1, 1, 1

        self.filtered = _lib.bf_out_desc()
        for name in ("means", "covs", "pred_means", "pred_covs"):
            stream(getattr(self.filtered, name))
        self.B, self.T, self.S = B, T, S
        self.options = {}
        self.u = _lib.bf_cstream()
        self.uparams = _lib.bf_ukf_params(1.0, 2.0, 0.0)
        eye = np.eye(n, dtype=np.float32)
        if family == "linear":
            m = self.model = _lib.bf_lgssm()
            m.n, m.dq, m.m, m.dr = n, n, 1, 1
            m.A, m.Q, m.Q_steps, m.R_steps = fp(0.5 * eye), fp(eye), 1, 1
        else:
            m = self.model = _lib.bf_model()
            m.dyn_id, m.emi_id, m.n, m.dq, m.m, m.dr = LORENZ63, LINEAR_EMISSION, 3, 3, 2, 2
            m.dyn_theta, m.n_dyn_theta = fp([10.0, 28.0, 2.667, 0.01]), 4
            m.emi_theta, m.n_emi_theta = fp(np.concatenate([np.eye(2, 3).ravel(), np.eye(2).ravel()])), 10
            m.Q, m.R, m.Q_steps, m.R_steps = fp(eye), fp(np.eye(2)), 1, 1
        if product == "smoother":
            self.out = _lib.bf_smooth_desc()
            for name in ("means", "covs", "cross_covs"):
                stream(getattr(self.out, name))
            self.carry = _lib.bf_smooth_carry()
        else:
            self.out = _lib.bf_sample_desc()
            stream(self.out.samples)
            stream(self.out.noise)
            self.carry = _lib.bf_sample_carry()
        self.pointers = {"model": True, "uparams": True, "filtered": True, "out": True}

    def host_ptr(self):
        return self.keep[0].ctypes.data

    def run(self, lib):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        for k, v in self.options.items():
            assert lib.bf_set_call_option(k, v) == _lib.BF_OK
        head = {"linear": (ref("model"),), "extended": (ref("model"), C.byref(self.u)),
                "unscented": (ref("model"), ref("uparams"), C.byref(self.u))}[self.family]
        sizes = (self.B, self.T) if self.product == "smoother" else (self.B, self.T, self.S)
        name = {("linear", "smoother"): "bf_rts_smoother_f32", ("extended", "smoother"): "bf_eks_smoother_f32",
                ("unscented", "smoother"): "bf_uks_smoother_f32", ("linear", "sampler"): "bf_ffbs_sample_f32",
                ("extended", "sampler"): "bf_effbs_sample_f32", ("unscented", "sampler"): "bf_uffbs_sample_f32"}[self.family, self.product]
        code = getattr(lib, name)(*head, ref("filtered"), *sizes, C.byref(self.carry), ref("out"), None)
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


def no_stream(*names):
    def go(c):
        for name in names:
            getattr(c.filtered, name).ptr = None
    return go


def both(*steps):
    def go(c):
        for s in steps:
            s(c)
    return go


def big_linear(n):
    """a linear model of dimension n (the filtered streams are never read, so their buffers need not grow)"""
    def go(c):
        keep = [np.ascontiguousarray(0.5 * np.eye(n, dtype=np.float32)), np.eye(n, dtype=np.float32)]
        c.keep += keep
        c.model.n = c.model.dq = n
        c.model.A, c.model.Q = keep[0].ctypes.data_as(_lib._FP), keep[1].ctypes.data_as(_lib._FP)
    return go


def option(name, value):
    return lambda c: c.options.__setitem__(name, value)


NULL_ARGUMENT = (EINVAL, "NULL argument")
BT = "B and T must be positive (B=%d, T=%d)"
DIMENSION = (EINVAL, "non-positive model dimension")
PAIR = (EINVAL, "pred_means and pred_covs are given together or not at all")

# ---- rows of a route family, run against both products ---------------------------------------------------------------------
LINEAR = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("B-zero", size("B", 0), EINVAL, BT % (0, T)),
    ("T-negative", size("T", -1), EINVAL, BT % (B, -1)),
    ("n-zero", model(n=0)) + DIMENSION,
    ("dq-negative", model(dq=-2)) + DIMENSION,
    ("no-A", model(A=None), EINVAL, "A is required"),
    ("no-G-dq-differs", model(dq=2), EINVAL, "G == NULL requires dq == n"),
    ("no-filtered-means", no_stream("means"), EINVAL, "filtered means and covariances are required"),
    ("no-filtered-covs", no_stream("covs"), EINVAL, "filtered means and covariances are required"),
    ("pred-means-only", no_stream("pred_covs")) + PAIR,
    ("pred-covs-only", no_stream("pred_means")) + PAIR,
    ("recompute-no-Q", both(no_stream("pred_means", "pred_covs"), model(Q=None)), EINVAL, "recomputing the predictions needs Q"),
    ("recompute-Q-steps-5", both(no_stream("pred_means", "pred_covs"), model(Q_steps=5)), EINVAL, "Q_steps must be 1 or T = 8"),
    ("recompute-Q-steps-0", both(no_stream("pred_means", "pred_covs"), model(Q_steps=0)), EINVAL, "Q_steps must be 1 or T = 8"),
]

NEED_PRED = (EINVAL, "the extended and the unscented {product} need the predicted means and covariances")
MODEL = [   # bf_model: the extended and the unscented family
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("flags", model(flags=_lib.BF_MODEL_PREDICT_FIRST), EUNSUPPORTED,
     "the {route} {product} needs the JAX path's update -> predict streams (flags = 0)"),
    ("B-negative", size("B", -4), EINVAL, BT % (-4, T)),
    ("T-zero", size("T", 0), EINVAL, BT % (B, 0)),
    ("n-zero", model(n=0)) + DIMENSION,
    ("m-zero", model(m=0)) + DIMENSION,
    ("dq-zero", model(dq=0)) + DIMENSION,
    ("dr-negative", model(dr=-1)) + DIMENSION,
    ("no-Q", model(Q=None), EINVAL, "Q and R are required"),
    ("no-R", model(R=None), EINVAL, "Q and R are required"),
    ("no-filtered-means", no_stream("means"), EINVAL, "filtered means and covariances are required"),
    ("no-predictions", no_stream("pred_means", "pred_covs")) + NEED_PRED,
]
SOURCE_NULL = (EUNSUPPORTED, "the extended {product} serves functions given as source through bf_model.user (bf_user_model_create); it is NULL")
EXTENDED = MODEL + [
    ("dynamics-from-source-no-handle", model(dyn_id=_lib.BF_FN_USER)) + SOURCE_NULL,
    ("emission-from-source-no-handle", model(emi_id=_lib.BF_FN_USER)) + SOURCE_NULL,
    ("registry-theta-layout", model(n_dyn_theta=3), EINVAL, "lorenz63: n = dq = 3, theta = (sigma, rho, beta, dt)"),
]
NO_SOURCE = (EUNSUPPORTED, "the unscented {product} serves registry dynamics; functions given as source are not supported")
UNSCENTED = MODEL + [
    ("null-uparams", null("uparams")) + NULL_ARGUMENT,
    ("handle", lambda c: setattr(c.model, "user", c.host_ptr())) + NO_SOURCE,
    ("dynamics-from-source", model(dyn_id=_lib.BF_FN_USER)) + NO_SOURCE,
    ("emission-from-source", model(emi_id=_lib.BF_FN_USER)) + NO_SOURCE,
    ("alpha-zero", lambda c: setattr(c.uparams, "alpha", 0.0), EINVAL, "ParamsUKF.alpha must be positive"),
    ("alpha-negative", lambda c: setattr(c.uparams, "alpha", -1.0), EINVAL, "ParamsUKF.alpha must be positive"),
    ("lambda-cancels-L", lambda c: setattr(c.uparams, "kappa", -6.0), EINVAL,
     "ParamsUKF: L + lambda = alpha^2 (n + dq + kappa) must be positive and finite (alpha = 1, kappa = -6, n + dq = 6)"),
    ("lambda-below-minus-L", lambda c: setattr(c.uparams, "kappa", -8.0), EINVAL,
     "ParamsUKF: L + lambda = alpha^2 (n + dq + kappa) must be positive and finite (alpha = 1, kappa = -8, n + dq = 6)"),
]
SHARED = {"linear": LINEAR, "extended": EXTENDED, "unscented": UNSCENTED}

# ---- rows only one product has --------------------------------------------------------------------------------------------
def smooth_out(name):
    return lambda c: setattr(getattr(c.out, name), "ptr", None)


def carry(**fields):
    return lambda c: [setattr(c.carry, k, c.host_ptr()) for k in fields]


NO_OUTPUT = (EINVAL, "smoothed means and covariances are required outputs")
STAGED_GENERIC = (EINVAL, "rts_load_mode = 2 needs n <= 4 on the register kernel")
STAGED_LAYOUT = (EINVAL, "rts_load_mode = 2 needs n <= 4 and the contiguous reference layout with 16-byte aligned rows")
SMOOTHER_ANY = [
    ("no-smoothed-means", smooth_out("means")) + NO_OUTPUT,
    ("no-smoothed-covs", smooth_out("covs")) + NO_OUTPUT,
    ("carry-m-in-only", carry(m_in=1), EINVAL, "carry.m_in and carry.P_in are given together or not at all"),
    ("carry-P-in-only", carry(P_in=1), EINVAL, "carry.m_in and carry.P_in are given together or not at all"),
    ("carry-m-out-only", carry(m_out=1), EINVAL, "carry.m_out and carry.P_out are given together or not at all"),
    ("carry-P-out-only", carry(P_out=1), EINVAL, "carry.m_out and carry.P_out are given together or not at all"),
]
SMOOTHER = {
    "linear": SMOOTHER_ANY + [
        ("staged-n-5", both(option(b"rts_load_mode", 2), big_linear(5))) + STAGED_LAYOUT,
        ("staged-n-9", both(option(b"rts_load_mode", 2), big_linear(9))) + STAGED_GENERIC,
        ("lds-n-200", big_linear(200), EUNSUPPORTED, "smoother: n = 200 needs 807200 bytes of LDS (160 KiB per workgroup)"),
    ],
    "extended": SMOOTHER_ANY + [
        ("pred-means-only", no_stream("pred_covs")) + NEED_PRED,
        ("pred-covs-only", no_stream("pred_means")) + NEED_PRED,
        ("staged-strided-layout", option(b"rts_load_mode", 2)) + STAGED_LAYOUT,
    ],
    "unscented": SMOOTHER_ANY + [
        ("pred-means-only", no_stream("pred_covs")) + NEED_PRED,
        ("pred-covs-only", no_stream("pred_means")) + NEED_PRED,
        ("staged", option(b"rts_load_mode", 2), EINVAL, "rts_load_mode = 2 is not offered on the unscented route"),
    ],
}


def sample_out(**fields):
    def go(c):
        for k, v in fields.items():
            if k == "keys":
                c.out.keys = c.host_ptr() if v else None
            else:
                getattr(c.out, k).ptr = None
    return go


S_MSG = "the number of samples S must be positive (S=%d)"
SAMPLER_ANY = [
    ("S-zero", size("S", 0), EINVAL, S_MSG % 0),
    ("S-negative", size("S", -3), EINVAL, S_MSG % -3),
    ("no-samples", sample_out(samples=None), EINVAL, "the samples stream is a required output"),
    ("no-noise-no-keys", sample_out(noise=None), EINVAL, "give the noise stream or the keys"),
    ("keys-too-many-values", both(sample_out(noise=None, keys=True), size("S", 1 << 20), size("T", 1 << 10)), EINVAL,
     "drawing from keys serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T"),
    ("S-too-large", size("S", 1 << 30), EINVAL, "S too large"),
    ("pred-means-only", no_stream("pred_covs")) + PAIR,
    ("pred-covs-only", no_stream("pred_means")) + PAIR,
]
SAMPLER = {
    "linear": SAMPLER_ANY[:-2] + [
        ("grid-too-large", size("B", 1 << 41), EINVAL, "sampler: B x S too large for one launch"),
        ("lds-n-200", big_linear(200), EUNSUPPORTED, "sampler: n = 200 needs 808800 bytes of LDS (160 KiB per workgroup: n <= 89)"),
    ],
    "extended": SAMPLER_ANY,
    "unscented": SAMPLER_ANY,
}


def _cases():
    for family, rows in SHARED.items():
        for product in ("smoother", "sampler"):
            for row in rows:
                yield pytest.param(family, product, row, id=f"{family}-{product}-{row[0]}")
    for product, table in (("smoother", SMOOTHER), ("sampler", SAMPLER)):
        for family, rows in table.items():
            for row in rows:
                yield pytest.param(family, product, row, id=f"{family}-{product}-only-{row[0]}")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("family, product, row", _cases())
def test_refusal_code_and_message(lib, family, product, row):
    _, break_it, code, message = row
    call = Call(family, product)
    break_it(call)
    route = {"extended": "extended", "unscented": "unscented"}.get(family, "")
    assert call.run(lib) == (code, message.format(product=product, route=route))


def test_ffbs_spl_outside_the_compiled_counts(lib):
    for setter in (lib.bf_set_option, lib.bf_set_call_option):
        for value in (3, -1, 16):
            assert setter(b"ffbs_spl", value) == EINVAL
            assert lib.bf_last_error() == b"ffbs_spl must be 0, 1, 2, 4 or 8"
