"""The parallel-in-time RTS smoother without a GPU: the algebra of its header restated in float64, what
bf_rts_smoother_pscan_f32 refuses before its first HIP call (through ctypes with host buffers, word for word), the workspace
size against its documented formula, and the Python-side refusals that precede device work."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import common as cm
from tests import parallel_smoother_cases as psc

EINVAL, EUNSUPPORTED = _lib.BF_EINVAL, _lib.BF_EUNSUPPORTED
B, T = 4, 8
ALGEBRA_TOL = 1e-10   # float64 arithmetic on well-conditioned 1..4-dimensional systems: ~1e-16 x a few hundred operations


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-30))


@pytest.mark.parametrize("recompute", [False, True], ids=["given", "recomputed"])
@pytest.mark.parametrize("name", ["2x1", "bias", "cv"])
def test_combination_is_associative_and_suffixes_are_the_smoother(name, recompute):
    Tn = 48
    a, ys, init, _ = psc.case(name, 1, Tn)
    kf = psc.kalman_f64(a, ys[0].astype(np.float64), init[0], a["P0"])
    ms, Ps, _ = psc.rts_f64(kf["m"], kf["P"], kf["pm"], kf["pP"], a["A"])
    pred = (lambda t: (None, None)) if recompute else (lambda t: (kf["pm"][t], kf["pP"][t]))
    els = [psc.element(a, kf["m"][t], kf["P"][t], *pred(t)) for t in range(Tn - 1)]
    # (a (+) b) (+) c == a (+) (b (+) c), on single steps and on spans
    for i in (1, 7, 20):
        x, y, z = els[i], psc.combine(els[i + 1], els[i + 2]), els[i + 3]
        left, right = psc.combine(psc.combine(x, y), z), psc.combine(x, psc.combine(y, z))
        for l, r in zip(left, right):
            assert _rel(l, r) <= ALGEBRA_TOL
    # the suffix of the elements of steps t ... T-2 applied to the filtered state at T-1 is the smoother at t
    m, P = kf["m"][Tn - 1], kf["P"][Tn - 1]
    n = m.shape[0]
    suffix = None
    for t in range(Tn - 2, -1, -1):
        suffix = els[t] if suffix is None else psc.combine(els[t], suffix)
        mt, Pt = psc.apply_span(suffix, m, P)
        assert _rel(mt, ms[t]) <= ALGEBRA_TOL
        assert _rel(Pt, Ps[t]) <= ALGEBRA_TOL
        # a smoothed state is the span (0, m, P): combining with it is apply_span and leaves E exactly 0
        g = psc.combine(suffix, (np.zeros((n, n)), m, P))
        assert not g[0].any()
        assert _rel(g[1], mt) <= ALGEBRA_TOL and _rel(g[2], Pt) <= ALGEBRA_TOL


class Call:
    """A valid call of bf_rts_smoother_pscan_f32 on host buffers that no row lets the library read."""

    def __init__(self, n=3):
        self.keep = keep = []

        def fp(a):
            keep.append(np.ascontiguousarray(a, np.float32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def buf():
            keep.append(np.zeros(4096, np.float32))
            return keep[-1].ctypes.data

        m = self.model = _lib.bf_lgssm()
        m.n, m.dq, m.m, m.dr = n, n, 1, 1
        m.A, m.Q = fp(0.5 * np.eye(n)), fp(np.eye(n))
        m.Q_steps, m.R_steps = 1, 1
        self.filtered = _lib.bf_out_desc()
        for name, e in (("means", n), ("covs", n * n), ("pred_means", n), ("pred_covs", n * n)):
            s = getattr(self.filtered, name)
            s.ptr, s.sB, s.sT, s.sE = buf(), T * e, e, 1
        self.out = _lib.bf_smooth_desc()
        for name, e in (("means", n), ("covs", n * n)):
            s = getattr(self.out, name)
            s.ptr, s.sB, s.sT, s.sE = buf(), T * e, e, 1
        self.carry = None
        self.workspace = buf()
        self.B, self.T, self.workspace_bytes, self.block = B, T, 4096 * 4, 0
        self.pointers = {"model": True, "filtered": True, "out": True, "workspace": True}

    def run(self, lib):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        ws = self.workspace if self.pointers["workspace"] else None
        if self.block:
            assert lib.bf_set_call_option(b"prs_block", self.block) == _lib.BF_OK
        code = lib.bf_rts_smoother_pscan_f32(ref("model"), ref("filtered"), self.B, self.T,
                                             C.byref(self.carry) if self.carry is not None else None, ref("out"), ws,
                                             self.workspace_bytes, None)
        return code, lib.bf_last_error().decode()


def null(name):
    return lambda c: c.pointers.__setitem__(name, False)


def size(**values):
    def go(c):
        for k, v in values.items():
            setattr(c, k, v)
    return go


def model(**fields):
    def go(c):
        for k, v in fields.items():
            setattr(c.model, k, v)
    return go


def no_stream(desc, *names):
    def go(c):
        for name in names:
            getattr(getattr(c, desc), name).ptr = None
    return go


def half_carry(c):
    c.carry = _lib.bf_smooth_carry()
    c.carry.m_in = c.keep[0].ctypes.data


def misaligned(c):
    c.workspace += 1


NULL_ARGUMENT = (EINVAL, "NULL argument")
BT = "B and T must be positive (B=%d, T=%d)"
FILTERED = "filtered means and covariances are required"
SMOOTHED = "smoothed means and covariances are required outputs"
TOGETHER = "pred_means and pred_covs are given together or not at all"
DIMS = "parallel rts smoother: n=%d is not compiled in (register kernels for n = 1..6, the parallel filter's limit)"
CONSTANT = "parallel rts smoother: constant Q only (Q_steps=%d)"
LANES = "parallel rts smoother: B * ceil(T / block) = %d * %d must stay below 2^31"
# B = 4, T = 8, default block 16: one block per trajectory, 4 * 4 * 1 * (3 * 9 + 2 * 3) bytes
SMALL = "parallel rts smoother: workspace of 527 bytes is too small: B=4, T=8, block=16 need 528 bytes (bf_rts_pscan_workspace_bytes)"
ALIGNED = "parallel rts smoother: workspace must be 4-byte aligned"

ROWS = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("null-workspace", null("workspace")) + NULL_ARGUMENT,
    ("no-filtered-means", no_stream("filtered", "means"), EINVAL, FILTERED),
    ("no-filtered-covs", no_stream("filtered", "covs"), EINVAL, FILTERED),
    ("no-smoothed-means", no_stream("out", "means"), EINVAL, SMOOTHED),
    ("no-smoothed-covs", no_stream("out", "covs"), EINVAL, SMOOTHED),
    ("pred-means-alone", no_stream("filtered", "pred_covs"), EINVAL, TOGETHER),
    ("pred-covs-alone", no_stream("filtered", "pred_means"), EINVAL, TOGETHER),
    ("B-zero", size(B=0), EINVAL, BT % (0, T)),
    ("T-negative", size(T=-1), EINVAL, BT % (B, -1)),
    ("too-many-lanes", size(B=2 ** 20, T=2 ** 20, block=4), EINVAL, LANES % (2 ** 20, 2 ** 18)),
    ("n-above-the-built-limit", model(n=7, dq=7), EUNSUPPORTED, DIMS % 7),
    ("per-step-Q", model(Q_steps=T), EUNSUPPORTED, CONSTANT % T),
    ("workspace-too-small", size(workspace_bytes=527), EINVAL, SMALL),
    ("workspace-misaligned", misaligned, EINVAL, ALIGNED),
    ("half-a-carry", half_carry, EINVAL, "carry.m_in and carry.P_in are given together or not at all"),
]


@pytest.mark.parametrize("name,breaker,code,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusals_before_the_first_hip_call(name, breaker, code, message):
    lib = _lib.load()
    call = Call()
    breaker(call)
    assert call.run(lib) == (code, message)


@pytest.mark.parametrize("value", [3, -1, 4097])
def test_block_length_out_of_range_is_refused(value):
    lib = _lib.load()
    assert lib.bf_set_call_option(b"prs_block", value) == EINVAL
    assert lib.bf_last_error().decode() == "prs_block must be 0 or 4..4096"
    assert lib.bf_set_option(b"prs_block", value) == EINVAL
    assert lib.bf_rts_pscan_workspace_bytes(3, B, T, value) == EINVAL
    assert lib.bf_last_error().decode() == f"parallel rts smoother: block length {value} is outside 4..4096"


def test_workspace_bytes_formula():
    lib = _lib.load()
    for n, b, t, block in [(1, 1, 1, 4), (4, 3, 1203, 4), (4, 3, 1000, 64), (6, 5, 37, 64), (2, 7, 4096, 4096)]:
        blocks = -(-t // block)
        assert lib.bf_rts_pscan_workspace_bytes(n, b, t, block) == 4 * b * blocks * (3 * n * n + 2 * n)
    # block = 0: the parallel filter's rule -- the largest of ceil(B T / 65 536), the smallest s with 50 s^2 >= T, and 16;
    # at most 4096
    for b, t, block in [(1, 5000, 16), (64, 300, 16), (1, 10 ** 6, 142), (8, 10 ** 6, 142), (64, 10 ** 5, 98), (1, 10 ** 7, 448),
                        (65536, 10 ** 4, 4096)]:
        s = next(s for s in range(1, 4097) if 50 * s * s >= t or s == 4096)
        assert block == min(max(-(-b * t // 65536), s, 16), 4096)
        blocks = -(-t // block)
        assert lib.bf_rts_pscan_workspace_bytes(4, b, t, 0) == 4 * b * blocks * (3 * 16 + 8)
        assert lib.bf_rts_pscan_workspace_bytes(4, b, t, 0) <= lib.bf_kalman_pscan_workspace_bytes(4, 2, b, t, 0)
    assert lib.bf_rts_pscan_workspace_bytes(4, 0, 10, 4) == EINVAL
    assert lib.bf_rts_pscan_workspace_bytes(4, 10, -1, 4) == EINVAL
    assert lib.bf_rts_pscan_workspace_bytes(7, 10, 10, 4) == EUNSUPPORTED
    assert lib.bf_rts_pscan_workspace_bytes(0, 10, 10, 4) == EINVAL
    assert lib.bf_rts_pscan_workspace_bytes(1, 2 ** 20, 2 ** 20, 4) == EINVAL   # B * blocks >= 2^31


def _posterior(B_, K, T_, n, pred=True):
    import torch
    import bayesianfiltering_amd as bfa
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return bfa.PosteriorGaussianSumFiltered(None, z(B_, K, T_, n), z(B_, K, T_, n, n), z(B_, K, T_, n) if pred else None,
                                            z(B_, K, T_, n, n) if pred else None)


def test_python_refusals_that_precede_device_work():
    import torch
    import bayesianfiltering_amd as bfa
    lin = cm.product_params(cm.cv_model_arrays())
    with pytest.raises(ValueError, match="one component"):
        bfa.parallel_rts_smoother(lin, _posterior(2, 3, 8, 4))
    post = _posterior(2, 1, 8, 4)
    with pytest.raises(ValueError, match="together"):
        bfa.parallel_rts_smoother(lin, post._replace(predicted_means=None))
    with pytest.raises(ValueError, match="together"):
        bfa.parallel_rts_smoother(lin, post._replace(predicted_covariances=None))
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"out.smoothed_means has shape \(2, 1, 7, 4\), expected \(2, 1, 8, 4\)"):
        bfa.parallel_rts_smoother(lin, post, out=bfa.PosteriorGaussianSmoothed(smoothed_means=z(2, 1, 7, 4)))
    # the cross-covariances have T-1 steps without a carry
    with pytest.raises(ValueError, match=r"out.smoothed_cross_covariances has shape \(2, 1, 8, 4, 4\), expected \(2, 1, 7, 4, 4\)"):
        bfa.parallel_rts_smoother(lin, post, out=bfa.PosteriorGaussianSmoothed(smoothed_cross_covariances=z(2, 1, 8, 4, 4)))
    with pytest.raises(TypeError):
        bfa.parallel_rts_smoother(lin, post, extended=True)
