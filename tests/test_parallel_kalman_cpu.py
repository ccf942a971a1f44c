"""The parallel-in-time Kalman filter without a GPU: the algebra of its header restated in float64, what
bf_kalman_filter_pscan_f32 refuses before its first HIP call (through ctypes with host buffers, word for word), and the
workspace size against its documented formula."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import parallel_kalman_cases as pk

EINVAL, EUNSUPPORTED = _lib.BF_EINVAL, _lib.BF_EUNSUPPORTED
B, T = 4, 8
ALGEBRA_TOL = 1e-10   # float64 arithmetic on well-conditioned 1..4-dimensional systems: ~1e-16 x a few hundred operations


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-30))


@pytest.mark.parametrize("name", ["2x1", "bias", "cv"])
def test_combination_is_associative_and_prefixes_are_the_filter(name):
    a, ys, init, _ = pk.case(name, 1, 48)
    els = [pk.element(a, ys[0, t]) for t in range(48)]
    # (a (+) b) (+) c == a (+) (b (+) c), on single steps and on spans
    for i in (1, 7, 20):
        x, y, z = els[i], pk.combine(els[i + 1], els[i + 2]), els[i + 3]
        left, right = pk.combine(pk.combine(x, y), z), pk.combine(x, pk.combine(y, z))
        for l, r in zip(left, right):
            assert _rel(l, r) <= ALGEBRA_TOL
    # the prefix of the elements of steps 1 ... t applied to the filtered state of step 0 is the jitter-free filter at t
    ref = pk.kalman_f64(a, ys, init, a["P0"], jitter=0.0)
    m, P = ref["means"][0, 0, 0], ref["covariances"][0, 0, 0]
    prefix = els[1]
    for t in range(1, 48):
        if t > 1:
            prefix = pk.combine(prefix, els[t])
        mt, Pt = pk.apply_span(prefix, m, P)
        assert _rel(mt, ref["means"][0, 0, t]) <= ALGEBRA_TOL
        assert _rel(Pt, ref["covariances"][0, 0, t]) <= ALGEBRA_TOL
    # a filtered state is the span (0, m, P, 0, 0): combining it with a later span is apply_span
    n = m.shape[0]
    g = pk.combine((np.zeros((n, n)), m, P, np.zeros(n), np.zeros((n, n))), prefix)
    assert _rel(g[1], mt) <= ALGEBRA_TOL and _rel(g[2], Pt) <= ALGEBRA_TOL
    assert not g[0].any() and not g[3].any() and not g[4].any()


class Call:
    """A valid call of bf_kalman_filter_pscan_f32 on host buffers that no row lets the library read."""

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
        m.A, m.H, m.Q, m.R = fp(0.5 * np.eye(n)), fp(np.ones((1, n))), fp(np.eye(n)), fp(np.eye(1))
        m.Q_steps, m.R_steps = 1, 1
        self.y = _lib.bf_cstream()
        self.y.ptr, self.y.sB, self.y.sT, self.y.sE = buf(), T, 1, 1
        self.carry = _lib.bf_carry()
        self.carry.m_in, self.carry.P_in = buf(), buf()
        self.out = _lib.bf_out_desc()
        self.out.means.ptr, self.out.means.sB, self.out.means.sT, self.out.means.sE = buf(), T * n, n, 1
        self.workspace = buf()
        self.B, self.T, self.workspace_bytes = B, T, 4096 * 4
        self.pointers = {"model": True, "y": True, "carry": True, "out": True, "workspace": True}

    def run(self, lib):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        ws = self.workspace if self.pointers["workspace"] else None
        code = lib.bf_kalman_filter_pscan_f32(ref("model"), ref("y"), self.B, self.T, ref("carry"), ref("out"), ws,
                                              self.workspace_bytes, None)
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
    return lambda c: setattr(getattr(c.out, name), "ptr", c.keep[0].ctypes.data)


NULL_ARGUMENT = (EINVAL, "NULL argument")
BT = "B and T must be positive (B=%d, T=%d)"
DIMS = "parallel kalman filter: (n=%d, m=%d) is not compiled in (register kernels for n = 1..6, m = 1..4; the scan needs scratch from n = 7)"
CONSTANT = "parallel kalman filter: constant Q and R only (Q_steps=%d, R_steps=%d)"
COLLAPSED = "parallel kalman filter: collapsed streams are not produced (with one component they equal means / covs)"
# B = 4, T = 8, default block 16: one block per trajectory, 4 * 4 * 1 * (4 * 9 + 3 * 3) bytes
SMALL = "parallel kalman filter: workspace of 719 bytes is too small: B=4, T=8, block=16 need 720 bytes (bf_kalman_pscan_workspace_bytes)"

ROWS = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-y", null("y")) + NULL_ARGUMENT,
    ("null-carry", null("carry")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("null-workspace", null("workspace")) + NULL_ARGUMENT,
    ("B-zero", size("B", 0), EINVAL, BT % (0, T)),
    ("T-negative", size("T", -1), EINVAL, BT % (B, -1)),
    ("n-above-the-built-limit", model(n=7, dq=7), EUNSUPPORTED, DIMS % (7, 1)),
    ("m-above-four", model(m=5, dr=5), EUNSUPPORTED, DIMS % (3, 5)),
    ("per-step-Q", model(Q_steps=T), EUNSUPPORTED, CONSTANT % (T, 1)),
    ("per-step-R", model(R_steps=T), EUNSUPPORTED, CONSTANT % (1, T)),
    ("collapsed-mean", collapsed("coll_mean"), EUNSUPPORTED, COLLAPSED),
    ("collapsed-cov", collapsed("coll_cov"), EUNSUPPORTED, COLLAPSED),
    ("workspace-too-small", size("workspace_bytes", 719), EINVAL, SMALL),
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
    assert lib.bf_set_call_option(b"pkf_block", value) == EINVAL
    assert lib.bf_last_error().decode() == "pkf_block must be 0 or 4..4096"
    assert lib.bf_kalman_pscan_workspace_bytes(3, 1, B, T, value) == EINVAL
    assert lib.bf_last_error().decode() == f"parallel kalman filter: block length {value} is outside 4..4096"


def test_workspace_bytes_formula():
    lib = _lib.load()
    for n, m, b, t, block in [(1, 1, 1, 1, 4), (4, 2, 3, 1203, 4), (4, 2, 3, 1000, 64), (6, 4, 5, 37, 64), (2, 2, 7, 4096, 4096)]:
        blocks = -(-t // block)
        assert lib.bf_kalman_pscan_workspace_bytes(n, m, b, t, block) == 4 * b * blocks * (4 * n * n + 3 * n)
    # block = 0: the largest of ceil(B T / 65 536), the smallest s with 50 s^2 >= T, and 16; at most 4096
    for b, t, block in [(1, 5000, 16), (64, 300, 16), (1, 10 ** 6, 142), (8, 10 ** 6, 142), (64, 10 ** 5, 98), (1, 10 ** 7, 448),
                        (65536, 10 ** 4, 4096)]:
        s = next(s for s in range(1, 4097) if 50 * s * s >= t or s == 4096)
        assert block == min(max(-(-b * t // 65536), s, 16), 4096)
        blocks = -(-t // block)
        assert lib.bf_kalman_pscan_workspace_bytes(4, 2, b, t, 0) == 4 * b * blocks * (4 * 16 + 12)
    assert lib.bf_kalman_pscan_workspace_bytes(4, 2, 0, 10, 4) == EINVAL
    assert lib.bf_kalman_pscan_workspace_bytes(4, 2, 10, -1, 4) == EINVAL
    assert lib.bf_kalman_pscan_workspace_bytes(7, 2, 10, 10, 4) == EUNSUPPORTED
    assert lib.bf_kalman_pscan_workspace_bytes(4, 5, 10, 10, 4) == EUNSUPPORTED
    assert lib.bf_kalman_pscan_workspace_bytes(0, 1, 10, 10, 4) == EINVAL
    assert lib.bf_kalman_pscan_workspace_bytes(1, 1, 2 ** 20, 2 ** 20, 4) == EINVAL   # B * blocks >= 2^31
