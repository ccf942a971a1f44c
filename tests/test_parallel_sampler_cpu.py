"""The parallel-in-time posterior sampler without a GPU: the algebra of its header restated in float64, what
bf_ffbs_sample_pscan_f32 refuses before its first HIP call (through ctypes with host buffers, word for word), the block option,
the workspace size against its documented formula, and the Python-side refusals that precede device work."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import common as cm
from tests import parallel_sampler_cases as psc

EINVAL, EUNSUPPORTED = _lib.BF_EINVAL, _lib.BF_EUNSUPPORTED
B, T, S = 4, 8, 2
ALGEBRA_TOL = 1e-12   # the issue's bound: float64 products of a few 1..4-dimensional matrices with entries of order one


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1.0))


@pytest.mark.parametrize("recompute", [False, True], ids=["given", "recomputed"])
@pytest.mark.parametrize("name", ["2x1", "bias", "cv"])
def test_combination_is_associative_and_suffixes_are_the_sampler(name, recompute):
    Tn, Sn = 48, 3
    a, ys, init, _ = psc.case(name, 1, Tn)
    kf = psc.kalman_f64(a, ys[0].astype(np.float64), init[0], a["P0"])
    n = kf["m"].shape[1]
    xi = np.random.default_rng(5).normal(size=(Sn, Tn, n))
    A, Qb, u = psc.terms(a)
    if recompute:   # the yardstick on the predictions the route recomputes
        pm = np.stack([A @ m + u for m in kf["m"]])
        pP = np.stack([A @ P @ A.T + Qb for P in kf["P"]])
    else:
        pm, pP = kf["pm"], kf["pP"]
    pred = (lambda t: (None, None)) if recompute else (lambda t: (pm[t], pP[t]))
    els = [psc.element(a, kf["m"][t], kf["P"][t], xi[:, t], *pred(t)) for t in range(Tn)]
    # (a (+) b) (+) c == a (+) (b (+) c), on single steps and on spans
    for i in (1, 7, 20):
        x, y, z = els[i], psc.combine(els[i + 1], els[i + 2]), els[i + 3]
        left, right = psc.combine(psc.combine(x, y), z), psc.combine(x, psc.combine(y, z))
        for l, r in zip(left, right):
            assert _rel(l, r) <= ALGEBRA_TOL
    # the suffix of the elements of steps t ... T-2 applied to the terminal draw is the sampler at t
    ref = psc.ffbs_f64(kf["m"], kf["P"], pm, pP, a["A"], xi)
    last = kf["m"][Tn - 1] + xi[:, Tn - 1] @ psc.psdchol_f64(kf["P"][Tn - 1], np.diag(kf["P"][Tn - 1])).T
    assert _rel(last, ref[:, Tn - 1]) <= ALGEBRA_TOL
    suffix = None
    for t in range(Tn - 2, -1, -1):
        suffix = els[t] if suffix is None else psc.combine(els[t], suffix)
        xt = psc.apply_span(suffix, last)
        assert _rel(xt, ref[:, t]) <= ALGEBRA_TOL
        # a sample is the span (0, x): combining with it is apply_span and leaves E exactly 0
        g = psc.combine(suffix, (np.zeros((n, n)), last))
        assert not g[0].any()
        assert _rel(g[1], xt) <= ALGEBRA_TOL
    # with a carry every step has an element, and the suffixes start from the carry
    carry = np.random.default_rng(6).normal(size=(Sn, n))
    ref = psc.ffbs_f64(kf["m"], kf["P"], pm, pP, a["A"], xi, carry=carry)
    suffix = None
    for t in range(Tn - 1, -1, -1):
        suffix = els[t] if suffix is None else psc.combine(els[t], suffix)
        assert _rel(psc.apply_span(suffix, carry), ref[:, t]) <= ALGEBRA_TOL


class Call:
    """A valid call of bf_ffbs_sample_pscan_f32 on host buffers that no row lets the library read."""

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
        self.out = _lib.bf_sample_desc()
        for s in (self.out.samples, self.out.noise):
            s.ptr, s.sB, s.sK, s.sT, s.sE = buf(), S * T * n, T * n, n, 1
        self.carry = None
        self.workspace = buf()
        self.B, self.T, self.S, self.workspace_bytes, self.block = B, T, S, 4096 * 4, 0
        self.pointers = {"model": True, "filtered": True, "out": True, "workspace": True}

    def run(self, lib):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        ws = self.workspace if self.pointers["workspace"] else None
        if self.block:
            assert lib.bf_set_call_option(b"pfs_block", self.block) == _lib.BF_OK
        code = lib.bf_ffbs_sample_pscan_f32(ref("model"), ref("filtered"), self.B, self.T, self.S,
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


def keys_too(c):
    c.out.keys = c.keep[0].ctypes.data


def misaligned(c):
    c.workspace += 1


NULL_ARGUMENT = (EINVAL, "NULL argument")
BT = "B and T must be positive (B=%d, T=%d)"
SAMPLES = "the number of samples S must be positive (S=%d)"
FILTERED = "filtered means and covariances are required"
TOGETHER = "pred_means and pred_covs are given together or not at all"
DIMS = "parallel sampler: n=%d is not compiled in (register kernels for n = 1..6, the parallel filter's limit)"
CONSTANT = "parallel sampler: constant Q only (Q_steps=%d)"
LANES = "parallel sampler: B * S * ceil(T / block) = %d * %d * %d must stay below 2^31"
# B = 4, T = 8, S = 2, default block 16: one block per trajectory, 4 * 4 * 1 * (9 + 2 * 2 * 3) bytes
SMALL = "parallel sampler: workspace of 335 bytes is too small: B=4, T=8, S=2, block=16 need 336 bytes (bf_ffbs_pscan_workspace_bytes)"
ALIGNED = "parallel sampler: workspace must be 4-byte aligned"

ROWS = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("null-workspace", null("workspace")) + NULL_ARGUMENT,
    ("no-filtered-means", no_stream("filtered", "means"), EINVAL, FILTERED),
    ("no-filtered-covs", no_stream("filtered", "covs"), EINVAL, FILTERED),
    ("no-samples", no_stream("out", "samples"), EINVAL, "the samples stream is a required output"),
    ("pred-means-alone", no_stream("filtered", "pred_covs"), EINVAL, TOGETHER),
    ("pred-covs-alone", no_stream("filtered", "pred_means"), EINVAL, TOGETHER),
    ("B-zero", size(B=0), EINVAL, BT % (0, T)),
    ("T-negative", size(T=-1), EINVAL, BT % (B, -1)),
    ("S-zero", size(S=0), EINVAL, SAMPLES % 0),
    ("S-negative", size(S=-3), EINVAL, SAMPLES % -3),
    ("too-many-lanes", size(B=2 ** 20, T=2 ** 20, block=4), EINVAL, LANES % (2 ** 20, S, 2 ** 18)),
    ("n-above-the-built-limit", model(n=7, dq=7), EUNSUPPORTED, DIMS % 7),
    ("per-step-Q", model(Q_steps=2), EUNSUPPORTED, CONSTANT % 2),
    ("workspace-too-small", size(workspace_bytes=335), EINVAL, SMALL),
    ("workspace-misaligned", misaligned, EINVAL, ALIGNED),
    ("neither-noise-nor-keys", no_stream("out", "noise"), EINVAL, "give the noise stream or the keys"),
    ("both-noise-and-keys", keys_too, EINVAL, "parallel sampler: give the noise stream or the keys, not both"),
]


@pytest.mark.parametrize("name,breaker,code,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusals_before_the_first_hip_call(name, breaker, code, message):
    lib = _lib.load()
    call = Call()
    breaker(call)
    assert call.run(lib) == (code, message)


def test_samples_per_lane_count_that_is_not_built_is_refused():
    lib = _lib.load()
    assert lib.bf_set_call_option(b"ffbs_spl", 8) == _lib.BF_OK
    assert Call().run(lib) == (EINVAL, "parallel sampler: ffbs_spl must be 0 or one of the compiled counts 1, 2, 4")


@pytest.mark.parametrize("value", [3, -1, 4097])
def test_block_length_out_of_range_is_refused(value):
    lib = _lib.load()
    assert lib.bf_set_call_option(b"pfs_block", value) == EINVAL
    assert lib.bf_last_error().decode() == "pfs_block must be 0 or 4..4096"
    assert lib.bf_set_option(b"pfs_block", value) == EINVAL
    assert lib.bf_ffbs_pscan_workspace_bytes(3, B, T, S, value) == EINVAL
    assert lib.bf_last_error().decode() == f"parallel sampler: block length {value} is outside 4..4096"


def test_workspace_bytes_formula():
    lib = _lib.load()
    for n, b, t, s, block in [(1, 1, 1, 1, 4), (4, 3, 1203, 5, 4), (4, 3, 1000, 5, 64), (6, 5, 37, 2, 64), (2, 7, 4096, 16, 4096)]:
        blocks = -(-t // block)
        assert lib.bf_ffbs_pscan_workspace_bytes(n, b, t, s, block) == 4 * b * blocks * (n * n + 2 * s * n)
    # block = 0: the largest of ceil(B ceil(S / 4) T / 65 536), the smallest r with 250 r^2 >= T, and 16; at most 4096
    for b, s, t, block in [(1, 1, 5000, 16), (64, 4, 300, 16), (1, 1, 10 ** 6, 64), (1, 16, 10 ** 6, 64), (1, 17, 10 ** 6, 77),
                           (64, 4, 10 ** 5, 98), (1024, 4, 10 ** 4, 157), (65536, 1, 256, 256), (65536, 8, 10 ** 4, 4096)]:
        r = next(r for r in range(1, 4097) if 250 * r * r >= t or r == 4096)
        assert block == min(max(-(-b * -(-s // 4) * t // 65536), r, 16), 4096)
        blocks = -(-t // block)
        assert lib.bf_ffbs_pscan_workspace_bytes(4, b, t, s, 0) == 4 * b * blocks * (16 + 8 * s)
    assert lib.bf_ffbs_pscan_workspace_bytes(4, 0, 10, 1, 4) == EINVAL
    assert lib.bf_ffbs_pscan_workspace_bytes(4, 10, -1, 1, 4) == EINVAL
    assert lib.bf_ffbs_pscan_workspace_bytes(4, 10, 10, 0, 4) == EINVAL
    assert lib.bf_ffbs_pscan_workspace_bytes(7, 10, 10, 1, 4) == EUNSUPPORTED
    assert lib.bf_ffbs_pscan_workspace_bytes(0, 10, 10, 1, 4) == EINVAL
    assert lib.bf_ffbs_pscan_workspace_bytes(1, 2 ** 20, 2 ** 20, 1, 4) == EINVAL    # B * S * blocks >= 2^31
    assert lib.bf_ffbs_pscan_workspace_bytes(1, 2 ** 5, 2 ** 20, 2 ** 8, 4) == EINVAL    # 2^5 * 2^8 * 2^18 = 2^31
    assert lib.bf_last_error().decode() == LANES % (2 ** 5, 2 ** 8, 2 ** 18)
    assert lib.bf_ffbs_pscan_workspace_bytes(1, 2 ** 4, 2 ** 20, 2 ** 8, 4) == 4 * 2 ** 4 * 2 ** 18 * (1 + 2 * 2 ** 8)


def _posterior(B_, K, T_, n, pred=True):
    import torch
    import bayesianfiltering_amd as bfa
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return bfa.PosteriorGaussianSumFiltered(None, z(B_, K, T_, n), z(B_, K, T_, n, n), z(B_, K, T_, n) if pred else None,
                                            z(B_, K, T_, n, n) if pred else None)


def test_python_refusals_that_precede_device_work():
    import torch
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    lin = cm.product_params(cm.cv_model_arrays())
    key = bfa.PRNGKey(0)
    post = _posterior(2, 1, 8, 4)
    ext = bfa.ParamsNLSSM(np.zeros(3, np.float32), np.eye(3, dtype=np.float32), nl.lorenz63(), np.zeros(3, np.float32),
                          np.eye(3, dtype=np.float32), nl.linear_emission(np.eye(3, dtype=np.float32)),
                          np.zeros(3, np.float32), np.eye(3, dtype=np.float32))
    with pytest.raises(ValueError, match="must be linear_dynamics for the parallel sampler"):
        bfa.parallel_posterior_sample(ext, _posterior(2, 1, 8, 3), 2, key=key)
    for refused in ({"extended": True}, {"uparams": (1.0, 2.0, 0.0)}, {"inputs": np.zeros((2, 8, 1), np.float32)}):
        with pytest.raises(ValueError, match="does not take " + next(iter(refused))):
            bfa.parallel_posterior_sample(lin, post, 2, key=key, **refused)
    with pytest.raises(TypeError):
        bfa.parallel_posterior_sample(lin, post, 2, key=key, cross_covariances=True)
    with pytest.raises(ValueError, match="one component"):
        bfa.parallel_posterior_sample(lin, _posterior(2, 3, 8, 4), 2, key=key)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="num_samples must be positive"):
            bfa.parallel_posterior_sample(lin, post, bad, key=key)
    with pytest.raises(ValueError, match="exactly one"):
        bfa.parallel_posterior_sample(lin, post, 2)
    with pytest.raises(ValueError, match="exactly one"):
        bfa.parallel_posterior_sample(lin, post, 2, key=key, noise=torch.zeros(2, 2, 8, 4))
    with pytest.raises(ValueError, match=r"noise has shape \(2, 3, 8, 4\), expected \(2, 2, 8, 4\)"):
        bfa.parallel_posterior_sample(lin, post, 2, noise=torch.zeros(2, 3, 8, 4))
    with pytest.raises(ValueError, match="noise has shape"):
        bfa.parallel_posterior_sample(lin, post, 2, noise=torch.zeros(2, 8, 4))
    with pytest.raises(ValueError, match="workspace must be a contiguous uint8 tensor"):
        bfa.parallel_posterior_sample(lin, post, 2, key=key, workspace=torch.zeros(4096, dtype=torch.float32))
    with pytest.raises(ValueError, match="together"):
        bfa.parallel_posterior_sample(lin, post._replace(predicted_means=None), 2, key=key)
