"""Gaussian-sum backward passes, no GPU: the float64 statement (``gs_smooth_f64``) pinned against the exact dense mixture
of a linear model with a K-component prior, the float32 restatement of the component draw, and every refusal the three
new C entry points and the Python functions make before any device work (pointers that are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

from bayesianfiltering_amd import _lib
from tests import gaussian_sum_backward_cases as gc

EINVAL, EUNSUPPORTED = _lib.BF_EINVAL, _lib.BF_EUNSUPPORTED


# ---- the float64 statement against the dense mixture ----------------------------------------------------------------------
@pytest.mark.parametrize("n,m,K,T,seed", [(4, 2, 3, 16, 300), (3, 2, 5, 24, 310)])
def test_gs_smooth_f64_matches_exact_dense_mixture(n, m, K, T, seed):
    a, ys, m_inits = gc.mixture_case(n, m, K, T, seed)
    chains = [gc.kalman_loglik_f64(a, ys, m_inits[k], a["P0"]) for k in range(K)]
    st = {k: np.stack([c[0][k] for c in chains]) for k in ("m", "P", "pm", "pP")}
    ll = np.array([c[1] for c in chains])
    w_filter = np.exp(ll - ll.max())
    w_filter /= w_filter.sum()                       # the weight recursion from 1 / K, at its last step
    w, dm, dP, dmu, dS = gc.dense_mixture(a, ys, m_inits, a["P0"])
    assert np.max(np.abs(w_filter - w)) <= 1e-9      # the smoothed weights ARE the final filter weights
    ms, Ps, _, mu, Sigma = gc.gs_smooth_f64(st["m"], st["P"], st["pm"], st["pP"], a["A"], w_filter)
    for got, ref in ((ms, dm), (Ps, dP), (mu, dmu), (Sigma, dS)):
        assert np.max(np.abs(got - ref)) <= 1e-9 * max(1.0, np.max(np.abs(ref)))
    assert np.ptp(w) > 1e-3                          # a mixture, not one surviving component


# ---- the component draw ------------------------------------------------------------------------------------------------------
def test_draw_components_f32():
    f = gc.draw_components_f32
    v = np.array([[0.0, 0.3, 0.999999]], np.float32)
    assert f([[0.0, 1.0, 0.0]], v).tolist() == [[1, 1, 1]]                  # one-hot
    assert f([[0.2, 0.5, 0.3]], [[0.0]]).tolist() == [[0]]                  # v = 0: the first component with weight
    assert f([[0.0, 0.5, 0.5]], [[0.0, 0.49, 0.5]]).tolist() == [[1, 1, 2]]   # a zero leading weight is never drawn
    assert f([[2.0, 5.0, 3.0]], [[0.1, 0.2, 0.69, 0.7, 0.95]]).tolist() == [[0, 1, 1, 2, 2]]   # unnormalised
    assert f([[np.nan, 0.5]], v).tolist() == [[-1, -1, -1]]
    assert f([[0.0, 0.0]], v).tolist() == [[-1, -1, -1]]
    assert f([[np.inf, 1.0]], v).tolist() == [[-1, -1, -1]]
    one = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert f([[0.25, 0.25, 0.5]], [[one]]).tolist() == [[2]]
    assert f([[0.5, 0.5, 0.0]], [[one]]).tolist() == [[1]]                  # a zero trailing weight is never drawn
    # a uniform of exactly 1 (outside the contract) finds no c_j above c_{K-1}: the draw is clamped to K - 1
    assert f([[0.1, 0.2, 0.3]], [[1.0]]).tolist() == [[2]]
    # rows are independent
    assert f([[1.0, 0.0], [np.nan, 1.0], [0.0, 1.0]], [[0.5], [0.5], [0.5]]).tolist() == [[0], [-1], [1]]


# ---- refusals of bf_gs_smoother_f32 before its first HIP call ------------------------------------------------------------------
B, T, K, S = 4, 8, 3, 2
LORENZ63, LINEAR_EMISSION = 2, 0


class Call:
    """A valid call of bf_gs_smoother_f32 -- or, ``sampler=True``, of bf_gs_sample_f32 -- (Lorenz-63, n = 3) over host
    buffers that no row lets the library read."""

    def __init__(self, unscented=False, sampler=False):
        self.keep = keep = []

        def fp(a):
            keep.append(np.ascontiguousarray(a, np.float32))
            return keep[-1].ctypes.data_as(_lib._FP)

        def stream(s):
            keep.append(np.zeros(64, np.float32))
            s.ptr, s.sB, s.sK, s.sT, s.sE = keep[-1].ctypes.data, 1, 1, 1, 1

        self.filtered = _lib.bf_out_desc()
        for name in ("means", "covs", "pred_means", "pred_covs"):
            stream(getattr(self.filtered, name))
        self.B, self.T, self.K, self.S = B, T, K, S
        self.sampler = sampler
        self.options = {}
        self.u = _lib.bf_cstream()
        self.uparams = _lib.bf_ukf_params(1.0, 2.0, 0.0)
        self.unscented = unscented
        eye = np.eye(3, dtype=np.float32)
        m = self.model = _lib.bf_model()
        m.dyn_id, m.emi_id, m.n, m.dq, m.m, m.dr = LORENZ63, LINEAR_EMISSION, 3, 3, 2, 2
        m.dyn_theta, m.n_dyn_theta = fp([10.0, 28.0, 2.667, 0.01]), 4
        m.emi_theta, m.n_emi_theta = fp(np.concatenate([np.eye(2, 3).ravel(), np.eye(2).ravel()])), 10
        m.Q, m.R, m.Q_steps, m.R_steps = fp(eye), fp(np.eye(2)), 1, 1
        if sampler:
            self.out = _lib.bf_gs_sample_desc()
            stream(self.out.samples)
            stream(self.out.noise)
            self.out.weights = self.out.comp_noise = self.host_ptr()
            self.carry = _lib.bf_sample_carry()
        else:
            self.out = _lib.bf_gs_smooth_desc()
            for name in ("means", "covs", "cross_covs", "coll_mean", "coll_cov"):
                stream(getattr(self.out, name))
            self.out.coll_mean.sB, self.out.coll_mean.sT = T * 3, 3          # contiguous [B][T][E]
            self.out.coll_cov.sB, self.out.coll_cov.sT = T * 9, 9
            self.out.weights = self.host_ptr()
            self.carry = _lib.bf_smooth_carry()
        self.pointers = {"model": True, "filtered": True, "out": True}

    def host_ptr(self):
        return self.keep[0].ctypes.data

    def run(self, lib):
        ref = lambda name: C.byref(getattr(self, name)) if self.pointers[name] else None
        for k, v in self.options.items():
            assert lib.bf_set_call_option(k, v) == _lib.BF_OK
        fn, sizes = (lib.bf_gs_sample_f32, (self.K, self.S)) if self.sampler else (lib.bf_gs_smoother_f32, (self.K,))
        code = fn(ref("model"), C.byref(self.uparams) if self.unscented else None, C.byref(self.u), ref("filtered"), self.B, self.T,
                  *sizes, C.byref(self.carry), ref("out"), None)
        return code, lib.bf_last_error().decode()


def null(name):
    return lambda c: c.pointers.__setitem__(name, False)


def size(name, value):
    return lambda c: setattr(c, name, value)


def model(**fields):
    return lambda c: [setattr(c.model, k, v) for k, v in fields.items()]


def no_stream(*names):
    return lambda c: [setattr(getattr(c.filtered, name), "ptr", None) for name in names]


def no_out(*names):
    return lambda c: [setattr(getattr(c.out, name), "ptr", None) for name in names]


def both(*steps):
    return lambda c: [s(c) for s in steps]


def option(name, value):
    return lambda c: c.options.__setitem__(name, value)


def carry(name):
    return lambda c: setattr(c.carry, name, c.host_ptr())


def strided(name):
    return lambda c: setattr(getattr(c.out, name), "sT", 1)


NULL_ARGUMENT = (EINVAL, "NULL argument")
DIMENSION = (EINVAL, "non-positive model dimension")
BT = "B and T must be positive (B=%d, T=%d)"
NEED_PRED = (EINVAL, "the Gaussian-sum smoother needs the predicted means and covariances (pred_means, pred_covs)")
PAIR = (EINVAL, "out->means and out->covs are given together or not at all")
ALL_OUT = ("means", "covs", "cross_covs", "coll_mean", "coll_cov")
COLL_ALONE_K = ("Gaussian-sum smoother: collapsed moments alone serve K <= 64 components and n <= 6, where the fused instances "
                "build without scratch (K = 65, n = 3); ask for the per-component streams too")
COLL_ALONE_GENERIC = ("Gaussian-sum smoother: collapsed moments alone serve n <= 6 on the register kernel (n = 3, force_generic); "
                      "ask for the per-component streams too")
CONTIG = "out->coll_mean / coll_cov must be contiguous [B][T][E] for K > 64, n > 6 and force_generic"
ROWS = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("flags", model(flags=_lib.BF_MODEL_PREDICT_FIRST), EUNSUPPORTED,
     "the {route} Gaussian-sum smoother needs the JAX path's update -> predict streams (flags = 0)"),
    ("B-zero", size("B", 0), EINVAL, BT % (0, T)),
    ("T-negative", size("T", -2), EINVAL, BT % (B, -2)),
    ("K-zero", size("K", 0), EINVAL, "K must be at least 1 (K=0)"),
    ("K-negative", size("K", -5), EINVAL, "K must be at least 1 (K=-5)"),
    ("K-huge", size("K", 1 << 31), EINVAL, "K too large (K=2147483648)"),
    ("n-zero", model(n=0)) + DIMENSION,
    ("dr-negative", model(dr=-1)) + DIMENSION,
    ("no-Q", model(Q=None), EINVAL, "Q and R are required"),
    ("no-filtered-means", no_stream("means"), EINVAL, "filtered means and covariances are required"),
    ("no-filtered-covs", no_stream("covs"), EINVAL, "filtered means and covariances are required"),
    ("no-predictions", no_stream("pred_means", "pred_covs")) + NEED_PRED,
    ("pred-means-only", no_stream("pred_covs")) + NEED_PRED,
    ("means-without-covs", no_out("covs")) + PAIR,
    ("covs-without-means", no_out("means")) + PAIR,
    ("cross-covs-alone", no_out("means", "covs"), EINVAL, "out->cross_covs needs out->means and out->covs"),
    ("no-output", no_out(*ALL_OUT), EINVAL, "at least one output is required: out->means / covs or out->coll_mean / coll_cov"),
    ("collapsed-without-weights", lambda c: setattr(c.out, "weights", None), EINVAL,
     "out->weights is required with collapsed outputs (coll_mean, coll_cov)"),
    ("carry-m-in-only", carry("m_in"), EINVAL, "carry.m_in and carry.P_in are given together or not at all"),
    ("carry-P-out-only", carry("P_out"), EINVAL, "carry.m_out and carry.P_out are given together or not at all"),
    ("collapsed-alone-K-65", both(size("K", 65), no_out("means", "covs", "cross_covs")), EUNSUPPORTED, COLL_ALONE_K),
    ("collapsed-alone-generic", both(option(b"force_generic", 1), no_out("means", "covs", "cross_covs")), EUNSUPPORTED, COLL_ALONE_GENERIC),
    ("strided-collapsed-K-65", both(size("K", 65), strided("coll_mean")), EUNSUPPORTED, CONTIG),
    ("strided-collapsed-generic", both(option(b"force_generic", 1), strided("coll_cov")), EUNSUPPORTED, CONTIG),
]
EXTENDED = ROWS + [
    ("dynamics-from-source-no-handle", model(dyn_id=_lib.BF_FN_USER), EUNSUPPORTED,
     "the extended Gaussian-sum smoother serves functions given as source through bf_model.user (bf_user_model_create); it is NULL"),
    ("registry-theta-layout", model(n_dyn_theta=3), EINVAL, "lorenz63: n = dq = 3, theta = (sigma, rho, beta, dt)"),
    ("staged-strided-layout", option(b"rts_load_mode", 2), EINVAL,
     "rts_load_mode = 2 serves per-component output on the contiguous reference layout only"),
]
NO_SOURCE = (EUNSUPPORTED, "the unscented Gaussian-sum smoother serves registry dynamics; functions given as source are not supported")
UNSCENTED = ROWS + [
    ("handle", lambda c: setattr(c.model, "user", c.host_ptr())) + NO_SOURCE,
    ("dynamics-from-source", model(dyn_id=_lib.BF_FN_USER)) + NO_SOURCE,
    ("alpha-zero", lambda c: setattr(c.uparams, "alpha", 0.0), EINVAL, "ParamsUKF.alpha must be positive"),
    ("lambda-cancels-L", lambda c: setattr(c.uparams, "kappa", -6.0), EINVAL,
     "ParamsUKF: L + lambda = alpha^2 (n + dq + kappa) must be positive and finite (alpha = 1, kappa = -6, n + dq = 6)"),
    ("staged", option(b"rts_load_mode", 2), EINVAL, "rts_load_mode = 2 is not offered on the unscented route"),
]


def _cases():
    for route, rows in (("extended", EXTENDED), ("unscented", UNSCENTED)):
        for row in rows:
            yield pytest.param(route, row, id=f"{route}-{row[0]}")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("route, row", _cases())
def test_gs_smoother_refusal_code_and_message(lib, route, row):
    _, break_it, code, message = row
    call = Call(unscented=route == "unscented")
    break_it(call)
    assert call.run(lib) == (code, message.format(route=route))


# ---- refusals of bf_gs_sample_f32 before its first HIP call -------------------------------------------------------------------
def sample_field(**fields):
    def go(c):
        for k, v in fields.items():
            if k in ("samples", "noise"):
                getattr(c.out, k).ptr = None
            else:
                setattr(c.out, k, c.host_ptr() if v else None)
    return go


S_MSG = "the number of samples S must be positive (S=%d)"
COMP_SOURCE = (EINVAL, "give exactly one of out->comp_noise and out->comp_keys (or out->comp_in)")
SAMPLER_ROWS = [
    ("null-model", null("model")) + NULL_ARGUMENT,
    ("null-filtered", null("filtered")) + NULL_ARGUMENT,
    ("null-out", null("out")) + NULL_ARGUMENT,
    ("flags", model(flags=_lib.BF_MODEL_PREDICT_FIRST), EUNSUPPORTED,
     "the {route} Gaussian-sum sampler needs the JAX path's update -> predict streams (flags = 0)"),
    ("n-zero", model(n=0)) + DIMENSION,
    ("no-R", model(R=None), EINVAL, "Q and R are required"),
    ("B-negative", size("B", -4), EINVAL, BT % (-4, T)),
    ("T-zero", size("T", 0), EINVAL, BT % (B, 0)),
    ("K-zero", size("K", 0), EINVAL, "K must be at least 1 (K=0)"),
    ("K-huge", size("K", 1 << 31), EINVAL, "K too large (K=2147483648)"),
    ("S-zero", size("S", 0), EINVAL, S_MSG % 0),
    ("S-negative", size("S", -3), EINVAL, S_MSG % -3),
    ("no-filtered-covs", no_stream("covs"), EINVAL, "filtered means and covariances are required"),
    ("no-predictions", no_stream("pred_means", "pred_covs"), EINVAL,
     "the Gaussian-sum sampler needs the predicted means and covariances (pred_means, pred_covs)"),
    ("pred-covs-only", no_stream("pred_means"), EINVAL,
     "the Gaussian-sum sampler needs the predicted means and covariances (pred_means, pred_covs)"),
    ("no-samples", sample_field(samples=None), EINVAL, "the samples stream is a required output"),
    ("no-noise-no-keys", sample_field(noise=None), EINVAL, "give the noise stream or the keys"),
    ("keys-too-many-values", both(sample_field(noise=None, keys=True), size("S", 1 << 20), size("T", 1 << 10)), EINVAL,
     "drawing from keys serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T"),
    ("S-too-large", size("S", 1 << 30), EINVAL, "S too large"),
    ("no-weights", sample_field(weights=False), EINVAL, "out->weights is required to draw the components (or give out->comp_in)"),
    ("comp-noise-and-comp-keys", sample_field(comp_keys=True)) + COMP_SOURCE,
    ("no-comp-noise-no-comp-keys", sample_field(comp_noise=False)) + COMP_SOURCE,
    ("grid-too-large", size("B", 1 << 41), EINVAL, "Gaussian-sum sampler: B x S too large for one launch"),
    ("grid-too-large-generic", both(size("B", 1 << 30), option(b"force_generic", 1)), EINVAL,
     "Gaussian-sum sampler: B x K too large for the run-time-dimension kernel"),
]
SAMPLER_EXTENDED = SAMPLER_ROWS + [
    ("dynamics-from-source-no-handle", model(dyn_id=_lib.BF_FN_USER), EUNSUPPORTED,
     "the extended Gaussian-sum sampler serves functions given as source through bf_model.user (bf_user_model_create); it is NULL"),
    ("registry-theta-layout", model(n_dyn_theta=3), EINVAL, "lorenz63: n = dq = 3, theta = (sigma, rho, beta, dt)"),
    # 4 (5 n (n + 1) + 3 n + S + 3 n) bytes: five matrices, three vectors, the sample indices, one sample per buffer
    ("lds-S-generic", both(size("S", 50000), option(b"force_generic", 1)), EUNSUPPORTED,
     "Gaussian-sum sampler: n = 3 with S = 50000 samples needs 200312 bytes of LDS (160 KiB per workgroup)"),
]
SAMPLER_UNSCENTED = SAMPLER_ROWS + [
    # ... plus the root's matrix n (n + 1) and vectors (3 * 4 + 4 * 4 floats at n = 3)
    ("lds-S-generic", both(size("S", 50000), option(b"force_generic", 1)), EUNSUPPORTED,
     "Gaussian-sum sampler: n = 3 with S = 50000 samples needs 200472 bytes of LDS (160 KiB per workgroup)"),

    ("handle", lambda c: setattr(c.model, "user", c.host_ptr()), EUNSUPPORTED,
     "the unscented Gaussian-sum sampler serves registry dynamics; functions given as source are not supported"),
    ("alpha-negative", lambda c: setattr(c.uparams, "alpha", -1.0), EINVAL, "ParamsUKF.alpha must be positive"),
]


def _sampler_cases():
    for route, rows in (("extended", SAMPLER_EXTENDED), ("unscented", SAMPLER_UNSCENTED)):
        for row in rows:
            yield pytest.param(route, row, id=f"{route}-{row[0]}")


@pytest.mark.parametrize("route, row", _sampler_cases())
def test_gs_sampler_refusal_code_and_message(lib, route, row):
    _, break_it, code, message = row
    call = Call(unscented=route == "unscented", sampler=True)
    break_it(call)
    assert call.run(lib) == (code, message.format(route=route))


def test_gs_sampler_accepts_comp_in_without_weights(lib):
    """with comp_in nothing is drawn: weights, comp_noise and comp_keys may all be absent (the call then reaches the device
    check of the launch; without a GPU that is the first HIP call's error, not a refusal of the arguments)"""
    call = Call(sampler=True)
    call.out.weights = call.out.comp_noise = None
    call.out.comp_in = call.host_ptr()
    call.S = 0   # stop at the next argument check
    assert call.run(lib) == (EINVAL, S_MSG % 0)
    call.S = 1 << 30
    assert call.run(lib) == (EINVAL, "S too large")


def test_gs_abi_check_and_version(lib):
    assert lib.bf_version() == 210
    sizes = C.sizeof(_lib.bf_gs_smooth_desc), C.sizeof(_lib.bf_gs_sample_desc)
    assert lib.bf_gs_abi_check(*sizes) == _lib.BF_OK
    assert lib.bf_gs_abi_check(0, 0) == _lib.BF_OK
    assert lib.bf_gs_abi_check(3 * C.sizeof(_lib.bf_stream), 0) == EINVAL
    assert b"bf_gs_smooth_desc" in lib.bf_last_error()
    assert lib.bf_gs_abi_check(0, C.sizeof(_lib.bf_sample_desc)) == EINVAL
    assert b"bf_gs_sample_desc" in lib.bf_last_error()
    assert sizes == (5 * C.sizeof(_lib.bf_stream) + 8, 2 * C.sizeof(_lib.bf_stream) + 6 * 8)


def test_struct_size_agrees_with_a_c_compiler(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bayesfilt.h"\nint main(void) { printf("%zu %zu\\n", sizeof(bf_gs_smooth_desc), '
                   'sizeof(bf_gs_sample_desc)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [C.sizeof(_lib.bf_gs_smooth_desc), C.sizeof(_lib.bf_gs_sample_desc)]


# ---- Python argument checks that need no device ------------------------------------------------------------------------------
def _posterior(B, K, T, n, pred=True, weights=True):
    import torch
    import bayesianfiltering_amd as bfa
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return bfa.PosteriorGaussianSumFiltered(z(B, K, T) if weights else None, z(B, K, T, n), z(B, K, T, n, n),
                                            z(B, K, T, n) if pred else None, z(B, K, T, n, n) if pred else None)


def _lorenz_params():
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    e3 = np.eye(3, dtype=np.float32)
    return bfa.ParamsNLSSM(np.zeros(3, np.float32), e3, nl.lorenz63(), np.zeros(3, np.float32), e3, nl.linear_emission(e3),
                           np.zeros(3, np.float32), e3)


def test_python_validation_without_device():
    import bayesianfiltering_amd as bfa
    p = _lorenz_params()
    with pytest.raises(ValueError, match="components, collapsed moments or both"):
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 3), components=False, collapsed=False)
    with pytest.raises(ValueError, match="cross_covariances needs components"):
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 3), components=False, cross_covariances=True)
    with pytest.raises(ValueError, match="predicted"):
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 3, pred=False))
    with pytest.raises(ValueError, match="predicted"):
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 3, pred=False), uparams=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="state dimension"):
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 4))
    with pytest.raises(ValueError, match="covariances have shape"):
        post = _posterior(2, 3, 8, 3)
        bfa.gaussian_sum_smoother(p, post._replace(covariances=post.covariances[:, :2]))
    with pytest.raises(ValueError, match="float32 device tensors"):   # host tensors: refused before the library is asked for a GPU
        bfa.gaussian_sum_smoother(p, _posterior(2, 3, 8, 3))
    # the sampler
    s3 = lambda **kw: bfa.gaussian_sum_posterior_sample(p, _posterior(2, 3, 8, 3), 4, **kw)
    import torch
    zn, zc, zi = torch.zeros(2, 4, 8, 3), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="num_samples must be positive"):
        bfa.gaussian_sum_posterior_sample(p, _posterior(2, 3, 8, 3), 0, key=bfa.PRNGKey(0))
    with pytest.raises(ValueError, match="components or component_noise, not both"):
        s3(noise=zn, components=zi, component_noise=zc)
    with pytest.raises(ValueError, match="key is required"):
        s3()
    with pytest.raises(ValueError, match="key is required"):
        s3(noise=zn)
    with pytest.raises(ValueError, match="key is required"):
        s3(component_noise=zc)
    with pytest.raises(ValueError, match="key would not be read"):
        s3(key=bfa.PRNGKey(0), noise=zn, components=zi)
    with pytest.raises(ValueError, match="the carry holds the components"):
        s3(noise=zn, component_noise=zc, carry=bfa.GaussianSumSamplerCarry(torch.zeros(2, 4, 3), zi))
    with pytest.raises(ValueError, match="noise has shape"):
        s3(noise=zn[:, :2], components=zi)
    with pytest.raises(ValueError, match="predicted"):
        bfa.gaussian_sum_posterior_sample(p, _posterior(2, 3, 8, 3, pred=False), 4, key=bfa.PRNGKey(0))
    with pytest.raises(ValueError, match="float32 device tensors"):
        s3(noise=zn, components=zi)
    # the one-component passes keep refusing K > 1
    with pytest.raises(ValueError, match="one component"):
        bfa.rts_smoother(p, _posterior(2, 3, 8, 3))
    with pytest.raises(ValueError, match="one component"):
        bfa.posterior_sample(p, _posterior(2, 3, 8, 3), key=bfa.PRNGKey(0))
