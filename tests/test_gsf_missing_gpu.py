"""GPU parity of the Gaussian-sum filters with missing observations (``missing="nan"``: bf_gsf_ekf_missing_f32,
bf_ugsf_ukf_missing_f32) against the float32 reference of tests/gsf_missing_cases.py: the oracle's own update / reweight /
predict on the row-compacted model, step by step.  Bounds: those of tests/test_gsf_gpu.py and tests/test_ugsf_gpu.py on complete
data (1e-5 norm-wise, weights 2e-5), or four times the distance of that reference from its float64 copy where that is larger
(gsf_missing_cases.bounds; never more than 2e-4).  Measured figures: DESIGN.md 4b'."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go, models as om
from tests import gsf_missing_cases as gc

pytestmark = pytest.mark.gpu
F32 = np.float32
STREAMS = gc.STREAMS
UP = (1.0, 0.0, 0.0)


def _bfa():
    import bayesianfiltering_amd as bfa
    return bfa


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return np.ascontiguousarray(_np(t), F32).view(np.uint32)


def _filter(c, K, y=None, unscented=False, pp=None, missing="nan", **kw):
    bfa = _bfa()
    pp = c["pp"] if pp is None else pp
    y = c["gapped"] if y is None else y
    kw.setdefault("initial_means", c["init"])
    kw.setdefault("return_loglik", True)
    kw.setdefault("return_carry", True)
    if missing is not None:
        kw["missing"] = missing
    if unscented:
        return bfa.unscented_gaussian_sum_filter(pp, bfa.ParamsUKF(*UP), y, K, 1, c["inputs"], **kw)
    return bfa.gaussian_sum_filter(pp, y, K, 1, c["inputs"], **kw)


def _compare(got, ref, bound, nr=None, label=""):
    """The five streams, the log-likelihood and the carry of ``got`` = (post, ll, carry) against the reference dict."""
    post, ll, carry = got
    worst = {}
    for k in STREAMS + ("loglik",):
        g = _np(ll if k == "loglik" else getattr(post, k))[:nr]
        assert g.shape == ref[k].shape, (k, g.shape, ref[k].shape)
        assert np.isfinite(g).all(), k
        worst[k] = float(np.max(np.abs(g - ref[k]))) if k == "weights" else gc.rel_err(g, ref[k])
    # the carry is the last step of the weights and of the predicted streams (bit for bit), so it is held to the reference on
    # the scale of those streams: a norm over the last step alone would ask more of it than of the stream it is part of
    for name, g, r, k in zip(("carry_w", "carry_m", "carry_P"), carry, ref["carry"], ("weights", "predicted_means", "predicted_covariances")):
        assert np.array_equal(_bits(g), _bits(getattr(post, k)[:, :, -1])), name
        g = _np(g)[:nr]
        d = float(np.max(np.abs(g - r)))
        worst[name] = d if name == "carry_w" else d / max(float(np.max(np.abs(ref[k]))), 1e-30)
    print(label, {k: f"{v:.2e}" for k, v in worst.items()}, {k: f"{v:.2e}" for k, v in bound.items()})
    for k, v in worst.items():
        b = bound[{"carry_w": "weights", "carry_m": "predicted_means", "carry_P": "predicted_covariances"}.get(k, k)]
        assert v < b, (label, k, v, b)
    return worst


# ---- 1. extended nodes, registry models -----------------------------------------------------------------------------------
EXT = [(name, B, T, K) for name in ("bot", "l63", "sv", "l96") for (B, T, K) in ((37, 19, 3), (1, 64, 1))]


@pytest.mark.parametrize("name,B,T,K", EXT + [("bot", 1, 19, 64)])     # K = 64 at two lanes per chain: two waves per trajectory
def test_extended_registry_strided(name, B, T, K):
    c = gc.case(name, B, T, K)
    bound, _ = gc.bounds(c, K)
    _compare(_filter(c, K), c["ref"], bound, label=f"{name} B={B} T={T} K={K}")


@pytest.mark.parametrize("name", ["bot", "sv", "l96"])     # (n = 3 has no staged tiles: 32 is no multiple of 9)
def test_extended_registry_staged(name):
    """K = 4, B = 64 (a multiple of the trajectories per workgroup), T = 64: the LDS-staged emitter, forced (the call fails
    if the launch is not eligible), against the reference on the first trajectories (the fixed patterns among them) and bit
    for bit against the strided emitter on all."""
    B, T, K = 64, 64, 4
    c = gc.case(name, B, T, K, nref=5)
    bound, _ = gc.bounds(c, K)
    staged = _filter(c, K, options={"kf_emit_mode": 2})
    _compare(staged, c["ref"], bound, nr=c["nref"], label=f"{name} staged")
    strided = _filter(c, K, options={"kf_emit_mode": 0})
    for k in STREAMS:
        assert np.array_equal(_bits(getattr(staged[0], k)), _bits(getattr(strided[0], k))), k
    assert np.array_equal(_bits(staged[1]), _bits(strided[1]))
    for a, b in zip(staged[2], strided[2]):
        assert np.array_equal(_bits(a), _bits(b))


def test_lorenz96_dense_instance():
    """The (8, 4) model on the generic instance (gsf_structured = 0) beside the structure-aware one of the cases above."""
    c = gc.case("l96", 37, 19, 3)
    bound, _ = gc.bounds(c, 3)
    _compare(_filter(c, 3, options={"gsf_structured": 0}), c["ref"], bound, label="l96 dense")


# ---- 2. a fixed pattern is the reduced model --------------------------------------------------------------------------------
BEARING_FULL_NOISE = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  out[0] = atan2(x[2], x[0]) + r[0];
}
"""


def test_never_observed_component_is_the_reduced_model_extended():
    """Bearing / range with the range never observed, on the new route, against the (4, 1) bearing-only registry model on the
    existing plain route."""
    B, T, K = 5, 19, 3
    c = gc.case("bot", B, T, K)
    y = c["ys"].copy()
    y[:, :, 1] = np.nan
    got = _filter(c, K, y=y)
    red = _filter(c, K, y=np.ascontiguousarray(c["ys"][:, :, :1]), pp=gc.model("bot1", T)[1], missing=None)
    for k in STREAMS[1:]:
        assert gc.rel_err(_np(getattr(got[0], k)), _np(getattr(red[0], k))) < gc.TOL, k
    assert np.max(np.abs(_np(got[0].weights) - _np(red[0].weights))) < gc.WTOL
    assert gc.rel_err(_np(got[1]), _np(red[1])) < gc.TOL


def test_never_observed_component_is_the_reduced_model_unscented():
    """The same for the unscented bank.  The reduced model is h[o] with the WHOLE noise vector (m = 1, dr = 2, given as source):
    the sigma points of the full augmented state, as the contract says -- a (4, 1) model with dr = 1 has other points."""
    bfa = _bfa()
    nl = bfa.nonlinearities
    B, T, K = 5, 19, 3
    c = gc.case("bot", B, T, K, unscented=True)
    y = c["ys"].copy()
    y[:, :, 1] = np.nan
    got = _filter(c, K, y=y, unscented=True)
    pp1 = c["pp"]._replace(emission_function=nl.user_emission(BEARING_FULL_NOISE, 4, 1, noise_dim=2))
    red = _filter(c, K, y=np.ascontiguousarray(c["ys"][:, :, :1]), pp=pp1, unscented=True, missing=None)
    for k in STREAMS[1:]:
        assert gc.rel_err(_np(getattr(got[0], k)), _np(getattr(red[0], k))) < gc.TOL, k
    assert np.max(np.abs(_np(got[0].weights) - _np(red[0].weights))) < gc.WTOL
    assert gc.rel_err(_np(got[1]), _np(red[1])) < gc.TOL


# ---- 3. complete data: the new route against the plain one ---------------------------------------------------------------
@pytest.mark.parametrize("name,unscented", [("bot", False), ("l96", False), ("sv", False), ("bot", True), ("l96", True)])
def test_complete_data_new_route_against_plain(name, unscented):
    B, T, K = 37, 19, 3
    c = gc.case(name, B, T, K, unscented=unscented)
    new = _filter(c, K, y=c["ys"], unscented=unscented)
    old = _filter(c, K, y=c["ys"], unscented=unscented, missing=None)
    same = True
    for k in STREAMS[1:]:
        assert gc.rel_err(_np(getattr(new[0], k)), _np(getattr(old[0], k))) < gc.TOL, k
        same &= np.array_equal(_bits(getattr(new[0], k)), _bits(getattr(old[0], k)))
    assert np.max(np.abs(_np(new[0].weights) - _np(old[0].weights))) < gc.WTOL
    assert gc.rel_err(_np(new[1]), _np(old[1])) < gc.TOL
    same &= np.array_equal(_bits(new[0].weights), _bits(old[0].weights)) and np.array_equal(_bits(new[1]), _bits(old[1]))
    print(f"{name} unscented={unscented}: complete data bit-identical to the plain route: {bool(same)}")


# ---- 4. collapsed streams and per-step Q / R ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bot", "l96"])
def test_collapsed_streams_on_the_new_route(name):
    bfa = _bfa()
    B, T, K = 5, 19, 3
    c = gc.case(name, B, T, K)
    post, ll, carry, (cmean, ccov) = _filter(c, K, return_collapsed=True)
    bound, _ = gc.bounds(c, K)
    _compare((post, ll, carry), c["ref"], bound, label=f"{name} collapsed")
    for b in range(B):
        for t in range(T):
            mu, Sg = go.collapse(_np(post.means[b, :, t]).astype(np.float64), _np(post.covariances[b, :, t]).astype(np.float64),
                                 _np(post.weights[b, :, t]).astype(np.float64))
            assert gc.rel_err(_np(cmean[b, t]), mu) < 1e-5 and gc.rel_err(_np(ccov[b, t]), Sg) < 1e-5, (b, t)
    only = _filter(c, K, fields=(), return_collapsed=True, return_loglik=False, return_carry=False)
    assert np.array_equal(_bits(only[1][0]), _bits(cmean)) and np.array_equal(_bits(only[1][1]), _bits(ccov))


@pytest.mark.parametrize("name,unscented", [("bot", False), ("l63", False), ("bot", True)])
def test_per_step_covariances_on_the_new_route(name, unscented):
    B, T, K = 5, 19, 3
    c = gc.case(name, B, T, K, tv=True, unscented=unscented)
    bound, _ = gc.bounds(c, K)
    _compare(_filter(c, K, unscented=unscented), c["ref"], bound, label=f"{name} per-step Q/R unscented={unscented}")


# ---- 5. chunks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,unscented", [("bot", False), ("l96", False), ("bot", True)])
def test_chunks_through_the_carry_are_bit_identical(name, unscented):
    """The cut lies inside a gap: the second chunk opens with the wholly missing step T // 2."""
    B, T, K = 37, 19, 3
    c = gc.case(name, B, T, K, unscented=unscented)
    whole = _filter(c, K, unscented=unscented)
    cut = T // 2
    u = c["inputs"]
    parts, carry = [], None
    for lo, hi in ((0, cut), (cut, T)):
        cc = dict(c, inputs=None if u is None else u[lo:hi])
        kw = dict(initial_means=c["init"]) if carry is None else dict(carry=carry, initial_means=None)
        parts.append(_filter(cc, K, y=np.ascontiguousarray(c["gapped"][:, lo:hi]), unscented=unscented, **kw))
        carry = parts[-1][2]
    for k in STREAMS:
        joined = np.concatenate([_bits(getattr(p[0], k)) for p in parts], axis=2)
        assert np.array_equal(joined, _bits(getattr(whole[0], k))), k
    assert np.array_equal(np.concatenate([_bits(p[1]) for p in parts], axis=2), _bits(whole[1]))
    for a, b in zip(parts[-1][2], whole[2]):
        assert np.array_equal(_bits(a), _bits(b))


# ---- 6. models from source and recorded Python functions ---------------------------------------------------------------------
L63_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  const float s = th[0], r = th[1], b = th[2], dt = th[3];
  out[0] = dt * s * (x[1] - x[0]) + x[0] + q[0];
  out[1] = dt * (x[0] * r - x[1] - x[0] * x[2]) + x[1] + q[1];
  out[2] = dt * (x[0] * x[1] - b * x[2]) + x[2] + q[2];
}
"""
LIN3_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  for (int a = 0; a < 3; ++a) out[a] = th[3 * a] * x[0] + th[3 * a + 1] * x[1] + th[3 * a + 2] * x[2] + r[a];
}
"""


class _PendulumDyn(om.Fn):
    out_dim, noise_dim = 2, 2

    def value(self, x, w, u):
        return (np.array([x[0] + F32(0.05) * x[1], x[1] - F32(0.05) * F32(9.81) * np.sin(x[0])], F32) + w).astype(F32)

    def jac_x(self, x, w, u):
        return np.array([[1.0, 0.05], [-F32(0.05) * F32(9.81) * np.cos(x[0]), 1.0]], F32)

    def jac_noise(self, x, w, u):
        return np.eye(2, dtype=F32)


class _PendulumEmi(om.Fn):
    out_dim, noise_dim = 1, 1

    def value(self, x, w, u):
        return (np.array([np.sin(x[0])], F32) + w).astype(F32)

    def jac_x(self, x, w, u):
        return np.array([[np.cos(x[0]), 0.0]], F32)

    def jac_noise(self, x, w, u):
        return np.eye(1, dtype=F32)


def _user_case(po, pp, B, T, K, seed=30):
    ys = gc.simulate(po, B, T, None, seed)
    m = ys.shape[-1]
    yg = gc.gapped(ys, gc.observed_mask(B, T, m))
    n = np.asarray(po.initial_mean).size
    init = (np.asarray(po.initial_mean, F32) + 0.05 * np.random.default_rng(5).normal(size=(B, K, n))).astype(F32)
    c = dict(po=po, pp=pp, inputs=None, gapped=yg, init=init, nref=B, uparams=None)
    c["ref"] = gc.batch(gc.reference, po, yg, K, init)
    return c


@pytest.mark.parametrize("K", [1, 3])
def test_recorded_python_model_pendulum(K):
    """The README's pendulum lambdas (2, 1), recorded and compiled at first use, on a gapped series."""
    bfa = _bfa()
    m0, P0 = np.array([1.0, 0.0], F32), 0.1 * np.eye(2, dtype=F32)
    Q, R = np.diag([1e-3, 2e-2]).astype(F32), 5e-2 * np.eye(1, dtype=F32)
    f = lambda x, q, u: np.array([x[0] + 0.05 * x[1], x[1] - 0.05 * 9.81 * np.sin(x[0])]) + q
    h = lambda x, r, u: np.array([np.sin(x[0])]) + r
    po = go.ParamsNLSSM(m0, P0, _PendulumDyn(), np.zeros(2, F32), Q, _PendulumEmi(), np.zeros(1, F32), R)
    pp = bfa.ParamsNLSSM(m0, P0, f, np.zeros(2, F32), Q, h, np.zeros(1, F32), R)
    c = _user_case(po, pp, 37, 19, K)
    # the bounds tests/test_user_model_gpu.py holds this model to on complete data (Jacobians by dual numbers)
    bound = dict({k: 2e-5 for k in STREAMS[1:]}, weights=5e-5, loglik=5e-5)
    _compare(_filter(c, K), c["ref"], bound, label=f"pendulum K={K}")


@pytest.mark.parametrize("K", [1, 3])
def test_source_twin_of_a_registry_model(K):
    """Lorenz-63 + linear (3, 3) with both functions given as source, against the reference of the registry model."""
    bfa = _bfa()
    nl = bfa.nonlinearities
    po, pp, _ = gc.model("l63")
    H = po.emission_function.M
    src = pp._replace(dynamics_function=nl.user_dynamics(L63_SRC, 3, theta=[10.0, 28.0, 2.667, 0.01]),
                      emission_function=nl.user_emission(LIN3_SRC, 3, 3, theta=list(np.asarray(H, F32).ravel())))
    c = gc.case("l63", 37, 19, K)
    bound, _ = gc.bounds(c, K)
    _compare(_filter(c, K, pp=src), c["ref"], bound, label=f"l63 from source K={K}")


# ---- 7. unscented nodes -------------------------------------------------------------------------------------------------------
def _unscented_model(name, T):
    _, nl = gc._bfa()
    eye = lambda d, s=1.0: (s * np.eye(d)).astype(F32)
    if name == "sine1":      # (1, 1, 1, 1)
        return gc._pair(np.zeros(1), eye(1), om.Sine(1, 1.5), nl.sine(1, 1.5), np.zeros(1), eye(1, 0.1), om.Quadratic(1, 0.5),
                        nl.quadratic(1, 0.5), np.zeros(1), eye(1, 0.5)) + (None,)
    if name == "l63h2":      # (3, 3, 2, 2): no ahead-of-time instance, built at run time
        H = np.array([[1.0, 0.2, 0.0], [0.0, 1.0, -0.3]], F32)
        return gc._pair([0.0, 1.0, 1.05], eye(3), om.Lorenz63(), nl.lorenz63(), np.zeros(3), eye(3, 0.1), om.Linear(H),
                        nl.linear_emission(H), [0.05, -0.1], np.diag([0.5, 0.3])) + (None,)
    return gc.model(name, T)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", ["sine1", "bot", "l96", "l63h2"])
def test_unscented(name, K):
    B, T = 37, 19
    if name in ("bot", "l96"):
        c = gc.case(name, B, T, K, unscented=True)
    else:
        po, pp, _ = _unscented_model(name, T)
        c = _user_case(po, pp, B, T, K)
        c["uparams"] = go.ParamsUKF(*UP)
        c["ref"] = gc.batch(gc.reference, po, c["gapped"], K, c["init"], None, c["uparams"])
    bound, _ = gc.bounds(c, K)
    _compare(_filter(c, K, unscented=True), c["ref"], bound, label=f"unscented {name} K={K}")


# ---- 8. containment ----------------------------------------------------------------------------------------------------------
LOG_ROW_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  out[0] = x[0] + r[0];
  out[1] = log(x[1]) + r[1];
}
"""


@pytest.mark.parametrize("unscented", [False, True])
def test_nan_of_the_model_in_a_missing_row_does_not_leak(unscented):
    """Row 1 is log of a state component that stays negative: NaN in h, its Jacobian row and its sigma-point images.  While
    that row is never observed the state must equal the run of the model that has row 0 only; +-Inf in an observed entry
    poisons its own trajectory and no other."""
    bfa = _bfa()
    nl = bfa.nonlinearities
    B, T, K = 6, 19, 3
    A = np.array([[0.9, 0.1], [0.0, 0.95]], F32)
    m0, P0 = np.array([0.5, -3.0], F32), 0.05 * np.eye(2, dtype=F32)
    Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([0.1, 0.2]).astype(F32)
    pp = bfa.ParamsNLSSM(m0, P0, nl.linear_dynamics(A), np.zeros(2, F32), Q, nl.user_emission(LOG_ROW_SRC, 2, 2), np.zeros(2, F32), R)
    rng = np.random.default_rng(3)
    y = np.full((B, T, 2), np.nan, F32)
    y[:, :, 0] = 0.5 + 0.3 * rng.normal(size=(B, T))
    y[:, T // 2] = np.nan                                   # one wholly missing step
    init = (m0 + 0.05 * rng.normal(size=(B, K, 2))).astype(F32)
    c = dict(pp=pp, inputs=None, gapped=y, init=init)
    post, ll, carry = _filter(c, K, unscented=unscented)
    for k in STREAMS:
        assert np.isfinite(_np(getattr(post, k))).all(), k
    assert np.isfinite(_np(ll)).all() and all(np.isfinite(_np(x)).all() for x in carry)
    # the row-0 model with the whole noise vector (the unscented sigma points are those of the full augmented state)
    row0 = "template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {\n  out[0] = x[0] + r[0];\n}\n"
    red = _filter(dict(c, pp=pp._replace(emission_function=nl.user_emission(row0, 2, 1, noise_dim=2))), K,
                  y=np.ascontiguousarray(y[:, :, :1]), unscented=unscented)
    for k in STREAMS[1:]:
        assert gc.rel_err(_np(getattr(post, k)), _np(getattr(red[0], k))) < gc.TOL, k
    assert np.max(np.abs(_np(post.weights) - _np(red[0].weights))) < gc.WTOL
    # +-Inf in an observed entry: that trajectory is poisoned from there on, the others keep their bits
    for bad in (np.inf, -np.inf):
        y2 = y.copy()
        y2[2, 5, 0] = bad
        p2, ll2, _ = _filter(c, K, y=y2, unscented=unscented)
        assert not np.isfinite(_np(p2.means)[2, :, 5:]).any()
        others = [b for b in range(B) if b != 2]
        for k in STREAMS:
            assert np.array_equal(_bits(getattr(p2, k))[others], _bits(getattr(post, k))[others]), k
        assert np.array_equal(_bits(getattr(p2, "means"))[2, :, :5], _bits(post.means)[2, :, :5])


LP_SRC = """
template <class T> __device__ T log_prob(const T* x, const float* y, T u, const float* th) {
  const T d = y[0] - x[0];
  return -0.5f * d * d;
}
"""
DECAY_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  out[0] = 0.9f * x[0] + q[0];
}
"""


def test_handle_with_a_log_density_is_refused_by_both_entry_points():
    """A model from source whose handle carries a log-density (it needs a device to exist) is the particle filter's: the
    extended entry point answers BF_EUNSUPPORTED (not eligible for the register kernel, and no other kernel takes gaps), the
    unscented one BF_EINVAL as its plain twin does."""
    import ctypes as C
    bfa = _bfa()
    from bayesianfiltering_amd import inference as inf, _lib
    nl = bfa.nonlinearities
    one = np.eye(1, dtype=F32)
    pp = bfa.ParamsNLSSM(np.zeros(1, F32), one, nl.user_dynamics(DECAY_SRC, 1), np.zeros(1, F32), one, nl.linear_emission(one),
                         np.zeros(1, F32), one)
    k = inf._filter_call(inf._Model(pp, LP_SRC), np.zeros((4, 1), F32), 1, "K", np.zeros((1, 1), F32), one)
    lib = _lib.require_gpu()
    rc = lib.bf_gsf_ekf_missing_f32(C.byref(k.mdl.c), C.byref(k.yd), C.byref(k.ud), k.B, k.T, 1, C.byref(k.cr), C.byref(k.od), None)
    assert rc == _lib.BF_EUNSUPPORTED and "not eligible for the register kernel" in lib.bf_last_error().decode()
    up = _lib.bf_ukf_params(1.0, 0.0, 0.0)
    rc = lib.bf_ugsf_ukf_missing_f32(C.byref(k.mdl.c), C.byref(up), C.byref(k.yd), C.byref(k.ud), k.B, k.T, 1, C.byref(k.cr),
                                     C.byref(k.od), None)
    assert rc == _lib.BF_EINVAL and "log-density" in lib.bf_last_error().decode()


# ---- 9. backward passes ---------------------------------------------------------------------------------------------------------
def test_backward_passes_run_on_the_gapped_posterior():
    """The wrappers pass ``missing`` to their filter; the backward pass reads no observation: bit for bit the two-call form."""
    bfa = _bfa()
    B, T = 5, 19
    c = gc.case("l63", B, T, 1)
    pp, y = c["pp"], c["gapped"]
    im = c["init"]
    pred = ("means", "covariances", "predicted_means", "predicted_covariances")
    post = bfa.gaussian_sum_filter(pp, y, 1, initial_means=im, fields=pred, missing="nan")
    a = bfa.extended_kalman_smoother(pp, y, initial_means=im, missing="nan")
    b = bfa.rts_smoother(pp, post, extended=True)
    assert np.isfinite(_np(a.smoothed_means)).all()
    assert np.array_equal(_bits(a.smoothed_means), _bits(b.smoothed_means))
    assert np.array_equal(_bits(a.smoothed_covariances), _bits(b.smoothed_covariances))
    # the mask form of the same gaps
    a2 = bfa.extended_kalman_smoother(pp, c["ys"], initial_means=im, observed=c["mask"])
    assert np.array_equal(_bits(a2.smoothed_means), _bits(a.smoothed_means))
    # Gaussian-sum smoother and posterior sample, K = 3
    K = 3
    c3 = gc.case("l63", B, T, K)
    post3 = bfa.gaussian_sum_filter(pp, c3["gapped"], K, initial_means=c3["init"], missing="nan")
    s1 = bfa.extended_gaussian_sum_smoother(pp, c3["gapped"], K, initial_means=c3["init"], missing="nan")
    s2 = bfa.gaussian_sum_smoother(pp, post3)
    for f in s1._fields:
        x1, x2 = getattr(s1, f), getattr(s2, f)
        if x1 is not None and hasattr(x1, "cpu"):
            assert np.array_equal(_bits(x1), _bits(x2)), f
    key = bfa.PRNGKey(4)
    d1 = bfa.extended_gaussian_sum_posterior_sample(pp, c3["gapped"], K, 2, key, initial_means=c3["init"], missing="nan")
    d2 = bfa.gaussian_sum_posterior_sample(pp, post3, 2, key=key)
    t1, t2 = (d1[0] if isinstance(d1, tuple) else d1), (d2[0] if isinstance(d2, tuple) else d2)
    assert np.isfinite(_np(t1)).all() and np.array_equal(_bits(t1), _bits(t2))
