"""Rauch-Tung-Striebel smoothing on the HIP engine: the reference's ``SSM.smoother(params, emissions, inputs)``
(gaussfiltax/ssm.py:55-61, 282-300), p(z_t | y_{1:T}), for the Kalman, extended-Kalman and unscented Kalman filters.

The backward pass consumes the streams a filter already wrote (``kalman_filter`` / ``gaussian_sum_filter`` /
``unscented_gaussian_sum_filter`` with one component) and runs in ``bf_rts_smoother_f32`` / ``bf_eks_smoother_f32`` /
``bf_uks_smoother_f32`` (include/bayesfilt.h, csrc/rts_smoother.hpp, where the recursion is stated).  PyTorch only allocates and passes device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Optional, Any

import numpy as np

from . import _lib
from .inference import (_torch, _dev_f32, _host_f32, _fp, _alloc_stream, _stream_desc, _time_varying, _Model, _param_dims,
                        _check_out_tensor, kalman_filter, gaussian_sum_filter, unscented_gaussian_sum_filter, ParamsUKF)
from .nonlinearities import DYN_LINEAR, DeviceFunction, require_device_function


class PosteriorGaussianSmoothed(NamedTuple):
    """Filtered and smoothed marginals (dynamax's field names).  Arrays are shaped like ``kalman_filter``'s: (1, T, ...)
    for one trajectory, (B, 1, T, ...) for a batch.  ``smoothed_cross_covariances`` holds Cov(x_t, x_{t+1} | y_{1:T})
    for t < T-1 (T-1 steps), or None unless requested."""
    filtered_means: Optional[Any] = None
    filtered_covariances: Optional[Any] = None
    smoothed_means: Optional[Any] = None
    smoothed_covariances: Optional[Any] = None
    smoothed_cross_covariances: Optional[Any] = None


class SmootherCarry(NamedTuple):
    """Smoothed state at one step, contiguous (B, n) / (B, n, n): what a backward chunk hands to the chunk before it."""
    means: Any
    covariances: Any


class _LinearDynamics:
    """bf_lgssm holding the dynamics half of a linear model (the smoother never reads the emission)."""

    def __init__(self, params, f):
        self.n, self.dq = f.out_dim, f.noise_dim
        self.A, self.G = np.ascontiguousarray(f.M), np.ascontiguousarray(f.N)
        self.q0 = _host_f32(params.dynamics_noise_bias).reshape(self.dq)
        self.Q, self.Q_steps = _time_varying(params.dynamics_noise_covariance, self.dq)
        self.H = np.zeros((1, self.n), np.float32)
        self.R = np.ones((1, 1), np.float32)
        c = _lib.bf_lgssm()
        c.n, c.dq, c.m, c.dr = self.n, self.dq, 1, 1
        c.A, c.G, c.H, c.Q, c.R, c.q0 = _fp(self.A), _fp(self.G), _fp(self.H), _fp(self.Q), _fp(self.R), _fp(self.q0)
        c.Q_steps, c.R_steps = self.Q_steps, 1
        self.c = c


def _batched(x, event_dims):
    """(K, T, *ev) -> (1, K, T, *ev); (B, K, T, *ev) unchanged."""
    if x is None:
        return None
    return x.unsqueeze(0) if x.dim() == 2 + event_dims else x


def _ukf_params(uparams, extended):
    """``uparams`` (a :class:`ParamsUKF` or a 3-tuple) as the C struct; it excludes ``extended=True``."""
    if extended:
        raise ValueError("uparams selects the unscented route; it cannot be combined with extended=True")
    if not isinstance(uparams, ParamsUKF):
        uparams = ParamsUKF(*uparams)
    return _lib.bf_ukf_params(float(uparams.alpha), float(uparams.beta), float(uparams.kappa))


def _inputs_desc(inputs, B, T, dev, keep):
    """bf_cstream of the filter's inputs ((T,), (T, d) or (B, T, d); None = zeros)."""
    ud = _lib.bf_cstream()
    if inputs is not None:
        u = _dev_f32(inputs, dev)
        if u.dim() == 1:
            u = u.reshape(1, T, 1)
        elif u.dim() == 2:
            u = u.reshape(1, T, -1)
        if u.shape[1] != T or u.shape[0] not in (1, B):
            raise ValueError(f"inputs must be (T,), (T,d) or (B,T,d); got {tuple(u.shape)}")
        keep.append(u)
        ud.ptr, ud.sB, ud.sT, ud.sE = u.data_ptr(), (u.stride(0) if u.shape[0] == B else 0), u.stride(1), 1
    return ud


def rts_smoother(params, posterior, *, inputs=None, carry=None, cross_covariances: bool = False, layout: str = "reference",
                 out=None, return_carry: bool = False, extended: Optional[bool] = None, uparams=None, device="cuda",
                 options=None):
    """Smooth the filtered posterior ``posterior`` (a ``PosteriorGaussianSumFiltered`` of ``kalman_filter``, or of
    ``gaussian_sum_filter`` with one component) backwards in time on the device.

    Linear dynamics (``linear_dynamics``) run ``bf_rts_smoother_f32``; without ``predicted_means`` /
    ``predicted_covariances`` in ``posterior`` the predictions are recomputed from the filtered streams.  Other registry
    dynamics, ``nonlinearities.user_dynamics`` source and plain Python functions (recorded at the model's dimensions, as
    the filters record them) run ``bf_eks_smoother_f32`` (F_t = the Jacobian at the filtered mean and ``inputs``, as the
    filter's predict used it; by forward-mode dual numbers for functions from source, in kernels built on first use) and
    need the predicted streams; ``extended=True`` sends a linear model there too.
    ``uparams`` (a :class:`ParamsUKF` or a 3-tuple): the posterior is ``unscented_gaussian_sum_filter``'s with one component
    and the backward gain uses the sigma-point cross-covariance of the filter's predict (``bf_uks_smoother_f32``; the
    contract is in csrc/rts_smoother.hpp); it needs the predicted streams and excludes ``extended=True``.  For linear
    dynamics it is the linear smoother's function of the streams; it serves registry dynamics only.  The cross-covariance is a float32 difference of
    sigma-point images: its relative error grows like 2^-24 |f(m)| / (alpha sqrt(n + dq + kappa) |P|^1/2), 1e-4 ... 2e-4
    at alpha = 1e-3.
    ``carry``: the :class:`SmootherCarry` returned (``return_carry=True``) by the smoothing of the steps that FOLLOW
    these (backward chunking); the chunk's last step then gets a cross-covariance too, so the cross-covariances cover
    all T steps of the chunk instead of T-1.  ``out``: a previous :class:`PosteriorGaussianSmoothed` whose smoothed
    buffers are reused: float32 tensors on the posterior's device in exactly the shapes this call returns
    (``smoothed_cross_covariances`` with T-1 steps, T with a carry; giving it asks for the cross-covariances; at T = 1
    without a carry that is the empty (B, 1, 0, n, n) tensor and nothing is stored into it), anything else is refused
    before a kernel is launched.  Returns :class:`PosteriorGaussianSmoothed` (and the carry when ``return_carry``).
    """
    torch = _torch()
    f = params.dynamics_function
    if not isinstance(f, DeviceFunction):  # a plain Python function is recorded at the model's dimensions, as the filters do
        n0, dq0, _ = _param_dims(params)
        f = require_device_function(f, "dynamics", "params.dynamics_function", n0, dq0)
    f = require_device_function(f, "dynamics", "params.dynamics_function")
    means, covs = posterior.means, posterior.covariances
    if means is None or covs is None:
        raise ValueError("the smoother needs the filtered means and covariances")
    squeeze = means.dim() == 3
    m_b, P_b = _batched(means, 1), _batched(covs, 2)
    pm_b, pP_b = _batched(posterior.predicted_means, 1), _batched(posterior.predicted_covariances, 2)
    if (pm_b is None) != (pP_b is None):
        raise ValueError("predicted_means and predicted_covariances are given together or not at all")
    B, K, T, n = (int(v) for v in m_b.shape)
    if K != 1:
        raise ValueError(f"the smoother serves one component (Kalman / extended Kalman); the posterior has K = {K}")
    if T == 0 or B == 0:
        raise ValueError("empty posterior")
    if tuple(P_b.shape) != (B, 1, T, n, n):
        raise ValueError(f"covariances have shape {tuple(covs.shape)}, expected {(B, 1, T, n, n)}")
    if f.out_dim != n:
        raise ValueError(f"the dynamics function has state dimension {f.out_dim}, the posterior {n}")
    up = _ukf_params(uparams, extended) if uparams is not None else None
    use_ext = (f.fn_id != DYN_LINEAR) if extended is None else bool(extended)
    if up is not None and pm_b is None:
        raise ValueError("the unscented smoother needs the predicted means and covariances (filter with FULL5 fields)")
    if use_ext and pm_b is None:
        raise ValueError("the extended smoother needs the predicted means and covariances (filter with FULL5 fields)")
    for t_ in (m_b, P_b, pm_b, pP_b):
        if t_ is not None and (t_.dtype != torch.float32 or not t_.is_cuda):
            raise ValueError("posterior streams must be float32 device tensors")
    lib = _lib.require_gpu()
    dev = m_b.device

    fd = _lib.bf_out_desc()
    fd.means, fd.covs = _stream_desc(m_b, 1), _stream_desc(P_b, 2)
    fd.pred_means, fd.pred_covs = _stream_desc(pm_b, 1), _stream_desc(pP_b, 2)

    def buf(name, ev, steps):
        """out.<name> after the checks a raw-pointer store needs (float32, the streams' device, the exact shape), or None."""
        reuse = getattr(out, name, None) if out is not None else None
        if reuse is None:
            return None
        _check_out_tensor(name, reuse, dev)
        want = (B, 1, steps) + ev
        if squeeze and tuple(reuse.shape) == want[1:]:
            return reuse.unsqueeze(0)
        if tuple(reuse.shape) != want:
            raise ValueError(f"out.{name} has shape {tuple(reuse.shape)}, expected {want[1:] if squeeze else want}")
        return reuse

    ms, Ps = buf("smoothed_means", (n,), T), buf("smoothed_covariances", (n, n), T)
    # the cross-covariances a call returns have T-1 steps, T with a carry: that is the shape a given buffer must have
    c_steps = T if carry is not None else T - 1
    Cs = buf("smoothed_cross_covariances", (n, n), c_steps)
    if ms is None:
        ms = _alloc_stream((B, 1, T), (n,), layout, dev)
    if Ps is None:
        Ps = _alloc_stream((B, 1, T), (n, n), layout, dev)
    if Cs is None and cross_covariances:
        Cs = _alloc_stream((B, 1, T), (n, n), layout, dev)[:, :, :c_steps]
    sd = _lib.bf_smooth_desc()
    # (T = 1 without a carry: the cross-covariances have no step, the kernel is not given the empty stream)
    sd.means, sd.covs, sd.cross_covs = _stream_desc(ms, 1), _stream_desc(Ps, 2), _stream_desc(Cs if c_steps > 0 else None, 2)

    cr = _lib.bf_smooth_carry()
    keep = []
    if carry is not None:
        cm, cP = (_dev_f32(v, dev).contiguous() for v in carry)
        if cm.numel() != B * n or cP.numel() != B * n * n:
            raise ValueError("carry does not match (B, n) / (B, n, n)")
        keep += [cm, cP]
        cr.m_in, cr.P_in = cm.data_ptr(), cP.data_ptr()
    c_out = None
    if return_carry:
        c_out = SmootherCarry(torch.empty((B, n), dtype=torch.float32, device=dev),
                              torch.empty((B, n, n), dtype=torch.float32, device=dev))
        cr.m_out, cr.P_out = c_out.means.data_ptr(), c_out.covariances.data_ptr()

    stream = torch.cuda.current_stream(dev).cuda_stream
    if up is not None:
        mdl = _Model(params)
        ud = _inputs_desc(inputs, B, T, dev, keep)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_uks_smoother_f32(C.byref(mdl.c), C.byref(up), C.byref(ud), C.byref(fd), B, T, C.byref(cr),
                                           C.byref(sd), C.c_void_p(stream)))
    elif use_ext:
        mdl = _Model(params)
        ud = _inputs_desc(inputs, B, T, dev, keep)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_eks_smoother_f32(C.byref(mdl.c), C.byref(ud), C.byref(fd), B, T, C.byref(cr), C.byref(sd),
                                           C.c_void_p(stream)))
    else:
        if getattr(f, "M", None) is None:
            raise ValueError("params.dynamics_function must be linear_dynamics for the linear smoother")
        mdl = _LinearDynamics(params, f)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_rts_smoother_f32(C.byref(mdl.c), C.byref(fd), B, T, C.byref(cr), C.byref(sd),
                                           C.c_void_p(stream)))
    for t_ in keep:  # buffers made for this call stay allocated until the asynchronous launch has read them
        t_.record_stream(torch.cuda.current_stream(dev))

    sq = (lambda x: x[0] if (squeeze and x is not None) else x)
    post = PosteriorGaussianSmoothed(sq(m_b), sq(P_b), sq(ms), sq(Ps), sq(Cs))
    return (post, c_out) if return_carry else post


_FILTER_KW = ("initial_means", "initial_covariances", "layout", "device")


def kalman_smoother(params, emissions, **kw):
    """``kalman_filter`` emitting the filtered fields only, then :func:`rts_smoother` on the recompute path (the
    predictions are formed again inside the backward pass: 80 instead of 160 bytes read per step at n = 4).
    Keywords of :func:`kalman_filter` (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the
    filter, the others to :func:`rts_smoother`."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    post = kalman_filter(params, emissions, fields=("means", "covariances"), **fkw)
    return rts_smoother(params, post, **skw)


def extended_kalman_smoother(params, emissions, inputs=None, **kw):
    """The extended Kalman filter (``gaussian_sum_filter`` with one component, started from ``params.initial_mean``
    unless ``initial_means`` is given), then :func:`rts_smoother` through ``bf_eks_smoother_f32``."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    if "initial_means" not in fkw:
        fkw["initial_means"] = _host_f32(params.initial_mean).reshape(1, -1)
    post = gaussian_sum_filter(params, emissions, 1, inputs=inputs,
                               fields=("means", "covariances", "predicted_means", "predicted_covariances"), **fkw)
    return rts_smoother(params, post, inputs=inputs, extended=True, **skw)


def unscented_kalman_smoother(params, uparams, emissions, inputs=None, **kw):
    """The unscented Kalman filter (``unscented_gaussian_sum_filter`` with one component, started from
    ``params.initial_mean`` unless ``initial_means`` is given), then :func:`rts_smoother` through ``bf_uks_smoother_f32``
    (dynamax's ``unscented_kalman_smoother``)."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    if "initial_means" not in fkw:
        fkw["initial_means"] = _host_f32(params.initial_mean).reshape(1, -1)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, 1, inputs=inputs,
                                         fields=("means", "covariances", "predicted_means", "predicted_covariances"), **fkw)
    return rts_smoother(params, post, inputs=inputs, uparams=uparams, **skw)
