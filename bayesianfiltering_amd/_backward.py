"""What the two backward passes over a filter's streams share on the Python side: the RTS smoother (smoother.py) and the
posterior sampler (sampler.py).  One front half (the posterior's streams, their checks and the choice of route), one call
(the three C functions of a product) and the filter-then-backward-pass wrappers' keyword handling."""
import ctypes as C
from typing import NamedTuple, Optional, Any

import numpy as np

from . import _lib
from .inference import _torch, _host_f32, _fp, _stream_desc, _time_varying, _Model, _param_dims, _inputs_desc, _ukf_params
from .nonlinearities import DYN_LINEAR, DeviceFunction, require_device_function


class _LinearDynamics:
    """bf_lgssm holding the dynamics half of a linear model (the backward passes never read the emission)."""

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


class _Backward(NamedTuple):
    """What :func:`_front` hands a backward pass: the dynamics function, the batched streams (B, K, T, ...), the sizes,
    whether the caller's posterior was unbatched, the streams' device, their descriptor and the route (``up``: the
    unscented route's bf_ukf_params or None; else ``use_ext``: extended or linear).  ``K`` is 1 except for the
    Gaussian-sum passes (``_front(..., multi=True)``)."""
    f: Any
    lib: Any
    m_b: Any
    P_b: Any
    B: int
    T: int
    n: int
    squeeze: bool
    dev: Any
    fd: Any
    up: Optional[Any]
    use_ext: bool
    K: int = 1


def _front(noun, params, posterior, extended, uparams, product_checks=None, also=(), what="posterior streams", multi=False):
    """The front half of a backward pass of ``noun`` ("smoother" / "sampler") up to the device: resolves the dynamics
    function, batches the posterior, checks it and chooses the route.  ``product_checks(B, T, n, squeeze)``: the product's
    own argument checks, made once the sizes are known and before the route is chosen; ``also``: further tensors that
    must be float32 device tensors like the streams (``what`` names them all).  ``multi``: the pass serves K >= 1
    components (the Gaussian-sum smoother); every other pass refuses K > 1."""
    torch = _torch()
    f = params.dynamics_function
    if not isinstance(f, DeviceFunction):  # a plain Python function is recorded at the model's dimensions, as the filters do
        n0, dq0, _ = _param_dims(params)
        f = require_device_function(f, "dynamics", "params.dynamics_function", n0, dq0)
    f = require_device_function(f, "dynamics", "params.dynamics_function")
    means, covs = posterior.means, posterior.covariances
    if means is None or covs is None:
        raise ValueError(f"the {noun} needs the filtered means and covariances")
    squeeze = means.dim() == 3
    m_b, P_b = _batched(means, 1), _batched(covs, 2)
    pm_b, pP_b = _batched(posterior.predicted_means, 1), _batched(posterior.predicted_covariances, 2)
    if (pm_b is None) != (pP_b is None):
        raise ValueError("predicted_means and predicted_covariances are given together or not at all")
    B, K, T, n = (int(v) for v in m_b.shape)
    if K != 1 and not multi:
        raise ValueError(f"the {noun} serves one component (Kalman / extended Kalman); the posterior has K = {K}")
    if T == 0 or B == 0:
        raise ValueError("empty posterior")
    if tuple(P_b.shape) != (B, K, T, n, n):
        raise ValueError(f"covariances have shape {tuple(covs.shape)}, expected {(B, K, T, n, n)}")
    if f.out_dim != n:
        raise ValueError(f"the dynamics function has state dimension {f.out_dim}, the posterior {n}")
    if product_checks is not None:
        product_checks(B, T, n, squeeze)
    up = _ukf_params(uparams, extended) if uparams is not None else None
    use_ext = (f.fn_id != DYN_LINEAR) if extended is None else bool(extended)
    if up is not None and pm_b is None:
        raise ValueError(f"the unscented {noun} needs the predicted means and covariances (filter with FULL5 fields)")
    if use_ext and pm_b is None:
        raise ValueError(f"the extended {noun} needs the predicted means and covariances (filter with FULL5 fields)")
    for t_ in (m_b, P_b, pm_b, pP_b) + tuple(also):
        if t_ is not None and (t_.dtype != torch.float32 or not t_.is_cuda):
            raise ValueError(f"{what} must be float32 device tensors")
    lib = _lib.require_gpu()
    fd = _lib.bf_out_desc()
    fd.means, fd.covs = _stream_desc(m_b, 1), _stream_desc(P_b, 2)
    fd.pred_means, fd.pred_covs = _stream_desc(pm_b, 1), _stream_desc(pP_b, 2)
    return _Backward(f, lib, m_b, P_b, B, T, n, squeeze, m_b.device, fd, up, use_ext, K)


def _call(noun, names, bw, params, inputs, options, tail, keep, cur):
    """The one C call of a backward pass.  ``names``: the product's (linear, extended, unscented) C functions; ``tail``: its
    trailing arguments after ``B, T`` (``[S,] carry, desc``); the stream ``cur`` is appended.  The call options are armed
    after everything that can raise, immediately before the call; then the tensors in ``keep``, made for this call, are
    recorded on ``cur``: they stay allocated until the asynchronous launch has read them."""
    lib = bw.lib
    sizes = (bw.B, bw.T) + tuple(tail) + (C.c_void_p(cur.cuda_stream),)
    if bw.up is not None or bw.use_ext:
        mdl = _Model(params)
        ud = _inputs_desc(inputs, bw.B, bw.T, bw.dev, keep)
        head = (C.byref(mdl.c), C.byref(bw.up), C.byref(ud)) if bw.up is not None else (C.byref(mdl.c), C.byref(ud))
        fn = getattr(lib, names[2] if bw.up is not None else names[1])
    else:
        if getattr(bw.f, "M", None) is None:
            raise ValueError(f"params.dynamics_function must be linear_dynamics for the linear {noun}")
        mdl = _LinearDynamics(params, bw.f)
        head = (C.byref(mdl.c),)
        fn = getattr(lib, names[0])
    _lib.arm_call_options(lib, options)
    _lib.check(fn(*head, C.byref(bw.fd), *sizes))
    for t_ in keep:
        t_.record_stream(cur)


_FILTER_KW = ("initial_means", "initial_covariances", "layout", "device")
_FULL5_PRED = ("means", "covariances", "predicted_means", "predicted_covariances")


def _wrapper_kw(params, kw, nonlinear):
    """Keywords of a filter-then-backward-pass wrapper: those of the filter (``_FILTER_KW``; a nonlinear filter starts from
    ``params.initial_mean`` unless ``initial_means`` is given, and emits the predicted streams too) and those of the
    backward pass (``layout`` and ``device`` go to both)."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    if nonlinear and "initial_means" not in fkw:
        fkw["initial_means"] = _host_f32(params.initial_mean).reshape(1, -1)
    if nonlinear:   # ``missing`` / ``observed`` are the Gaussian-sum filters': a backward pass reads no observations
        fkw.update({k: skw.pop(k) for k in ("missing", "observed") if k in skw})
    fkw["fields"] = _FULL5_PRED if nonlinear else ("means", "covariances")
    return fkw, skw
