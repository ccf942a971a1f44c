"""Posterior sampling on the HIP engine: joint draws x_{0:T-1} ~ p(x_{0:T-1} | y_{0:T-1}) for the Kalman,
extended-Kalman and unscented Kalman filters (dynamax's ``lgssm_posterior_sample``): the backward half of forward-filter
backward-sampling.

The backward pass consumes the streams a filter already wrote, as the smoother does, and runs in ``bf_ffbs_sample_f32`` /
``bf_effbs_sample_f32`` / ``bf_uffbs_sample_f32`` (include/bayesfilt.h, csrc/ffbs_sampler.hpp, where the recursion and its treatment of singular
conditional covariances are stated).  PyTorch only allocates and passes device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Optional, Any

import numpy as np

from . import _lib
from .inference import (_torch, _dev_f32, _host_f32, _alloc_stream, _stream_desc, _Model, _param_dims, kalman_filter,
                        gaussian_sum_filter, unscented_gaussian_sum_filter)
from .nonlinearities import DYN_LINEAR, DeviceFunction, require_device_function
from .smoother import _LinearDynamics, _batched, _FILTER_KW, _ukf_params, _inputs_desc


class SamplerCarry(NamedTuple):
    """The samples at one step, contiguous (B, S, n): what a backward chunk hands to the chunk before it."""
    states: Any


def _keys_for(key, B):
    """(B, 2) uint32 keys: a (B, 2) array as it is, one key split B ways otherwise."""
    from . import random as bfr
    k = np.asarray(key.detach().cpu().numpy() if hasattr(key, "detach") else key)
    if k.ndim == 2:
        if k.shape != (B, 2):
            raise ValueError(f"keys have shape {k.shape}, expected {(B, 2)}")
        return np.ascontiguousarray(k.astype(np.uint32))
    if k.size != 2:
        raise ValueError(f"key must be a (2,) uint32 key or a ({B}, 2) array of keys; got shape {k.shape}")
    return bfr.split(k.astype(np.uint32), B)


def posterior_sample(params, posterior, num_samples: int = 1, *, key=None, noise=None, inputs=None, carry=None,
                     return_carry: bool = False, layout: str = "reference", out=None, extended: Optional[bool] = None,
                     uparams=None, device="cuda", options=None):
    """Draw ``num_samples`` joint trajectories per filtered trajectory of ``posterior`` (a ``PosteriorGaussianSumFiltered``
    of ``kalman_filter``, or of ``gaussian_sum_filter`` with one component) on the device.  Returns a float32 device
    tensor (S, T, n) for one trajectory, (B, S, T, n) for a batch.

    Exactly one of ``key`` and ``noise``.  ``noise``: a device float32 tensor of standard normals shaped like the result.
    ``key``: ``keys = random.split(key, B)`` (a (B, 2) array of keys is taken as it is) and trajectory b uses
    ``random.normal(keys[b], (S, T, n))``; chunked calls take a key per chunk.
    Linear dynamics run ``bf_ffbs_sample_f32`` (without the predicted streams in ``posterior`` they are recomputed);
    other registry dynamics, ``nonlinearities.user_dynamics`` source and plain Python functions (recorded at the model's
    dimensions) run ``bf_effbs_sample_f32`` and need them, ``extended=True`` sends a linear model there too.
    ``uparams`` (a :class:`ParamsUKF` or a 3-tuple): the posterior is ``unscented_gaussian_sum_filter``'s with one component
    and the gain uses the sigma-point cross-covariance of the filter's predict (``bf_uffbs_sample_f32``, the contract and
    its float32 error model as in :func:`rts_smoother`; registry dynamics only); it needs the predicted streams and excludes
    ``extended=True``.
    ``carry``: the :class:`SamplerCarry` returned (``return_carry=True``) by the sampling of the steps that FOLLOW these.
    ``out``: a tensor a previous call returned, reused.  ``device`` must name the device the posterior's streams live on.
    ``options``: e.g. ``{"ffbs_spl": 4}``, ``{"force_generic": 1}``.
    """
    torch = _torch()
    f = params.dynamics_function
    if not isinstance(f, DeviceFunction):  # a plain Python function is recorded at the model's dimensions, as the filters do
        n0, dq0, _ = _param_dims(params)
        f = require_device_function(f, "dynamics", "params.dynamics_function", n0, dq0)
    f = require_device_function(f, "dynamics", "params.dynamics_function")
    means, covs = posterior.means, posterior.covariances
    if means is None or covs is None:
        raise ValueError("the sampler needs the filtered means and covariances")
    squeeze = means.dim() == 3
    m_b, P_b = _batched(means, 1), _batched(covs, 2)
    pm_b, pP_b = _batched(posterior.predicted_means, 1), _batched(posterior.predicted_covariances, 2)
    if (pm_b is None) != (pP_b is None):
        raise ValueError("predicted_means and predicted_covariances are given together or not at all")
    B, K, T, n = (int(v) for v in m_b.shape)
    S = int(num_samples)
    if K != 1:
        raise ValueError(f"the sampler serves one component (Kalman / extended Kalman); the posterior has K = {K}")
    if T == 0 or B == 0:
        raise ValueError("empty posterior")
    if S <= 0:
        raise ValueError(f"num_samples must be positive; got {num_samples}")
    if tuple(P_b.shape) != (B, 1, T, n, n):
        raise ValueError(f"covariances have shape {tuple(covs.shape)}, expected {(B, 1, T, n, n)}")
    if f.out_dim != n:
        raise ValueError(f"the dynamics function has state dimension {f.out_dim}, the posterior {n}")
    if (key is None) == (noise is None):
        raise ValueError("exactly one of key and noise must be given")
    if noise is not None:
        if not isinstance(noise, torch.Tensor):
            raise ValueError("noise must be a float32 device tensor")
        want = (S, T, n) if squeeze else (B, S, T, n)
        if tuple(noise.shape) != want:
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {want}")
    up = _ukf_params(uparams, extended) if uparams is not None else None
    use_ext = (f.fn_id != DYN_LINEAR) if extended is None else bool(extended)
    if up is not None and pm_b is None:
        raise ValueError("the unscented sampler needs the predicted means and covariances (filter with FULL5 fields)")
    if use_ext and pm_b is None:
        raise ValueError("the extended sampler needs the predicted means and covariances (filter with FULL5 fields)")
    for t_ in (m_b, P_b, pm_b, pP_b, noise):
        if t_ is not None and (t_.dtype != torch.float32 or not t_.is_cuda):
            raise ValueError("posterior streams and noise must be float32 device tensors")
    lib = _lib.require_gpu()
    dev = m_b.device
    want_dev = torch.device(device)
    if want_dev.type != dev.type or (want_dev.index is not None and want_dev.index != dev.index):
        raise ValueError(f"device={device!r}, but the posterior lives on {dev}: the sampler runs where its streams are")
    cur = torch.cuda.current_stream(dev)

    fd = _lib.bf_out_desc()
    fd.means, fd.covs = _stream_desc(m_b, 1), _stream_desc(P_b, 2)
    fd.pred_means, fd.pred_covs = _stream_desc(pm_b, 1), _stream_desc(pP_b, 2)

    keep = []
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise ValueError(f"out must be a torch tensor; got {type(out).__name__}")
        xs = out.unsqueeze(0) if out.dim() == 3 else out
        if tuple(xs.shape) != (B, S, T, n) or xs.dtype != torch.float32 or not xs.is_cuda:
            raise ValueError(f"out has shape {tuple(out.shape)}, expected a float32 device tensor {(B, S, T, n)}")
        if xs.device != dev:
            raise ValueError(f"out is on {xs.device}, but the posterior lives on {dev}: the kernel stores where its streams are")
    else:
        xs = _alloc_stream((B, S, T), (n,), layout, dev)
    sd = _lib.bf_sample_desc()
    sd.samples = _stream_desc(xs, 1)
    if noise is not None:
        z = noise.unsqueeze(0) if squeeze else noise
        st = z.stride()
        sd.noise.ptr, sd.noise.sB, sd.noise.sK, sd.noise.sT, sd.noise.sE = z.data_ptr(), st[0], st[1], st[2], st[3]
    else:
        if S * T * n > 0x7fffffff:
            raise ValueError("drawing from a key serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T")
        kd = torch.as_tensor(_keys_for(key, B).view(np.int32), device=dev)
        keep.append(kd)
        sd.keys = kd.data_ptr()

    cr = _lib.bf_sample_carry()
    if carry is not None:
        cx = _dev_f32(carry.states if isinstance(carry, SamplerCarry) else carry, dev).contiguous()
        if cx.numel() != B * S * n:
            raise ValueError(f"carry does not match (B, S, n) = {(B, S, n)}")
        keep.append(cx)
        cr.x_in = cx.data_ptr()
    c_out = None
    if return_carry:
        c_out = SamplerCarry(torch.empty((B, S, n), dtype=torch.float32, device=dev))
        cr.x_out = c_out.states.data_ptr()

    stream = cur.cuda_stream
    if up is not None:
        mdl = _Model(params)
        ud = _inputs_desc(inputs, B, T, dev, keep)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_uffbs_sample_f32(C.byref(mdl.c), C.byref(up), C.byref(ud), C.byref(fd), B, T, S, C.byref(cr),
                                           C.byref(sd), C.c_void_p(stream)))
    elif use_ext:
        mdl = _Model(params)
        ud = _inputs_desc(inputs, B, T, dev, keep)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_effbs_sample_f32(C.byref(mdl.c), C.byref(ud), C.byref(fd), B, T, S, C.byref(cr), C.byref(sd),
                                           C.c_void_p(stream)))
    else:
        if getattr(f, "M", None) is None:
            raise ValueError("params.dynamics_function must be linear_dynamics for the linear sampler")
        mdl = _LinearDynamics(params, f)
        _lib.arm_call_options(lib, options)
        _lib.check(lib.bf_ffbs_sample_f32(C.byref(mdl.c), C.byref(fd), B, T, S, C.byref(cr), C.byref(sd),
                                          C.c_void_p(stream)))
    for t_ in keep:  # buffers made for this call stay allocated until the asynchronous launch has read them
        t_.record_stream(cur)

    res = xs[0] if squeeze else xs
    return (res, c_out) if return_carry else res


def kalman_posterior_sample(params, emissions, num_samples, key, **kw):
    """``kalman_filter`` emitting the filtered fields only, then :func:`posterior_sample` on the recompute path.
    Keywords of :func:`kalman_filter` (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the
    filter, the others to :func:`posterior_sample`."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    post = kalman_filter(params, emissions, fields=("means", "covariances"), **fkw)
    return posterior_sample(params, post, num_samples, key=key, **skw)


def extended_kalman_posterior_sample(params, emissions, num_samples, key, inputs=None, **kw):
    """The extended Kalman filter (``gaussian_sum_filter`` with one component, started from ``params.initial_mean``
    unless ``initial_means`` is given), then :func:`posterior_sample` through ``bf_effbs_sample_f32``."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    if "initial_means" not in fkw:
        fkw["initial_means"] = _host_f32(params.initial_mean).reshape(1, -1)
    post = gaussian_sum_filter(params, emissions, 1, inputs=inputs,
                               fields=("means", "covariances", "predicted_means", "predicted_covariances"), **fkw)
    return posterior_sample(params, post, num_samples, key=key, inputs=inputs, extended=True, **skw)


def unscented_kalman_posterior_sample(params, uparams, emissions, num_samples, key, inputs=None, **kw):
    """The unscented Kalman filter (``unscented_gaussian_sum_filter`` with one component, started from
    ``params.initial_mean`` unless ``initial_means`` is given), then :func:`posterior_sample` through
    ``bf_uffbs_sample_f32``."""
    fkw = {k: kw[k] for k in _FILTER_KW if k in kw}
    skw = {k: v for k, v in kw.items() if k not in ("initial_means", "initial_covariances")}
    if "initial_means" not in fkw:
        fkw["initial_means"] = _host_f32(params.initial_mean).reshape(1, -1)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, 1, inputs=inputs,
                                         fields=("means", "covariances", "predicted_means", "predicted_covariances"), **fkw)
    return posterior_sample(params, post, num_samples, key=key, inputs=inputs, uparams=uparams, **skw)
