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
from ._backward import _front, _call, _wrapper_kw
from .inference import (_torch, _dev_f32, _alloc_stream, _stream_desc, kalman_filter, gaussian_sum_filter,
                        unscented_gaussian_sum_filter)


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


def _sampler_front(params, posterior, S, key, noise, extended, uparams, device):
    """:func:`_front` for a sampler with ``S`` samples per trajectory: the checks of ``num_samples``, ``key`` / ``noise`` and
    ``device`` that every sampler of one-component streams makes before device work."""
    torch = _torch()

    def checks(B, T, n, squeeze):
        if S <= 0:
            raise ValueError(f"num_samples must be positive; got {S}")
        if (key is None) == (noise is None):
            raise ValueError("exactly one of key and noise must be given")
        if noise is not None:
            if not isinstance(noise, torch.Tensor):
                raise ValueError("noise must be a float32 device tensor")
            want = (S, T, n) if squeeze else (B, S, T, n)
            if tuple(noise.shape) != want:
                raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {want}")

    bw = _front("sampler", params, posterior, extended, uparams, checks, (noise,), "posterior streams and noise")
    want_dev = torch.device(device)
    if want_dev.type != bw.dev.type or (want_dev.index is not None and want_dev.index != bw.dev.index):
        raise ValueError(f"device={device!r}, but the posterior lives on {bw.dev}: the sampler runs where its streams are")
    return bw


def _sampler_args(bw, S, key, noise, carry, return_carry, layout, out):
    """The sample buffer (``out`` after its checks, or fresh in ``layout``), the bf_sample_desc and bf_sample_carry of one
    call, the :class:`SamplerCarry` to return (or None) and the tensors made for the call, to keep until it has run."""
    torch = _torch()
    B, T, n, squeeze, dev = bw.B, bw.T, bw.n, bw.squeeze, bw.dev
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
    return xs, sd, cr, c_out, keep


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
    S = int(num_samples)
    bw = _sampler_front(params, posterior, S, key, noise, extended, uparams, device)
    xs, sd, cr, c_out, keep = _sampler_args(bw, S, key, noise, carry, return_carry, layout, out)
    _call("sampler", ("bf_ffbs_sample_f32", "bf_effbs_sample_f32", "bf_uffbs_sample_f32"), bw, params, inputs, options,
          (S, C.byref(cr), C.byref(sd)), keep, _torch().cuda.current_stream(bw.dev))

    res = xs[0] if bw.squeeze else xs
    return (res, c_out) if return_carry else res


def kalman_posterior_sample(params, emissions, num_samples, key, **kw):
    """``kalman_filter`` emitting the filtered fields only, then :func:`posterior_sample` on the recompute path.
    Keywords of :func:`kalman_filter` (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the
    filter, the others to :func:`posterior_sample`.  ``missing`` / ``observed`` are :func:`kalman_filter`'s: the backward pass
    reads no observations, so it runs on the gapped posterior as it is."""
    gaps = {k: kw.pop(k) for k in ("missing", "observed") if k in kw}
    fkw, skw = _wrapper_kw(params, kw, False)
    return posterior_sample(params, kalman_filter(params, emissions, **fkw, **gaps), num_samples, key=key, **skw)


def extended_kalman_posterior_sample(params, emissions, num_samples, key, inputs=None, **kw):
    """The extended Kalman filter (``gaussian_sum_filter`` with one component, started from ``params.initial_mean``
    unless ``initial_means`` is given), then :func:`posterior_sample` through ``bf_effbs_sample_f32``."""
    fkw, skw = _wrapper_kw(params, kw, True)
    post = gaussian_sum_filter(params, emissions, 1, inputs=inputs, **fkw)
    return posterior_sample(params, post, num_samples, key=key, inputs=inputs, extended=True, **skw)


def unscented_kalman_posterior_sample(params, uparams, emissions, num_samples, key, inputs=None, **kw):
    """The unscented Kalman filter (``unscented_gaussian_sum_filter`` with one component, started from
    ``params.initial_mean`` unless ``initial_means`` is given), then :func:`posterior_sample` through
    ``bf_uffbs_sample_f32``."""
    fkw, skw = _wrapper_kw(params, kw, True)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, 1, inputs=inputs, **fkw)
    return posterior_sample(params, post, num_samples, key=key, inputs=inputs, uparams=uparams, **skw)
