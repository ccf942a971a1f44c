"""Joint draws from the smoothed Gaussian mixture of ``gaussian_sum_filter`` / ``unscented_gaussian_sum_filter`` with K >= 1
components, on the HIP engine.

The model is a mixture over the index of the initial component (gaussian_sum_smoother.py), so a joint draw picks its
component k ~ Cat(w_{T-1}) ONCE and then runs backward sampling along chain k: ``bf_gs_sample_f32`` (include/bayesfilt.h
states the draw and the recursion).  PyTorch only allocates and passes device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Any

import numpy as np

from . import _lib
from ._backward import _front, _inputs_desc
from .gaussian_sum_smoother import _gs_wrapper_kw
from .inference import (_torch, _dev_f32, _alloc_stream, _stream_desc, _Model, gaussian_sum_filter,
                        unscented_gaussian_sum_filter)
from .sampler import _keys_for


class GaussianSumSamplerCarry(NamedTuple):
    """The samples at one step, contiguous (B, S, n), and their components (B, S) int32: what a backward chunk hands to the
    chunk before it."""
    states: Any
    components: Any


def gaussian_sum_posterior_sample(params, posterior, num_samples: int = 1, *, key=None, noise=None, component_noise=None,
                                  components=None, inputs=None, weights=None, carry=None, return_carry: bool = False,
                                  return_components: bool = False, layout: str = "reference", uparams=None, device="cuda",
                                  options=None):
    """Draw ``num_samples`` joint trajectories per filtered trajectory of the K-component ``posterior`` (with ``uparams``:
    ``unscented_gaussian_sum_filter``'s).  Returns a float32 device tensor (B, S, T, n) -- (S, T, n) for one trajectory.

    Sample (b, s) draws a component z from ``weights`` (B, K) (default ``posterior.weights[..., -1]``, the filter's
    weights at the last step of the whole series) with the uniform v[b, s]: the smallest j whose cumulative weight exceeds
    v times the total; weights that are not finite or sum to nothing give z = -1 and a NaN sample.  It is then
    ``posterior_sample`` on component z with noise row (b, s), bit for bit.
    Normals: ``noise`` (B, S, T, n), else from ``key``; uniforms: ``components`` (B, S) integers given outright, else the
    ``carry``'s, else ``component_noise`` (B, S), else from ``key``.  ``key``: ``k_x, k_z = random.split(key, 2)``; the
    trajectory keys of each are formed as :func:`posterior_sample` forms them, ``random.split(k, B)`` (a (B, 2) array of
    keys: key b is split in two for trajectory b): trajectory b uses ``random.normal(keys_x[b], (S, T, n))`` and
    ``random.uniform(keys_z[b], (S,))``; chunked calls take a key per chunk.
    ``carry`` / ``return_carry``: backward chunking (:class:`GaussianSumSamplerCarry`; the components travel in it).
    ``return_components``: also return the (B, S) int32 components.  Returns ``samples[, carry][, components]``.
    """
    torch = _torch()
    S = int(num_samples)
    if S <= 0:
        raise ValueError(f"num_samples must be positive; got {num_samples}")
    if components is not None and component_noise is not None:
        raise ValueError("give components or component_noise, not both")
    carried = carry.components if (carry is not None and components is None) else None
    if carried is not None and component_noise is not None:
        raise ValueError("the carry holds the components: component_noise would not be read")
    draw = components is None and carried is None
    need_key = noise is None or (draw and component_noise is None)
    if need_key and key is None:
        raise ValueError("key is required unless noise and (component_noise or components or a carry) are given")
    if key is not None and not need_key:
        raise ValueError("key would not be read: noise and the components' source are both given")

    def checks(B, T, n, squeeze):
        if noise is not None:
            if not isinstance(noise, torch.Tensor):
                raise ValueError("noise must be a float32 device tensor")
            want = (S, T, n) if squeeze else (B, S, T, n)
            if tuple(noise.shape) != want:
                raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {want}")

    bw = _front("Gaussian-sum sampler", params, posterior, True if uparams is None else None, uparams, checks, (noise,),
                "posterior streams and noise", multi=True)
    B, T, n, K, squeeze, dev = bw.B, bw.T, bw.n, bw.K, bw.squeeze, bw.dev
    keep = []

    def per_sample(x, name, dtype):
        """a (B, S) argument -- (S,) for one trajectory -- as a contiguous device tensor"""
        t_ = torch.as_tensor(x.detach() if isinstance(x, torch.Tensor) else np.asarray(x), device=dev).to(dtype)
        if tuple(t_.shape) != ((S,) if squeeze else (B, S)) and tuple(t_.shape) != (B, S):
            raise ValueError(f"{name} has shape {tuple(t_.shape)}, expected {(S,) if squeeze else (B, S)}")
        t_ = t_.reshape(B, S).contiguous()
        keep.append(t_)
        return t_

    sd = _lib.bf_gs_sample_desc()
    xs = _alloc_stream((B, S, T), (n,), layout, dev)
    sd.samples = _stream_desc(xs, 1)
    if key is not None:
        from . import random as bfr
        k = np.asarray(key.detach().cpu().numpy() if hasattr(key, "detach") else key)
        if k.ndim == 2:  # a key per trajectory: split each
            if k.shape != (B, 2):
                raise ValueError(f"keys have shape {k.shape}, expected {(B, 2)}")
            pairs = np.stack([bfr.split(k[b].astype(np.uint32), 2) for b in range(B)])
            keys_x, keys_z = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        else:
            k_x, k_z = bfr.split(np.asarray(k, np.uint32).reshape(2), 2)
            keys_x, keys_z = _keys_for(k_x, B), _keys_for(k_z, B)
    if noise is not None:
        z = noise.unsqueeze(0) if squeeze else noise
        st = z.stride()
        sd.noise.ptr, sd.noise.sB, sd.noise.sK, sd.noise.sT, sd.noise.sE = z.data_ptr(), st[0], st[1], st[2], st[3]
    else:
        if S * T * n > 0x7fffffff:
            raise ValueError("drawing from a key serves S*T*n <= 2^31 - 1 values per trajectory; sample in chunks of T")
        kd = torch.as_tensor(keys_x.view(np.int32), device=dev)
        keep.append(kd)
        sd.keys = kd.data_ptr()
    if not draw:
        sd.comp_in = per_sample(components if components is not None else carried, "components", torch.int32).data_ptr()
    else:
        if weights is None:
            if posterior.weights is None:
                raise ValueError("give weights=, or a posterior that holds the filter's weights")
            weights = posterior.weights[..., -1]
        w = _dev_f32(weights, dev).reshape(-1, K)
        if w.shape[0] != B:
            raise ValueError(f"weights have shape {tuple(w.shape)}, expected {(B, K)}")
        w = w.contiguous()
        keep.append(w)
        sd.weights = w.data_ptr()
        if component_noise is not None:
            sd.comp_noise = per_sample(component_noise, "component_noise", torch.float32).data_ptr()
        else:
            kz = torch.as_tensor(keys_z.view(np.int32), device=dev)
            keep.append(kz)
            sd.comp_keys = kz.data_ptr()
    z_out = None
    if return_components or return_carry:
        z_out = torch.empty((B, S), dtype=torch.int32, device=dev)
        sd.comp_out = z_out.data_ptr()

    cr = _lib.bf_sample_carry()
    if carry is not None:
        cx = _dev_f32(carry.states, dev).contiguous()
        if cx.numel() != B * S * n:
            raise ValueError(f"carry does not match (B, S, n) = {(B, S, n)}")
        keep.append(cx)
        cr.x_in = cx.data_ptr()
    c_out = None
    if return_carry:
        c_out = GaussianSumSamplerCarry(torch.empty((B, S, n), dtype=torch.float32, device=dev), z_out)
        cr.x_out = c_out.states.data_ptr()

    mdl = _Model(params)
    ud = _inputs_desc(inputs, B, T, dev, keep)
    cur = torch.cuda.current_stream(dev)
    _lib.arm_call_options(bw.lib, options)
    _lib.check(bw.lib.bf_gs_sample_f32(C.byref(mdl.c), C.byref(bw.up) if bw.up is not None else None, C.byref(ud),
                                       C.byref(bw.fd), B, T, K, S, C.byref(cr), C.byref(sd), C.c_void_p(cur.cuda_stream)))
    for t_ in keep:
        t_.record_stream(cur)

    res = [xs[0] if squeeze else xs]
    if return_carry:
        res.append(c_out)
    if return_components:
        res.append(z_out[0] if squeeze else z_out)
    return res[0] if len(res) == 1 else tuple(res)


def extended_gaussian_sum_posterior_sample(params, emissions, num_components, num_samples, key, inputs=None, **kw):
    """``gaussian_sum_filter`` with ``num_components`` components, then :func:`gaussian_sum_posterior_sample`.  Keywords of
    the filter (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the filter, the others to the sampler."""
    fkw, skw = _gs_wrapper_kw(params, kw)
    post = gaussian_sum_filter(params, emissions, num_components, inputs=inputs, **fkw)
    return gaussian_sum_posterior_sample(params, post, num_samples, key=key, inputs=inputs, **skw)


def unscented_gaussian_sum_posterior_sample(params, uparams, emissions, num_components, num_samples, key, inputs=None, **kw):
    """``unscented_gaussian_sum_filter`` with ``num_components`` components, then :func:`gaussian_sum_posterior_sample` on the
    unscented route."""
    fkw, skw = _gs_wrapper_kw(params, kw)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, num_components, inputs=inputs, **fkw)
    return gaussian_sum_posterior_sample(params, post, num_samples, key=key, inputs=inputs, uparams=uparams, **skw)
