"""Particle smoothing on the HIP engine: joint draws x_{0:T-1} ~ p(x_{0:T-1} | y_{0:T-1}) from the history
``bootstrap_particle_filter`` returns -- the counterpart of :mod:`.sampler` for the models the Gaussian filters cannot handle.

Two methods (include/bayesfilt.h and csrc/pf_sampler.hpp state the contract):

* ``method="backward"``: backward simulation (``bf_pf_backward_sample_f32``).  Every step redraws a particle with the
  filter's weight times the transition density towards the state already drawn; needs registry dynamics with a positive
  definite ``F_q Q F_q^T`` and at most 4096 particles.
* ``method="genealogy"``: the filter's own ancestry traced back (``bf_pf_trace_sample_f32``).  Serves every model (singular
  noise, dynamics from source, any particle count) at the price of path degeneracy.

PyTorch only allocates and passes device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Any

import numpy as np

from . import _lib
from .inference import _torch, _dev_f32, _inputs_desc, _Model, bootstrap_particle_filter
from .nonlinearities import DeviceFunction
from .sampler import _keys_for

METHODS = ("backward", "genealogy")


class ParticleSamplerCarry(NamedTuple):
    """What a backward chunk hands to the chunk before it: the samples at its first step (B, S, n), the input u[0] of that
    step (B,) -- the u_{t+1} of the earlier chunk's last step -- and, for the genealogy, the slot a[j, t0] (B, S) int32."""
    states: Any
    input: Any
    slots: Any


def particle_posterior_sample(params, filtered, num_samples: int = 1, *, method: str = "backward", key=None, noise=None,
                              inputs=None, carry=None, return_carry: bool = False, return_indices: bool = False, out=None,
                              device="cuda", options=None):
    """Draw ``num_samples`` joint trajectories per filtered trajectory of ``filtered``, the dict
    ``bootstrap_particle_filter`` returned (``"weights"`` (N, T) and ``"particles"`` (N, T, n), with a leading batch axis for
    a batch; ``"ancestors"`` too for ``method="genealogy"``: filter with ``return_ancestors=True``).  Returns a float32 device
    tensor (S, T, n), or (B, S, T, n) for a batch; with ``return_indices`` also the drawn particle indices (…, S, T) int32.

    Exactly one of ``key`` and ``noise``.  ``noise``: a device float32 tensor of uniforms in [0, 1) shaped (S, T) /
    (B, S, T).  ``key``: ``keys = random.split(key, B)`` (a (B, 2) array of keys is taken as it is) and trajectory b uses
    ``random.uniform(keys[b], (S, T))``; chunked calls take a key per chunk.  The genealogy uses the uniforms of the last
    step only.  ``inputs``: the filter's inputs (backward simulation evaluates the dynamics).  ``carry``: the
    :class:`ParticleSamplerCarry` returned (``return_carry=True``) by the sampling of the steps that FOLLOW these.
    A history stored time-major (e.g. ``particles.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)``) is read with
    its own strides and gives the same bits.
    """
    torch = _torch()
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}; got {method!r}")
    if not isinstance(filtered, dict) or "weights" not in filtered or "particles" not in filtered:
        raise ValueError("filtered must be the dict bootstrap_particle_filter returns, with 'weights' and 'particles'")
    if method == "genealogy" and filtered.get("ancestors") is None:
        raise ValueError("method='genealogy' needs filtered['ancestors']: filter with return_ancestors=True")
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"num_samples must be positive; got {num_samples}")
    if (key is None) == (noise is None):
        raise ValueError("exactly one of key and noise must be given")
    w, x = filtered["weights"], filtered["particles"]
    anc = filtered.get("ancestors") if method == "genealogy" else None
    for t_ in (w, x, anc):
        if t_ is not None and (not isinstance(t_, torch.Tensor) or not t_.is_cuda):
            raise ValueError("the history must be device tensors (what bootstrap_particle_filter returns)")
    if w.dtype != torch.float32 or x.dtype != torch.float32 or (anc is not None and anc.dtype != torch.int32):
        raise ValueError("weights and particles must be float32, ancestors int32")
    squeeze = w.dim() == 2
    if squeeze:
        w, x = w.unsqueeze(0), x.unsqueeze(0)
        anc = anc.unsqueeze(0) if anc is not None else None
    if w.dim() != 3 or x.dim() != 4 or tuple(x.shape[:3]) != tuple(w.shape):
        raise ValueError(f"weights {tuple(filtered['weights'].shape)} and particles {tuple(filtered['particles'].shape)} do not "
                         "match (N, T) / (N, T, n)")
    B, NP, T, n = (int(v) for v in x.shape)
    if B < 1 or NP < 1 or T < 1:
        raise ValueError("empty history")
    if x.stride(3) != 1:
        raise ValueError("the particles' state axis must be contiguous")
    if anc is not None and (tuple(anc.shape) != tuple(w.shape) or tuple(anc.stride()) != tuple(w.stride())):
        raise ValueError("ancestors must have the weights' shape and strides")
    if noise is not None:
        want = (S, T) if squeeze else (B, S, T)
        if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or not noise.is_cuda:
            raise ValueError("noise must be a float32 device tensor")
        if tuple(noise.shape) != want:
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {want}")
    if S * T > 0x7fffffff:
        raise ValueError("S*T must not exceed 2^31 - 1; sample in chunks of T")
    dev = w.device
    want_dev = torch.device(device)
    if want_dev.type != dev.type or (want_dev.index is not None and want_dev.index != dev.index):
        raise ValueError(f"device={device!r}, but the history lives on {dev}: the sampler runs where its history is")
    mdl = None
    if method == "backward":
        if NP > 4096:
            raise ValueError(f"backward simulation serves at most 4096 particles (got {NP}); use method='genealogy'")
        f = params.dynamics_function
        if getattr(f, "source", None) is not None or not isinstance(f, DeviceFunction):
            raise _lib.BayesFiltError(_lib.BF_EUNSUPPORTED, "backward simulation serves registry dynamics; for dynamics given as "
                                      "source or as a Python function use method='genealogy'")
        mdl = _Model(params)
        if mdl.n != n:
            raise ValueError(f"the dynamics function has state dimension {mdl.n}, the particles {n}")
    lib = _lib.require_gpu()
    cur = torch.cuda.current_stream(dev)

    hd = _lib.bf_pf_history()
    hd.weights, (hd.w_sB, hd.w_sN, hd.w_sT) = w.data_ptr(), w.stride()
    hd.particles, (hd.x_sB, hd.x_sN, hd.x_sT) = x.data_ptr(), x.stride()[:3]
    if anc is not None:
        hd.ancestors = anc.data_ptr()

    keep = []
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise ValueError(f"out must be a torch tensor; got {type(out).__name__}")
        xs = out.unsqueeze(0) if out.dim() == 3 else out
        if tuple(xs.shape) != (B, S, T, n) or xs.dtype != torch.float32 or not xs.is_cuda:
            raise ValueError(f"out has shape {tuple(out.shape)}, expected a float32 device tensor {(B, S, T, n)}")
        if xs.device != dev:
            raise ValueError(f"out is on {xs.device}, but the history lives on {dev}: the kernel stores where its history is")
    else:
        xs = torch.empty((B, S, T, n), dtype=torch.float32, device=dev)
    sd = _lib.bf_pf_sample_desc()
    st = xs.stride()
    sd.samples.ptr, sd.samples.sB, sd.samples.sK, sd.samples.sT, sd.samples.sE = xs.data_ptr(), st[0], st[1], st[2], st[3]
    idx = None
    if return_indices:
        idx = torch.empty((B, S, T), dtype=torch.int32, device=dev)
        sd.indices = idx.data_ptr()
    if noise is not None:
        z = noise.unsqueeze(0) if squeeze else noise
        sd.noise, (sd.z_sB, sd.z_sS, sd.z_sT) = z.data_ptr(), z.stride()
    else:
        kd = torch.as_tensor(_keys_for(key, B).view(np.int32), device=dev)
        keep.append(kd)
        sd.keys = kd.data_ptr()

    ud = _inputs_desc(inputs, B, T, dev, keep)
    u = keep[-1] if inputs is not None else None      # (1 or B, T, d)

    cr = _lib.bf_pf_sample_carry()
    if carry is not None:
        if not isinstance(carry, ParticleSamplerCarry):
            raise ValueError("carry must be the ParticleSamplerCarry a later chunk returned")
        if method == "backward":
            cx = _dev_f32(carry.states, dev).contiguous()
            if cx.numel() != B * S * n:
                raise ValueError(f"carry.states does not match (B, S, n) = {(B, S, n)}")
            cu = _dev_f32(carry.input, dev).reshape(-1).contiguous()
            if cu.numel() != B:
                raise ValueError(f"carry.input does not match (B,) = {(B,)}")
            keep += [cx, cu]
            cr.x_in, cr.u_in = cx.data_ptr(), cu.data_ptr()
        else:
            if carry.slots is None:
                raise ValueError("the genealogy needs carry.slots (the carry of a method='genealogy' chunk)")
            ca = carry.slots.to(device=dev, dtype=torch.int32).contiguous()
            if ca.numel() != B * S:
                raise ValueError(f"carry.slots does not match (B, S) = {(B, S)}")
            keep.append(ca)
            cr.a_in = ca.data_ptr()
    c_out = None
    if return_carry:
        u0 = torch.zeros((B,), dtype=torch.float32, device=dev) if u is None else u[:, 0, 0].expand(B).contiguous()
        c_out = ParticleSamplerCarry(torch.empty((B, S, n), dtype=torch.float32, device=dev), u0,
                                     torch.empty((B, S), dtype=torch.int32, device=dev) if method == "genealogy" else None)
        cr.x_out = c_out.states.data_ptr()
        if c_out.slots is not None:
            cr.a_out = c_out.slots.data_ptr()

    stream = C.c_void_p(cur.cuda_stream)
    _lib.arm_call_options(lib, options)
    if method == "backward":
        bm = _lib.bf_bpf_model()
        bm.ssm = mdl.c
        _lib.check(lib.bf_pf_backward_sample_f32(C.byref(bm), C.byref(ud), C.byref(hd), B, T, NP, S, C.byref(cr), C.byref(sd), stream))
    else:
        _lib.check(lib.bf_pf_trace_sample_f32(C.byref(hd), B, T, NP, n, S, C.byref(cr), C.byref(sd), stream))
    for t_ in keep:  # buffers made for this call stay allocated until the asynchronous launch has read them
        t_.record_stream(cur)

    res = xs[0] if squeeze else xs
    if return_indices:
        res = (res, idx[0] if squeeze else idx)
    if return_carry:
        return (res + (c_out,)) if isinstance(res, tuple) else (res, c_out)
    return res


def bootstrap_particle_posterior_sample(params, emissions, num_particles, num_samples, key, inputs=None, **kw):
    """``bootstrap_particle_filter`` then :func:`particle_posterior_sample`, with ``kf, ks = random.split(key, 2)`` as the
    filter's and the sampler's keys.  ``ess_threshold``, ``resampler`` and the missing-observation keywords ``missing`` /
    ``observed`` go to the filter, the other keywords to the sampler (which reads no observations)."""
    from . import random as bfr
    kf, ks = bfr.split(np.asarray(key, dtype=np.uint32).reshape(2), 2)
    fkw = {k: kw.pop(k) for k in ("ess_threshold", "resampler", "missing", "observed") if k in kw}
    dev = kw.get("device", "cuda")
    filtered = bootstrap_particle_filter(params, emissions, num_particles, kf, inputs, return_ancestors=True, device=dev, **fkw)
    return particle_posterior_sample(params, filtered, num_samples, key=ks, inputs=inputs, **kw)
