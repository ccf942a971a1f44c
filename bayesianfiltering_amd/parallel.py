"""Parallel-in-time Kalman filter, RTS smoother and posterior sampler: :func:`kalman_filter`, :func:`rts_smoother` and
:func:`posterior_sample` for few long trajectories.

``kalman_filter`` gets its parallelism from the batch axis and walks time serially: one long series occupies one lane.
:func:`parallel_kalman_filter` cuts time into blocks of ``block`` steps that run on separate lanes (associative filtering
elements combined by a prefix scan; the scheme is stated at the head of ``csrc/kf_pscan.hpp``).  Inside a block the outputs
are the ordinary filter's from that block's start state; the start states come from a jitter-free recursion, so the result
agrees with ``kalman_filter`` to fp32 tolerance (1e-5 relative), not bit for bit.  It is worth calling up to a few thousand
trajectories (DESIGN.md has the measured crossover); ``kalman_filter`` never dispatches to it.

:func:`parallel_rts_smoother` is the backward pass with the same structure (associative smoothing elements combined by a
suffix scan; ``csrc/rts_pscan.hpp``): inside a block the outputs are ``rts_smoother``'s from that block's carry, the last
block -- with ``T <= block`` the whole call -- equals ``rts_smoother`` bit for bit, the rest agrees to fp32 tolerance.
:func:`parallel_kalman_smoother` runs the two in turn.  ``rts_smoother`` and ``kalman_smoother`` never dispatch to them.

:func:`parallel_posterior_sample` is the third consumer of those streams (the backward-sampling step is an affine map of the
sample at t+1, so spans of steps combine by a suffix scan; ``csrc/ffbs_pscan.hpp``): inside a block the samples are
``posterior_sample``'s from that block's start, the last block -- with ``T <= block`` the whole call -- equals it bit for bit
on the same streams and noise, the rest agrees to fp32 tolerance.  :func:`parallel_kalman_posterior_sample` runs the parallel
filter and then it.  ``posterior_sample`` and ``kalman_posterior_sample`` never dispatch to them.
"""
import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._backward import _front, _wrapper_kw, _LinearDynamics
from .inference import FULL5, _Lgssm, _kalman_call, _missing_route, _param_dims, _torch
from .nonlinearities import DeviceFunction
from .sampler import _sampler_front, _sampler_args
from .smoother import _out_buffer, _smoothed_buffers, _smoothed_result


def _bytes(lib, family, *sizes, block=None) -> int:
    """``bf_<family>_pscan_workspace_bytes(*sizes, block)``; a refusal raises with the library's text."""
    need = getattr(lib, f"bf_{family}_pscan_workspace_bytes")(*sizes, int(block or 0))
    if need < 0:
        _lib.check(int(need))
    return int(need)


def parallel_kalman_workspace_bytes(n: int, m: int, B: int, T: int, block=None) -> int:
    """Bytes of device workspace a call with these sizes needs: ``4 B ceil(T / L) (4 n^2 + 3 n)``."""
    return _bytes(_lib.load(), "kalman", n, m, B, T, block=block)


def _workspace(workspace, need, dev):
    """The call's workspace: ``workspace`` after its checks, or ``need`` fresh bytes on ``dev``."""
    torch = _torch()
    if workspace is None:
        return torch.empty(int(need), dtype=torch.uint8, device=dev)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != dev \
            or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous uint8 tensor on {dev}")
    return workspace


def _run(lib, family, sizes, block, workspace, dev, options, option, call, stream=None, keep=()):
    """The tail of a parallel call: the bytes these ``sizes`` need (refusals first), the workspace, ``option`` (the family's
    block option) armed for this call only, ``call(pointer, bytes)``, and ``keep`` recorded on ``stream``."""
    need = _bytes(lib, family, *sizes, block=block)
    workspace = _workspace(workspace, need, dev)
    _lib.arm_call_options(lib, {**(options or {}), option: int(block or 0)})   # tuning options for THIS call only (bf_set_call_option)
    _lib.check(call(C.c_void_p(workspace.data_ptr()), workspace.numel()))
    for t_ in keep:
        t_.record_stream(stream)


def _shared_workspace(params, emissions, kw, skw, other_bytes):
    """The filter-then-backward wrappers' workspace, into ``skw``: ``workspace=``, or one allocation of the larger of the
    filter's size and ``other_bytes(n, B, T, block)``.  Returns the filter's ``block`` and ``workspace`` keywords."""
    torch = _torch()
    block = kw.get("block")
    if kw.get("workspace") is None:
        shape = tuple(emissions.shape) if hasattr(emissions, "shape") else np.shape(emissions)
        T, m = int(shape[-2]), int(shape[-1])
        B = int(shape[0]) if len(shape) == 3 else 1
        n = _param_dims(params)[0]
        need = max(parallel_kalman_workspace_bytes(n, m, B, T, block), other_bytes(n, B, T, block))
        skw["workspace"] = torch.empty(need, dtype=torch.uint8, device=kw.get("device", "cuda"))
    return dict(block=block, workspace=skw["workspace"])


def parallel_kalman_filter(params, emissions, *, initial_means=None, initial_covariances=None, carry=None,
                           fields: Sequence[str] = FULL5, layout: str = "reference", out=None,
                           return_loglik: bool = False, return_carry: bool = False, device="cuda", options=None,
                           block=None, workspace=None, missing=None, observed=None):
    """``kalman_filter`` with time parallelism: same model, keywords, container, carry and log-likelihood.

    block: steps per block, 4 ... 4096; ``None`` = a default from (B, T): the largest of ceil(B T / 65 536) (one
    (trajectory, block) lane per lane of the device), sqrt(T / 50) (the measured balance between the scan and the lanes'
    work) and 16.  A trajectory's bits depend on (T, block) alone.
    workspace: a reusable ``torch.uint8`` device tensor of at least :func:`parallel_kalman_workspace_bytes` bytes; allocated
    when absent.  Its contents mean nothing before or after the call.
    Linear registry functions, constant Q and R, state dimension <= 6, emission dimension <= 4.

    ``missing="nan"`` / ``observed=``: the two keywords of :func:`kalman_filter`, with its contract (a NaN entry is a component
    that was not observed at that step; a step with none is predict-only with log-likelihood 0; trailing gaps are a forecast;
    +-Inf still poisons, and without the keyword so does NaN), through ``bf_kalman_filter_pscan_missing_f32``: the fold takes
    each step's element from a table with one entry per observation pattern, block 0 and the emit launch run the masked step.
    A mask is written as NaN into a device copy of the emissions; the caller's tensor is never written.
    """
    gaps, lib, emissions = _missing_route(missing, observed, emissions, device, lambda: _Lgssm(params).m)
    entry = lib.bf_kalman_filter_pscan_missing_f32 if gaps else lib.bf_kalman_filter_pscan_f32
    k = _kalman_call(params, emissions, initial_means, initial_covariances, carry, fields, layout, out, return_loglik,
                     return_carry, device)
    _run(lib, "kalman", (k.mdl.n, k.mdl.m, k.B, k.T), block, workspace, k.y.device, options, "pkf_block",
         lambda ws, size: entry(C.byref(k.mdl.c), C.byref(k.yd), k.B, k.T, C.byref(k.cr), C.byref(k.od), ws, size,
                                C.c_void_p(k.stream)))
    return k.result()


def parallel_rts_workspace_bytes(n: int, B: int, T: int, block=None) -> int:
    """Bytes of device workspace :func:`parallel_rts_smoother` needs at these sizes: ``4 B ceil(T / L) (3 n^2 + 2 n)``."""
    return _bytes(_lib.load(), "rts", n, B, T, block=block)


def parallel_rts_smoother(params, posterior, *, carry=None, cross_covariances: bool = False, layout: str = "reference",
                          out=None, return_carry: bool = False, device="cuda", options=None, block=None, workspace=None):
    """``rts_smoother`` with time parallelism for linear dynamics: same posterior (with the predicted streams, or without:
    they are recomputed), container (:class:`PosteriorGaussianSmoothed`), :class:`SmootherCarry`, ``out=`` rules and
    cross-covariance step counts (T-1, or T with a carry).

    block: steps per block, 4 ... 4096; ``None`` = the default of :func:`parallel_kalman_filter` for (B, T).  A trajectory's
    bits depend on (T, block) and on whether the predictions were given, on nothing else.
    workspace: a reusable ``torch.uint8`` device tensor of at least :func:`parallel_rts_workspace_bytes` bytes; allocated
    when absent.  Its contents mean nothing before or after the call.
    Linear registry dynamics, constant Q, state dimension <= 6.
    """
    torch = _torch()

    def out_shapes(B, T, n, squeeze):
        """``out``'s shapes, refused before the device is asked for (the full checks follow in ``_smoothed_buffers``)."""
        c_steps = T if carry is not None else T - 1
        for name, want in (("smoothed_means", (B, 1, T, n)), ("smoothed_covariances", (B, 1, T, n, n)),
                           ("smoothed_cross_covariances", (B, 1, c_steps, n, n))):
            _out_buffer(out, name, want, squeeze, None)

    bw = _front("smoother", params, posterior, False, None, product_checks=out_shapes)
    if getattr(bw.f, "M", None) is None:
        raise ValueError("params.dynamics_function must be linear_dynamics for the parallel smoother")
    ms, Ps, Cs, sd, cr, keep, c_out = _smoothed_buffers(bw, out, carry, cross_covariances, layout, return_carry)
    mdl = _LinearDynamics(params, bw.f)
    cur = torch.cuda.current_stream(bw.dev)
    _run(bw.lib, "rts", (bw.n, bw.B, bw.T), block, workspace, bw.dev, options, "prs_block",
         lambda ws, size: bw.lib.bf_rts_smoother_pscan_f32(C.byref(mdl.c), C.byref(bw.fd), bw.B, bw.T, C.byref(cr), C.byref(sd),
                                                           ws, size, C.c_void_p(cur.cuda_stream)), cur, keep)
    return _smoothed_result(bw, ms, Ps, Cs, c_out, return_carry)


def parallel_kalman_smoother(params, emissions, **kw):
    """:func:`parallel_kalman_filter` emitting the filtered fields only, then :func:`parallel_rts_smoother` on the recompute
    path.  Keywords of the filter (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the filter, the
    others to the smoother; ``block`` goes to both passes.  One workspace of the larger -- the filter's -- size is allocated
    once and handed to both (or ``workspace=`` is).  ``missing`` / ``observed`` are the filter's: the backward pass reads no
    observations, so it runs on the gapped posterior as it is."""
    gaps = {k: kw.pop(k) for k in ("missing", "observed") if k in kw}
    fkw, skw = _wrapper_kw(params, kw, False)
    fkw.update(_shared_workspace(params, emissions, kw, skw, parallel_rts_workspace_bytes))
    return parallel_rts_smoother(params, parallel_kalman_filter(params, emissions, **fkw, **gaps), **skw)


def parallel_ffbs_workspace_bytes(n: int, B: int, T: int, S: int, block=None) -> int:
    """Bytes of device workspace :func:`parallel_posterior_sample` needs at these sizes: ``4 B ceil(T / L) (n^2 + 2 S n)``."""
    return _bytes(_lib.load(), "ffbs", n, B, T, S, block=block)


def parallel_posterior_sample(params, posterior, num_samples: int = 1, *, key=None, noise=None, carry=None,
                              return_carry: bool = False, layout: str = "reference", out=None, device="cuda", options=None,
                              block=None, workspace=None, **unsupported):
    """``posterior_sample`` with time parallelism for linear dynamics: same posterior (with the predicted streams, or without:
    they are recomputed), ``key`` / ``noise`` rules, result shapes, :class:`SamplerCarry` and ``out=`` rules.

    block: steps per block, 4 ... 4096; ``None`` = a default from (B, S, T): the largest of ceil(B ceil(S / 4) T / 65 536) (one
    (trajectory, block, four samples) lane per lane of the device), sqrt(T / 250) (the measured balance between the scan and
    the lanes' work) and 16.  A sample's bits
    depend on (T, block), on whether the predictions were given, on its trajectory's streams and on its own noise row (with
    ``key``: on (S, T) too, through the key's definition), on nothing else.
    workspace: a reusable ``torch.uint8`` device tensor of at least :func:`parallel_ffbs_workspace_bytes` bytes; allocated
    when absent.  Its contents mean nothing before or after the call.
    ``options``: e.g. ``{"ffbs_spl": 2}`` (samples per lane: 1, 2 or 4).
    Linear registry dynamics, constant Q, state dimension <= 6; ``extended``, ``uparams`` and ``inputs`` are refused.
    """
    torch = _torch()
    for name in unsupported:
        if name not in ("extended", "uparams", "inputs"):
            raise TypeError(f"parallel_posterior_sample() got an unexpected keyword argument {name!r}")
        raise ValueError(f"the parallel sampler serves linear dynamics without inputs: it does not take {name}=")
    linear = "params.dynamics_function must be linear_dynamics for the parallel sampler"
    if isinstance(params.dynamics_function, DeviceFunction) and getattr(params.dynamics_function, "M", None) is None:
        raise ValueError(linear)
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8):
        raise ValueError("workspace must be a contiguous uint8 tensor on the posterior's device")
    S = int(num_samples)
    bw = _sampler_front(params, posterior, S, key, noise, False, None, device)
    if getattr(bw.f, "M", None) is None:   # a plain Python function, recorded by the front half
        raise ValueError(linear)
    xs, sd, cr, c_out, keep = _sampler_args(bw, S, key, noise, carry, return_carry, layout, out)
    mdl = _LinearDynamics(params, bw.f)
    cur = torch.cuda.current_stream(bw.dev)
    _run(bw.lib, "ffbs", (bw.n, bw.B, bw.T, S), block, workspace, bw.dev, options, "pfs_block",
         lambda ws, size: bw.lib.bf_ffbs_sample_pscan_f32(C.byref(mdl.c), C.byref(bw.fd), bw.B, bw.T, S, C.byref(cr), C.byref(sd),
                                                          ws, size, C.c_void_p(cur.cuda_stream)), cur, keep)
    res = xs[0] if bw.squeeze else xs
    return (res, c_out) if return_carry else res


def parallel_kalman_posterior_sample(params, emissions, num_samples, key, **kw):
    """:func:`parallel_kalman_filter` emitting the filtered fields only, then :func:`parallel_posterior_sample` on the
    recompute path.  Keywords of the filter (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the
    filter, the others to the sampler (``noise=`` among them: then ``key`` is None); ``block`` goes to both passes.  One
    workspace of the larger size is allocated once and handed to both (or ``workspace=`` is).  ``missing`` / ``observed`` are the
    filter's: the backward pass reads no observations."""
    gaps = {k: kw.pop(k) for k in ("missing", "observed") if k in kw}
    fkw, skw = _wrapper_kw(params, kw, False)
    fkw.update(_shared_workspace(params, emissions, kw, skw,
                                 lambda n, B, T, block: parallel_ffbs_workspace_bytes(n, B, T, int(num_samples), block)))
    return parallel_posterior_sample(params, parallel_kalman_filter(params, emissions, **fkw, **gaps), num_samples, key=key,
                                     **skw)
