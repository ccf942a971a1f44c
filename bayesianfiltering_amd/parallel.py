"""Parallel-in-time Kalman filter: :func:`kalman_filter` for few long trajectories.

``kalman_filter`` gets its parallelism from the batch axis and walks time serially: one long series occupies one lane.
:func:`parallel_kalman_filter` cuts time into blocks of ``block`` steps that run on separate lanes (associative filtering
elements combined by a prefix scan; the scheme is stated at the head of ``csrc/kf_pscan.hpp``).  Inside a block the outputs
are the ordinary filter's from that block's start state; the start states come from a jitter-free recursion, so the result
agrees with ``kalman_filter`` to fp32 tolerance (1e-5 relative), not bit for bit.  It is worth calling up to a few thousand
trajectories (DESIGN.md has the measured crossover); ``kalman_filter`` never dispatches to it.
"""
import ctypes as C
from typing import Sequence

from . import _lib
from .inference import FULL5, _kalman_call, _torch


def parallel_kalman_workspace_bytes(n: int, m: int, B: int, T: int, block=None) -> int:
    """Bytes of device workspace a call with these sizes needs: ``4 B ceil(T / L) (4 n^2 + 3 n)``."""
    lib = _lib.load()
    need = lib.bf_kalman_pscan_workspace_bytes(n, m, B, T, int(block or 0))
    if need < 0:
        _lib.check(int(need))
    return int(need)


def parallel_kalman_filter(params, emissions, *, initial_means=None, initial_covariances=None, carry=None,
                           fields: Sequence[str] = FULL5, layout: str = "reference", out=None,
                           return_loglik: bool = False, return_carry: bool = False, device="cuda", options=None,
                           block=None, workspace=None):
    """``kalman_filter`` with time parallelism: same model, keywords, container, carry and log-likelihood.

    block: steps per block, 4 ... 4096; ``None`` = a default from (B, T): the largest of ceil(B T / 65 536) (one
    (trajectory, block) lane per lane of the device), sqrt(T / 50) (the measured balance between the scan and the lanes'
    work) and 16.  A trajectory's bits depend on (T, block) alone.
    workspace: a reusable ``torch.uint8`` device tensor of at least :func:`parallel_kalman_workspace_bytes` bytes; allocated
    when absent.  Its contents mean nothing before or after the call.
    Linear registry functions, constant Q and R, state dimension <= 6, emission dimension <= 4.
    """
    torch = _torch()
    lib = _lib.require_gpu()
    k = _kalman_call(params, emissions, initial_means, initial_covariances, carry, fields, layout, out, return_loglik,
                     return_carry, device)
    L = int(block or 0)
    need = lib.bf_kalman_pscan_workspace_bytes(k.mdl.n, k.mdl.m, k.B, k.T, L)
    if need < 0:
        _lib.check(int(need))
    if workspace is None:
        workspace = torch.empty(int(need), dtype=torch.uint8, device=k.y.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != k.y.device \
            or not workspace.is_contiguous():
        raise ValueError(f"workspace must be a contiguous uint8 tensor on {k.y.device}")
    opts = dict(options or {})
    opts["pkf_block"] = L
    _lib.arm_call_options(lib, opts)         # tuning options for THIS call only (bf_set_call_option)
    _lib.check(lib.bf_kalman_filter_pscan_f32(C.byref(k.mdl.c), C.byref(k.yd), k.B, k.T, C.byref(k.cr), C.byref(k.od),
                                              C.c_void_p(workspace.data_ptr()), workspace.numel(), C.c_void_p(k.stream)))
    return k.result()
