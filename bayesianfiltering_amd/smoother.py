"""Rauch-Tung-Striebel smoothing on the HIP engine: the reference's ``SSM.smoother(params, emissions, inputs)``
(gaussfiltax/ssm.py:55-61, 282-300), p(z_t | y_{1:T}), for the Kalman, extended-Kalman and unscented Kalman filters.

The backward pass consumes the streams a filter already wrote (``kalman_filter`` / ``gaussian_sum_filter`` /
``unscented_gaussian_sum_filter`` with one component) and runs in ``bf_rts_smoother_f32`` / ``bf_eks_smoother_f32`` /
``bf_uks_smoother_f32`` (include/bayesfilt.h, csrc/rts_smoother.hpp, where the recursion is stated).  PyTorch only allocates and passes device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Optional, Any

from . import _lib
from ._backward import _front, _call, _wrapper_kw
from .inference import (_torch, _dev_f32, _alloc_stream, _stream_desc, _check_out_tensor, kalman_filter, gaussian_sum_filter,
                        unscented_gaussian_sum_filter)


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


def _out_buffer(out, name, want, squeeze, dev):
    """out.<name> after the checks a raw-pointer store needs (float32, the streams' device, the exact shape ``want`` =
    (B, 1, steps, ...)), or None.  ``dev`` = None: the shape alone (what can be refused before the device is known)."""
    reuse = getattr(out, name, None) if out is not None else None
    if reuse is None:
        return None
    if dev is not None:
        _check_out_tensor(name, reuse, dev)
    if squeeze and tuple(reuse.shape) == want[1:]:
        return reuse.unsqueeze(0)
    if tuple(reuse.shape) != want:
        raise ValueError(f"out.{name} has shape {tuple(reuse.shape)}, expected {want[1:] if squeeze else want}")
    return reuse


def _smoothed_buffers(bw, out, carry, cross_covariances, layout, return_carry):
    """The output half every smoother of one-component streams shares (:func:`rts_smoother`, ``parallel_rts_smoother``): the
    smoothed streams -- ``out``'s where given, else allocated in ``layout`` --, their bf_smooth_desc, the bf_smooth_carry
    with the tensors made for it (``keep``) and the carry to return."""
    torch = _torch()
    B, T, n, squeeze, dev = bw.B, bw.T, bw.n, bw.squeeze, bw.dev
    ms = _out_buffer(out, "smoothed_means", (B, 1, T, n), squeeze, dev)
    Ps = _out_buffer(out, "smoothed_covariances", (B, 1, T, n, n), squeeze, dev)
    # the cross-covariances a call returns have T-1 steps, T with a carry: that is the shape a given buffer must have
    c_steps = T if carry is not None else T - 1
    Cs = _out_buffer(out, "smoothed_cross_covariances", (B, 1, c_steps, n, n), squeeze, dev)
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
    return ms, Ps, Cs, sd, cr, keep, c_out


def _smoothed_result(bw, ms, Ps, Cs, c_out, return_carry):
    sq = (lambda x: x[0] if (bw.squeeze and x is not None) else x)
    post = PosteriorGaussianSmoothed(sq(bw.m_b), sq(bw.P_b), sq(ms), sq(Ps), sq(Cs))
    return (post, c_out) if return_carry else post


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
    bw = _front("smoother", params, posterior, extended, uparams)
    ms, Ps, Cs, sd, cr, keep, c_out = _smoothed_buffers(bw, out, carry, cross_covariances, layout, return_carry)

    _call("smoother", ("bf_rts_smoother_f32", "bf_eks_smoother_f32", "bf_uks_smoother_f32"), bw, params, inputs, options,
          (C.byref(cr), C.byref(sd)), keep, _torch().cuda.current_stream(bw.dev))
    return _smoothed_result(bw, ms, Ps, Cs, c_out, return_carry)


def kalman_smoother(params, emissions, **kw):
    """``kalman_filter`` emitting the filtered fields only, then :func:`rts_smoother` on the recompute path (the
    predictions are formed again inside the backward pass: 80 instead of 160 bytes read per step at n = 4).
    Keywords of :func:`kalman_filter` (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the
    filter, the others to :func:`rts_smoother`.  ``missing`` / ``observed`` are :func:`kalman_filter`'s: the backward pass reads
    no observations, so it runs on the gapped posterior as it is."""
    gaps = {k: kw.pop(k) for k in ("missing", "observed") if k in kw}
    fkw, skw = _wrapper_kw(params, kw, False)
    return rts_smoother(params, kalman_filter(params, emissions, **fkw, **gaps), **skw)


def extended_kalman_smoother(params, emissions, inputs=None, **kw):
    """The extended Kalman filter (``gaussian_sum_filter`` with one component, started from ``params.initial_mean``
    unless ``initial_means`` is given), then :func:`rts_smoother` through ``bf_eks_smoother_f32``."""
    fkw, skw = _wrapper_kw(params, kw, True)
    post = gaussian_sum_filter(params, emissions, 1, inputs=inputs, **fkw)
    return rts_smoother(params, post, inputs=inputs, extended=True, **skw)


def unscented_kalman_smoother(params, uparams, emissions, inputs=None, **kw):
    """The unscented Kalman filter (``unscented_gaussian_sum_filter`` with one component, started from
    ``params.initial_mean`` unless ``initial_means`` is given), then :func:`rts_smoother` through ``bf_uks_smoother_f32``
    (dynamax's ``unscented_kalman_smoother``)."""
    fkw, skw = _wrapper_kw(params, kw, True)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, 1, inputs=inputs, **fkw)
    return rts_smoother(params, post, inputs=inputs, uparams=uparams, **skw)
