"""Gaussian-sum smoothing on the HIP engine: the backward pass of ``gaussian_sum_filter`` /
``unscented_gaussian_sum_filter`` with K >= 1 components.

In those filters the components never interact: each is an extended (unscented) Kalman chain started from its own initial
mean, coupled only through the weight recursion (gaussfiltax/inference.py:345-353).  The model is therefore a mixture over
the index k of the initial component, and

    p(x_{0:T-1} | y_{0:T-1}) = sum_k w_{T-1,k} p(x_{0:T-1} | y_{0:T-1}, k):

the smoothed weights are the filter's weights at the last step, constant in time, and smoothed component k is the RTS pass of
chain k.  ``bf_gs_smoother_f32`` (include/bayesfilt.h states the contract) runs the chains and, fused into the same kernel
for n <= 6 and K <= 64, the moment-matched single Gaussian of the smoothed mixture.  PyTorch only allocates and passes
device buffers; there is no CPU path.
"""
import ctypes as C
from typing import NamedTuple, Optional, Any

from . import _lib
from ._backward import _front, _inputs_desc, _wrapper_kw
from .inference import (_torch, _dev_f32, _alloc_stream, _stream_desc, _Model, FULL5, gaussian_sum_filter,
                        unscented_gaussian_sum_filter)


class PosteriorGaussianSumSmoothed(NamedTuple):
    """Smoothed mixture.  ``weights`` (B, K): constant in time.  Per-component arrays are shaped like the filter's,
    (B, K, T, ...) -- (K, T, ...) for one trajectory; ``smoothed_cross_covariances`` as :class:`PosteriorGaussianSmoothed`'s.
    ``collapsed_means`` (B, T, n) / ``collapsed_covariances`` (B, T, n, n): the moment match of the smoothed mixture."""
    weights: Optional[Any] = None
    filtered_means: Optional[Any] = None
    filtered_covariances: Optional[Any] = None
    smoothed_means: Optional[Any] = None
    smoothed_covariances: Optional[Any] = None
    smoothed_cross_covariances: Optional[Any] = None
    collapsed_means: Optional[Any] = None
    collapsed_covariances: Optional[Any] = None


class GaussianSumSmootherCarry(NamedTuple):
    """Smoothed state of every chain at one step, contiguous (B, K, n) / (B, K, n, n), and the mixture's weights (B, K): what
    a backward chunk hands to the chunk before it."""
    means: Any
    covariances: Any
    weights: Any


def gaussian_sum_smoother(params, posterior, *, inputs=None, weights=None, carry=None, cross_covariances: bool = False,
                          collapsed: bool = True, components: bool = True, layout: str = "reference",
                          return_carry: bool = False, uparams=None, device="cuda", options=None):
    """Smooth the K-component filtered posterior ``posterior`` (``gaussian_sum_filter``'s, or with ``uparams``
    ``unscented_gaussian_sum_filter``'s; the predicted streams are needed) backwards in time on the device.

    ``weights`` (B, K): the filter's weights at the last step of the whole series; default ``posterior.weights[..., -1]``,
    with a ``carry`` the carry's.  ``components``: return the per-component smoothed streams (with
    ``cross_covariances`` the lag-one cross-covariances too); ``collapsed``: return the moment-matched mean and covariance
    of the smoothed mixture.  With ``components=False`` nothing per component is stored where the fused kernel serves the
    call (n <= 6, K <= 64, not ``force_generic``); elsewhere the components are smoothed into scratch tensors and
    collapsed.  ``carry`` / ``return_carry``: backward chunking, as :func:`rts_smoother`
    (:class:`GaussianSumSmootherCarry`).  Returns :class:`PosteriorGaussianSumSmoothed` (and the carry).
    """
    torch = _torch()
    if not components and not collapsed:
        raise ValueError("ask for components, collapsed moments or both")
    if cross_covariances and not components:
        raise ValueError("cross_covariances needs components=True")
    bw = _front("Gaussian-sum smoother", params, posterior, True if uparams is None else None, uparams, multi=True)
    m_b, P_b, B, T, n, K, squeeze, dev = bw.m_b, bw.P_b, bw.B, bw.T, bw.n, bw.K, bw.squeeze, bw.dev

    if weights is None and carry is not None:
        weights = carry.weights
    if weights is None:
        if posterior.weights is None:
            raise ValueError("give weights=, or a posterior that holds the filter's weights")
        weights = posterior.weights[..., -1]
    w = _dev_f32(weights, dev).reshape(-1, K)
    if w.shape[0] != B:
        raise ValueError(f"weights have shape {tuple(w.shape)}, expected {(B, K)}")
    w = w.contiguous()

    c_steps = T if carry is not None else T - 1
    cr = _lib.bf_smooth_carry()
    keep = [w]
    if carry is not None:
        cm_in, cP_in = (_dev_f32(v, dev).contiguous() for v in (carry.means, carry.covariances))
        if cm_in.numel() != B * K * n or cP_in.numel() != B * K * n * n:
            raise ValueError("carry does not match (B, K, n) / (B, K, n, n)")
        keep += [cm_in, cP_in]
        cr.m_in, cr.P_in = cm_in.data_ptr(), cP_in.data_ptr()
    c_out = None
    if return_carry:
        c_out = GaussianSumSmootherCarry(torch.empty((B, K, n), dtype=torch.float32, device=dev),
                                         torch.empty((B, K, n, n), dtype=torch.float32, device=dev), w)
        cr.m_out, cr.P_out = c_out.means.data_ptr(), c_out.covariances.data_ptr()

    cmean = ccov = None
    if collapsed:
        cmean = torch.empty((B, T, n), dtype=torch.float32, device=dev)
        ccov = torch.empty((B, T, n, n), dtype=torch.float32, device=dev)

    def desc(with_components):
        ms = Ps = Cs = None
        if with_components:
            ms = _alloc_stream((B, K, T), (n,), layout, dev)
            Ps = _alloc_stream((B, K, T), (n, n), layout, dev)
            if cross_covariances:
                Cs = _alloc_stream((B, K, T), (n, n), layout, dev)[:, :, :c_steps]
        sd = _lib.bf_gs_smooth_desc()
        sd.means, sd.covs = _stream_desc(ms, 1), _stream_desc(Ps, 2)
        sd.cross_covs = _stream_desc(Cs if c_steps > 0 else None, 2)
        if collapsed:
            sd.coll_mean.ptr, sd.coll_mean.sB, sd.coll_mean.sT, sd.coll_mean.sE = cmean.data_ptr(), T * n, n, 1
            sd.coll_cov.ptr, sd.coll_cov.sB, sd.coll_cov.sT, sd.coll_cov.sE = ccov.data_ptr(), T * n * n, n * n, 1
        sd.weights = w.data_ptr()
        return sd, ms, Ps, Cs

    mdl = _Model(params)
    ud = _inputs_desc(inputs, B, T, dev, keep)
    cur = torch.cuda.current_stream(dev)

    def call(sd):
        _lib.arm_call_options(bw.lib, options)
        return bw.lib.bf_gs_smoother_f32(C.byref(mdl.c), C.byref(bw.up) if bw.up is not None else None, C.byref(ud),
                                         C.byref(bw.fd), B, T, K, C.byref(cr), C.byref(sd), C.c_void_p(cur.cuda_stream))

    sd, ms, Ps, Cs = desc(components)
    rc = call(sd)
    if rc == _lib.BF_EUNSUPPORTED and not components:
        # collapsed moments alone are not served here (K > 64, n > 6, force_generic): smooth into scratch streams, collapse those
        first = bw.lib.bf_last_error().decode()
        sd, ms, Ps, Cs = desc(True)
        rc = call(sd)
        if rc != _lib.BF_OK:
            raise _lib.BayesFiltError(rc, first + " / " + bw.lib.bf_last_error().decode())
        keep += [ms, Ps]
        ms = Ps = Cs = None
    _lib.check(rc)
    for t_ in keep:
        t_.record_stream(cur)

    sq = (lambda x: x[0] if (squeeze and x is not None) else x)
    post = PosteriorGaussianSumSmoothed(sq(w), sq(m_b), sq(P_b), sq(ms), sq(Ps), sq(Cs), sq(cmean), sq(ccov))
    return (post, c_out) if return_carry else post


def _gs_wrapper_kw(params, kw):
    """:func:`_wrapper_kw` for K components: without ``initial_means`` the filter draws them as the reference does
    (``sample_initial_component_means``), and it emits the weights too."""
    fkw, skw = _wrapper_kw(params, kw, True)
    if "initial_means" not in kw:
        fkw.pop("initial_means", None)
    fkw["fields"] = FULL5
    return fkw, skw


def extended_gaussian_sum_smoother(params, emissions, num_components, inputs=None, **kw):
    """``gaussian_sum_filter`` with ``num_components`` components, then :func:`gaussian_sum_smoother`.  Keywords of the
    filter (``initial_means``, ``initial_covariances``, ``layout``, ``device``) go to the filter, the others to the
    smoother."""
    fkw, skw = _gs_wrapper_kw(params, kw)
    post = gaussian_sum_filter(params, emissions, num_components, inputs=inputs, **fkw)
    return gaussian_sum_smoother(params, post, inputs=inputs, **skw)


def unscented_gaussian_sum_smoother(params, uparams, emissions, num_components, inputs=None, **kw):
    """``unscented_gaussian_sum_filter`` with ``num_components`` components, then :func:`gaussian_sum_smoother` on the
    unscented route."""
    fkw, skw = _gs_wrapper_kw(params, kw)
    post = unscented_gaussian_sum_filter(params, uparams, emissions, num_components, inputs=inputs, **fkw)
    return gaussian_sum_smoother(params, post, inputs=inputs, uparams=uparams, **skw)
