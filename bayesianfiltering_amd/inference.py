"""Filter drivers with the reference's call surface, running on the HIP engine.

Mirrors ``gaussfiltax/inference.py``:

* :class:`PosteriorGaussianSumFiltered`   -- inference.py:29-39 (same fields, same order)
* :func:`gaussian_sum_filter`             -- inference.py:303-377
* :func:`bootstrap_particle_filter`       -- inference.py:1302-1380

What is new is the batch axis: ``emissions`` may be ``(T, m)`` like the reference (one
trajectory; outputs shaped ``(K, T, ...)`` exactly as the reference returns them after
``swap_axes_on_values``, inference.py:372) or ``(B, T, m)`` for B independent trajectories
(outputs ``(B, K, T, ...)``).  Outputs are ``torch`` tensors on the GPU.  PyTorch is plumbing
only (device memory + streams); all arithmetic happens in the HIP kernels behind the C-ABI of
``include/bayesfilt.h``.  There is no CPU path: without the built library or without an
MI355X the calls raise.
"""
import ctypes as C
from typing import NamedTuple, Optional, Any, Sequence

import numpy as np

from . import _lib
from .nonlinearities import DeviceFunction, DYN_LINEAR, EMI_LINEAR, require_device_function

F32 = np.float32
FULL5 = ("weights", "means", "covariances", "predicted_means", "predicted_covariances")
FILTERED = ("weights", "means", "covariances")


class PosteriorGaussianSumFiltered(NamedTuple):
    """Marginals of the Gaussian-sum filtering posterior (gaussfiltax/inference.py:29-39)."""
    weights: Optional[Any] = None
    means: Optional[Any] = None
    covariances: Optional[Any] = None
    predicted_means: Optional[Any] = None
    predicted_covariances: Optional[Any] = None


def _torch():
    import torch
    return torch


def _dev_f32(x, device):
    """float32 tensor on ``device`` (no copy if it already is one)."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float32)
    return torch.as_tensor(np.asarray(x, dtype=F32), device=device)


def _host_f32(x):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=F32))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _alloc_stream(shape_bkt, event_shape, layout, device):
    """Allocate one output stream with logical shape (B, K, T, *event) in the chosen physical layout."""
    torch = _torch()
    B, K, T = shape_bkt
    ev = tuple(event_shape)
    if layout == "reference":
        return torch.empty((B, K, T) + ev, dtype=torch.float32, device=device)
    if layout == "batch_inner":
        phys = torch.empty((K, T) + ev + (B,), dtype=torch.float32, device=device)
        nd = phys.dim()
        return phys.permute((nd - 1,) + tuple(range(nd - 1)))
    raise ValueError(f"unknown layout {layout!r}")


def _stream_desc(t, n_event_dims):
    """bf_stream for a (B, K, T, *event) tensor whose event dims flatten with one stride."""
    s = _lib.bf_stream()
    if t is None:
        return s
    st = t.stride()
    if n_event_dims == 0:
        sE = 1
    elif n_event_dims == 1:
        sE = st[3]
    else:
        if st[3] != st[4] * t.shape[4]:
            raise ValueError("matrix output must be row-major-flattenable")
        sE = st[4]
    s.ptr, s.sB, s.sK, s.sT, s.sE = t.data_ptr(), st[0], st[1], st[2], sE
    return s


def _check_out_tensor(name, t, device):
    """Refuse an ``out=`` tensor the kernels cannot write: they store float32 through raw pointers on the call's device."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"out.{name} must be a torch tensor; got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"out.{name} must be float32; got {t.dtype}")
    if t.device != device:
        raise ValueError(f"out.{name} must be on {device}; got a tensor on {t.device}")


def _time_varying(x, d):
    x = _host_f32(x)
    if x.ndim == 3:
        return x, x.shape[0]
    if x.shape != (d, d):
        raise ValueError(f"covariance must be ({d},{d}) or (T,{d},{d}); got {x.shape}")
    return x, 1


class _Lgssm:
    """Host-side build of bf_lgssm from a ParamsNLSSM with linear registry functions."""

    def __init__(self, params):
        f = require_device_function(params.dynamics_function, "dynamics", "params.dynamics_function")
        h = require_device_function(params.emission_function, "emission", "params.emission_function")
        if f.fn_id != DYN_LINEAR or h.fn_id != EMI_LINEAR:
            raise ValueError("kalman_filter needs linear_dynamics / linear_emission functions")
        self.n, self.dq, self.m, self.dr = f.out_dim, f.noise_dim, h.out_dim, h.noise_dim
        if f.in_dim != self.n or h.in_dim != self.n:
            raise ValueError("dynamics / emission matrices do not match the state dimension")
        self.A, self.G = np.ascontiguousarray(f.M), np.ascontiguousarray(f.N)
        self.H, self.D = np.ascontiguousarray(h.M), np.ascontiguousarray(h.N)
        self.q0 = _host_f32(params.dynamics_noise_bias).reshape(self.dq)
        self.r0 = _host_f32(params.emission_noise_bias).reshape(self.dr)
        self.Q, self.Q_steps = _time_varying(params.dynamics_noise_covariance, self.dq)
        self.R, self.R_steps = _time_varying(params.emission_noise_covariance, self.dr)
        c = _lib.bf_lgssm()
        c.n, c.dq, c.m, c.dr = self.n, self.dq, self.m, self.dr
        c.A, c.G, c.H, c.D = _fp(self.A), _fp(self.G), _fp(self.H), _fp(self.D)
        c.q0, c.r0, c.Q, c.R = _fp(self.q0), _fp(self.r0), _fp(self.Q), _fp(self.R)
        c.Q_steps, c.R_steps = self.Q_steps, self.R_steps
        self.c = c


class ParamsUKF(NamedTuple):
    """Hyper-parameters of the unscented transform, gaussfiltax/inference.py:41-49 (same defaults)."""
    alpha: float = 1e-3
    beta: float = 2
    kappa: float = 0


class FilterCarry(NamedTuple):
    """The scan carry (weights, pred_means, pred_covs) of inference.py:334,356 at the end of a
    chunk; feed it back through ``carry=`` to continue the same trajectories."""
    weights: Any
    means: Any
    covariances: Any


def _ukf_params(uparams, extended=False):
    """``uparams`` (a :class:`ParamsUKF` or a 3-tuple) as the C struct; it excludes ``extended=True``."""
    if extended:
        raise ValueError("uparams selects the unscented route; it cannot be combined with extended=True")
    if not isinstance(uparams, ParamsUKF):
        uparams = ParamsUKF(*uparams)
    return _lib.bf_ukf_params(float(uparams.alpha), float(uparams.beta), float(uparams.kappa))


def _emissions_desc(emissions, m, device):
    """``emissions`` (T, m) or (B, T, m) on ``device`` -> (y (B, T, m), its bf_cstream, whether it was unbatched, B, T).
    Empty emissions pass: the callers that refuse them in Python do so themselves."""
    y = _dev_f32(emissions, device)
    squeeze = y.dim() == 2
    if squeeze:
        y = y.unsqueeze(0)
    if y.dim() != 3 or y.shape[2] != m:
        raise ValueError(f"emissions must be (T,{m}) or (B,T,{m}); got {tuple(y.shape)}")
    yd = _lib.bf_cstream()
    yd.ptr, yd.sB, yd.sK, yd.sT, yd.sE = y.data_ptr(), y.stride(0), 0, y.stride(1), y.stride(2)
    return y, yd, squeeze, int(y.shape[0]), int(y.shape[1])


def _inputs_desc(inputs, B, T, dev, keep):
    """bf_cstream of the filter's inputs ((T,), (T, d) or (B, T, d); None = zeros); the tensor it points into joins ``keep``."""
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


def _carry_in(carry, initial_means, initial_covariances, B, K, n, label, device, reshape_weights=False):
    """The scan's initial (weights or None, means (B, K, n), covariances (B, K, n, n)), contiguous on ``device``: a
    :class:`FilterCarry`, or initial means (K, n) / (B, K, n) and covariances (n, n) / (K, n, n) / (B, K, n, n) expanded
    over the batch.  ``label`` names K in the shape error ("1", "K", "N0")."""
    if carry is not None:
        w_in, m_in, P_in = (_dev_f32(v, device).contiguous() for v in carry)
        if reshape_weights:
            w_in = w_in.reshape(B, K)
    else:
        w_in = None
        m_in = _dev_f32(initial_means, device).reshape(-1, K, n)
        m_in = m_in.expand(B, K, n).contiguous() if m_in.shape[0] == 1 else m_in.contiguous()
        P_in = _dev_f32(initial_covariances, device)
        if P_in.dim() == 2:
            P_in = P_in.reshape(1, 1, n, n).expand(B, K, n, n).contiguous()
        else:
            P_in = P_in.reshape(-1, K, n, n)
            P_in = P_in.expand(B, K, n, n).contiguous() if P_in.shape[0] == 1 else P_in.contiguous()
    if tuple(m_in.shape) != (B, K, n) or tuple(P_in.shape) != (B, K, n, n):
        raise ValueError(f"initial means / covariances do not match (B, {label}, n) / (B, {label}, n, n)")
    return w_in, m_in, P_in


def _alloc_outputs(B, K, T, n, fields, layout, out, return_loglik, device):
    ev = {"weights": (), "means": (n,), "covariances": (n, n), "predicted_means": (n,), "predicted_covariances": (n, n)}
    bufs = {}
    for name in FULL5:
        if name in fields:
            reuse = getattr(out, name, None) if out is not None else None
            if reuse is not None:
                _check_out_tensor(name, reuse, device)
                if tuple(reuse.shape) != (B, K, T) + ev[name]:
                    raise ValueError(f"out.{name} has shape {tuple(reuse.shape)}, expected {(B, K, T) + ev[name]}")
                bufs[name] = reuse
            else:
                bufs[name] = _alloc_stream((B, K, T), ev[name], layout, device)
        else:
            bufs[name] = None
    ll = _alloc_stream((B, K, T), (), layout, device) if return_loglik else None
    od = _lib.bf_out_desc()
    od.weights = _stream_desc(bufs["weights"], 0)
    od.means = _stream_desc(bufs["means"], 1)
    od.covs = _stream_desc(bufs["covariances"], 2)
    od.pred_means = _stream_desc(bufs["predicted_means"], 1)
    od.pred_covs = _stream_desc(bufs["predicted_covariances"], 2)
    od.loglik = _stream_desc(ll, 0)
    return bufs, ll, od


def _carry_desc(carry_in, B, K, n, return_carry, device):
    """bf_carry over the initial state of :func:`_carry_in` and, with ``return_carry``, a fresh :class:`FilterCarry` to end in."""
    torch = _torch()
    w_in, m_in, P_in = carry_in
    cr = _lib.bf_carry()
    cr.w_in = w_in.data_ptr() if w_in is not None else None
    cr.m_in, cr.P_in = m_in.data_ptr(), P_in.data_ptr()
    c_out = None
    if return_carry:
        c_out = FilterCarry(torch.empty((B, K), dtype=torch.float32, device=device),
                            torch.empty((B, K, n), dtype=torch.float32, device=device),
                            torch.empty((B, K, n, n), dtype=torch.float32, device=device))
        cr.w_out, cr.m_out, cr.P_out = (t.data_ptr() for t in c_out)
    return cr, c_out


class _FilterCall:
    """What a five-stream entry point of the C-ABI takes (bf_kalman_filter_f32, bf_kalman_filter_pscan_f32, bf_gsf_ekf_f32,
    bf_ugsf_ukf_f32, bf_agsf_*_f32): the model ``mdl``, the descriptors of the observations ``yd``, the inputs ``ud``, the
    carry ``cr`` and the outputs ``od``, the sizes, and the tensors those descriptors point into, which live as long as this
    object.  Built by :func:`_filter_call` without touching the GPU; the stream is read when the call is made."""

    @property
    def stream(self):
        return _torch().cuda.current_stream(self.y.device).cuda_stream

    def unwrap(self, v):
        """``v`` as the caller sees it: without the batch axis when the emissions had none."""
        return v[0] if (self.squeeze and v is not None) else v

    def result(self, *more, aux=None):
        """The posterior; as ``(post, aux)`` when ``aux`` is given (the augmented filters), else followed by the
        log-likelihood stream and the carry-out the call asked for and by ``more``, or alone when there is none."""
        post = PosteriorGaussianSumFiltered(**{k: self.unwrap(v) for k, v in self.bufs.items()})
        if aux is not None:
            return post, aux
        extras = [self.unwrap(self.ll)] if self.ll is not None else []
        if self.c_out is not None:
            extras.append(self.c_out)
        extras += more
        return (post, *extras) if extras else post


def _filter_call(mdl, emissions, K, label, initial_means, initial_covariances, carry=None, inputs=None, fields=FULL5,
                 layout="reference", out=None, return_loglik=False, return_carry=False, device="cuda", reshape_weights=False):
    """The front half of a five-stream filter: everything its C call takes, as a :class:`_FilterCall`.  ``mdl``: a
    :class:`_Lgssm` or :class:`_Model`; ``K``: the number of components, named ``label`` in the carry's shape error;
    ``initial_means``: the caller's, or a function returning the family's default (called only when no carry is given)."""
    k = _FilterCall()
    k.mdl, k.K, n = mdl, K, mdl.n
    k.y, k.yd, k.squeeze, B, T = _emissions_desc(emissions, mdl.m, device)
    k.B, k.T = B, T
    if T == 0 or B == 0:
        raise ValueError("empty emissions")
    if carry is None and callable(initial_means):
        initial_means = initial_means()
    k.carry_in = _carry_in(carry, initial_means, initial_covariances, B, K, n, label, device, reshape_weights)
    k.bufs, k.ll, k.od = _alloc_outputs(B, K, T, n, fields, layout, out, return_loglik, k.y.device)
    k.keep = []
    k.ud = _inputs_desc(inputs, B, T, device, k.keep)
    k.cr, k.c_out = _carry_desc(k.carry_in, B, K, n, return_carry, k.y.device)
    return k


def _kalman_call(params, emissions, initial_means, initial_covariances, carry, fields, layout, out, return_loglik,
                 return_carry, device):
    """:func:`_filter_call` for the keyword set of :func:`kalman_filter`: one component that starts at ``params.initial_mean``."""
    return _filter_call(_Lgssm(params), emissions, 1, "1",
                        (lambda: _host_f32(params.initial_mean)) if initial_means is None else initial_means,
                        params.initial_covariance if initial_covariances is None else initial_covariances, carry, None, fields,
                        layout, out, return_loglik, return_carry, device, reshape_weights=True)


def _observed_mask(observed, shape, m):
    """``observed`` as a host bool array shaped like emissions of ``shape`` ((T, m) or (B, T, m)) after broadcasting: a mask
    (T,), (T, m), (B, T) or (B, T, m), read in that order where two coincide (the batched forms only with batched
    emissions).  Host work only: a mask that does not fit is refused before the device is touched."""
    torch = _torch()
    if isinstance(observed, torch.Tensor):
        observed = observed.detach().cpu().numpy()
    mask = np.asarray(observed)
    if mask.dtype != np.bool_:
        raise ValueError(f"observed must be a bool mask; got dtype {mask.dtype}")
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3) or shape[-1] != m:
        raise ValueError(f"emissions must be (T,{m}) or (B,T,{m}); got {shape}")
    T, got = shape[-2], tuple(mask.shape)
    if got == (T,):
        mask = mask.reshape(T, 1)
    elif got == (T, m):
        pass
    elif len(shape) == 3 and got == shape[:2]:
        mask = mask.reshape(shape[0], T, 1)
    elif got != shape:
        forms = f"({T},), ({T},{m})" + (f", ({shape[0]},{T}) or ({shape[0]},{T},{m})" if len(shape) == 3 else "")
        raise ValueError(f"observed must have shape {forms}; got {got}")
    return np.array(np.broadcast_to(mask, shape))   # a writable, contiguous copy


def _masked_emissions(emissions, mask, device):
    """A float32 copy of ``emissions`` on ``device`` with NaN where ``mask`` (from :func:`_observed_mask`) is false.  Always a
    new tensor: the caller's array or tensor is never written."""
    torch = _torch()
    y = _dev_f32(emissions, device)
    return torch.where(torch.as_tensor(mask, device=y.device), y, torch.full((), float("nan"), dtype=torch.float32, device=y.device))


def _missing_route(missing, observed, emissions, device, emission_dim):
    """The front of every filter that takes ``missing=`` / ``observed=``.  Returns (gaps, lib, emissions): whether the call takes
    the missing-observation entry point (``missing="nan"``, or any ``observed=`` mask), the GPU library, and the emissions --
    with a mask, a device copy with NaN where it is false.  ``emission_dim()`` gives m, and is called only with a mask.  Host
    work first: a keyword or a mask that does not fit is refused before the device is asked for."""
    if missing not in (None, "nan"):
        raise ValueError(f"missing must be None or 'nan'; got {missing!r}")
    mask = None if observed is None else _observed_mask(observed, np.shape(emissions), int(emission_dim()))
    lib = _lib.require_gpu()
    if mask is not None:
        emissions = _masked_emissions(emissions, mask, device)
    return missing == "nan" or observed is not None, lib, emissions


def _gapped_entry(family, n, m, dq, dr, from_source=False, options=None):
    """Name of the C entry point that serves a call WITH gaps.  ``family``: "kalman" (linear model, one component) or "gsf"
    (the extended Gaussian-sum filter).  The register kernels of ``bf_*_missing_f32`` take what they always took; what they
    cannot take -- Kalman: n > 8, m > 4 or m > n; Gaussian sum: registry functions with n > 8 or m > 4, functions from source
    or recorded ones with any dimension above 8 -- and every call with ``options={"force_generic": 1}`` goes to the
    run-time-dimension kernel (``bf_*_missing_anydim_f32``, include/bayesfilt_ext.h).  Pure: no library, no device."""
    force = bool(options) and int(options.get("force_generic", 0)) != 0
    if family == "kalman":
        beyond = n > 8 or m > 4 or m > n
        return "bf_kalman_filter_missing_anydim_f32" if (beyond or force) else "bf_kalman_filter_missing_f32"
    if family != "gsf":
        raise ValueError(f"unknown filter family {family!r}")
    beyond = max(n, dq, m, dr) > 8 if from_source else (n > 8 or m > 4)
    return "bf_gsf_ekf_missing_anydim_f32" if (beyond or force) else "bf_gsf_ekf_missing_f32"


def _gapped_route(name, options=None):
    """The entry point a gapped call really takes, given the name :func:`_gapped_entry` chose: an ``*_anydim_*`` name becomes
    its ``*_tiles_*`` twin (include/bayesfilt_ext2.h) -- the MISSING instance of the one-wave matrix-core kernel where the plain
    call would run that kernel, the ``*_anydim_*`` entry point itself (same refusals, same kernel, same bits) everywhere else --
    unless ``options`` sets ``force_generic``, which keeps the run-time-dimension kernel by name.  Pure: no library, no device."""
    force = bool(options) and int(options.get("force_generic", 0)) != 0
    return name if force else name.replace("_missing_anydim_", "_missing_tiles_")


def kalman_filter(params, emissions, *, initial_means=None, initial_covariances=None, carry=None,
                  fields: Sequence[str] = FULL5, layout: str = "reference", out=None,
                  return_loglik: bool = False, return_carry: bool = False, device="cuda", options=None,
                  missing=None, observed=None):
    """Batched Kalman filter == ``gaussian_sum_filter(params, y, num_components=1)`` of the
    reference for linear ``f(x,q,u) = A x + G q``, ``h(x,r,u) = H x + D r`` with the initial
    component mean given explicitly (the reference samples it from N(m0, P0) with PRNGKey(0),
    inference.py:367; pass ``initial_means=`` to choose it, default ``params.initial_mean``).

    emissions: (T, m) or (B, T, m).  Returns PosteriorGaussianSumFiltered with arrays shaped
    (1, T, ...) or (B, 1, T, ...); ``layout='batch_inner'`` returns the same logical shapes as
    strided views of a [K][T][E][B] buffer (the fastest store pattern).  ``out`` may hold a
    previously returned posterior whose buffers are reused.

    ``missing="nan"``: a NaN entry of ``emissions`` is a component that was not observed at that step
    (the update conditions on the observed rows only, a step with none is predict-only with log-likelihood 0), at any
    dimensions: ``bf_kalman_filter_missing_f32`` (register kernels) for n <= 8 and m <= min(n, 4); the MISSING instance of the
    one-wave matrix-core kernel (``bf_kalman_filter_missing_tiles_f32``, DESIGN.md 4a''') where the plain call runs that
    kernel -- 9 <= n <= 32, m <= 32 and (n >= 16 or m > 8); everywhere else -- or with ``options={"force_generic": 1}`` --
    the run-time-dimension kernel (``bf_kalman_filter_missing_anydim_f32``, DESIGN.md 4a'', as far as its 160 KiB of LDS go;
    a gapped model with 33 <= n <= 64 leaves the four-wave matrix-core route for it).  Without it a NaN
    poisons its trajectory from that step on, as ever.  +-Inf is never
    "missing".  ``observed``: a bool mask of shape (T,), (B, T), (T, m) or (B, T, m), true where the entry was observed; it
    implies ``missing="nan"`` and the filter runs on a device copy of the emissions with NaN where the mask is false.
    """
    gaps, lib, emissions = _missing_route(missing, observed, emissions, device, lambda: _Lgssm(params).m)
    k = _kalman_call(params, emissions, initial_means, initial_covariances, carry, fields, layout, out, return_loglik,
                     return_carry, device)
    _lib.arm_call_options(lib, options)      # tuning options for THIS call only (bf_set_call_option)
    entry = getattr(lib, _gapped_route(_gapped_entry("kalman", k.mdl.n, k.mdl.m, k.mdl.dq, k.mdl.dr, False, options), options)) if gaps else lib.bf_kalman_filter_f32
    _lib.check(entry(C.byref(k.mdl.c), C.byref(k.yd), k.B, k.T, C.byref(k.cr), C.byref(k.od), C.c_void_p(k.stream)))
    return k.result()


def _param_dims(params):
    """(state_dim, state-noise dim, emission-noise dim) read off the parameter arrays (for recording Python functions)."""
    n0 = int(_host_f32(params.initial_mean).size)
    Qs, Rs = tuple(np.shape(params.dynamics_noise_covariance)), tuple(np.shape(params.emission_noise_covariance))
    return n0, (int(Qs[-1]) if len(Qs) >= 2 else 1), (int(Rs[-1]) if len(Rs) >= 2 else 1)


class _Model:
    """Host-side build of bf_model from a ParamsNLSSM / ParamsBPF holding registry functions."""

    def __init__(self, params, log_prob_source=None):
        # (a plain Python function of NumPy operations is recorded and compiled: its dimensions come from the parameters)
        f, h = params.dynamics_function, params.emission_function
        if not (isinstance(f, DeviceFunction) and isinstance(h, DeviceFunction)):
            n0, dq0, dr0 = _param_dims(params)
            f = require_device_function(f, "dynamics", "params.dynamics_function", n0, dq0)
            h = require_device_function(h, "emission", "params.emission_function", n0, dr0)
        f = require_device_function(f, "dynamics", "params.dynamics_function")
        h = require_device_function(h, "emission", "params.emission_function")
        self.n, self.dq, self.m, self.dr = f.out_dim, f.noise_dim, h.out_dim, h.noise_dim
        if f.in_dim != self.n or h.in_dim != self.n:
            raise ValueError("dynamics / emission functions do not match the state dimension")
        self.dyn_theta = np.ascontiguousarray(f.theta if f.theta.size else np.zeros(1, F32))
        self.emi_theta = np.ascontiguousarray(h.theta if h.theta.size else np.zeros(1, F32))
        self.q0 = _host_f32(params.dynamics_noise_bias).reshape(self.dq)
        self.r0 = _host_f32(params.emission_noise_bias).reshape(self.dr)
        # (T, d, d) covariances vary in time exactly as _get_params(x, 2, t) selects them (inference.py:21)
        self.Q, self.Q_steps = _time_varying(params.dynamics_noise_covariance, self.dq)
        self.R, self.R_steps = _time_varying(params.emission_noise_covariance, self.dr)
        c = _lib.bf_model()
        c.dyn_id, c.emi_id, c.n, c.dq, c.m, c.dr = f.fn_id, h.fn_id, self.n, self.dq, self.m, self.dr
        c.dyn_theta, c.n_dyn_theta = _fp(self.dyn_theta), int(f.theta.size)
        c.emi_theta, c.n_emi_theta = _fp(self.emi_theta), int(h.theta.size)
        c.q0, c.r0, c.Q, c.R = _fp(self.q0), _fp(self.r0), _fp(self.Q), _fp(self.R)
        c.Q_steps, c.R_steps = self.Q_steps, self.R_steps
        # functions given as source text (nonlinearities.user_dynamics / user_emission): compiled once per source by hiprtc
        dsrc = getattr(f, "source", None)
        esrc = getattr(h, "source", None)
        if dsrc is not None or esrc is not None or log_prob_source is not None:
            c.user = _compile_user_model(dsrc, esrc, self.n, self.dq, self.m, self.dr, log_prob_source)
        self.c = c


_USER_MODELS = {}


def _compile_user_model(dyn_src, emi_src, n, dq, m, dr, lp_src=None):
    """bf_user_model_create(_lp), memoised per (sources, dimensions); returns the opaque handle."""
    key = (dyn_src, emi_src, lp_src, n, dq, m, dr)
    h = _USER_MODELS.get(key)
    if h is None:
        lib = _lib.require_gpu()
        out = C.c_void_p()
        enc = lambda t: t.encode() if t is not None else None
        _lib.check(lib.bf_user_model_create_lp(enc(dyn_src), enc(emi_src), enc(lp_src), n, dq, m, dr, C.byref(out)))
        h = _USER_MODELS[key] = out.value
    return h


def PRNGKey(seed: int):
    """jax.random.PRNGKey for the default threefry PRNG: uint32 [hi32(seed), lo32(seed)]."""
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], dtype=np.uint32)


def _random_normal(key, count):
    lib = _lib.load()
    key = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
    out = np.empty(count, dtype=F32)
    _lib.check(lib.bf_random_normal_f32(key.ctypes.data_as(C.POINTER(C.c_uint32)), count, _fp(out)))
    return out


def sample_initial_component_means(params, num_components, key=None):
    """The draw of gaussfiltax/inference.py:367: ``MVN(m0, P0).sample(K, PRNGKey(0))`` restated as
    ``m0 + chol(P0) @ normal(key, (K, n))[k]`` (tfp's sampler is third-party; best-effort stream)."""
    key = PRNGKey(0) if key is None else key
    m0 = _host_f32(params.initial_mean).reshape(-1)
    L = np.linalg.cholesky(_host_f32(params.initial_covariance).astype(np.float64)).astype(F32)
    z = _random_normal(key, num_components * m0.size).reshape(num_components, m0.size)
    return (m0[None, :] + z @ L.T).astype(F32)


def gaussian_sum_filter(params, emissions, num_components: int = 1, num_iter: int = 1, inputs=None, *,
                        initial_means=None, initial_covariances=None, carry=None,
                        fields: Sequence[str] = FULL5, layout: str = "reference", out=None,
                        return_loglik: bool = False, return_carry: bool = False, return_collapsed: bool = False,
                        device="cuda", options=None, _uparams=None, missing=None, observed=None):
    """Gaussian-sum filter (bank of K extended Kalman filters + weight update),
    gaussfiltax/inference.py:303-377, on the HIP engine.

    Same positional signature as the reference.  ``num_iter`` is accepted and ignored exactly as
    there (:307, never read).  ``emissions``: (T, m) -> arrays shaped (K, T, ...) like the
    reference, or (B, T, m) -> (B, K, T, ...).  ``inputs``: None (zeros((T,1)), :23), (T,), (T, d)
    or (B, T, d); the registry functions use ``u[0]``.  ``initial_means`` (K, n) / (B, K, n)
    overrides the reference's fixed ``MVN(m0, P0).sample(K, PRNGKey(0))`` draw (:367).
    ``carry`` / ``return_carry`` continue a scan in chunks (the carry of :334,356).
    ``return_collapsed`` appends ``(mean (T, n), covariance (T, n, n))`` of the moment-matched single
    Gaussian of the filtered mixture at every step (utils.collapse, utils.py:10-18; the point estimate of
    BOT_Experiment_script.py:101), formed inside the scan: with ``fields=()`` a K-component run then
    returns 4(n + n^2) bytes per step instead of the K-fold streams (COLLAPSED mode).

    ``missing="nan"``: a NaN entry of ``emissions`` is a component that was not observed at that step
    (``bf_gsf_ekf_missing_f32``, DESIGN.md 4b'): every component of the bank conditions on the observed rows only, a step with
    none leaves means and covariances untouched with log-likelihood 0 (the weights are renormalised only), trailing gaps are a
    forecast.  Any dimensions: the register kernels take registry models with n <= 8 and m <= 4 and models from source with
    every dimension <= 8; models the plain call runs on the one-wave matrix-core kernel (9 <= n <= 32, linear emission,
    linear / Lorenz-96 / sine dynamics, K <= 64, per-step tables included) run on its MISSING instance
    (``bf_gsf_ekf_missing_tiles_f32``, DESIGN.md 4a'''); everything else -- and any call with
    ``options={"force_generic": 1}`` -- runs on the run-time-dimension kernel (``bf_gsf_ekf_missing_anydim_f32``, DESIGN.md
    4a''; no collapsed streams on either).  The unscented
    bank keeps its limit (every dimension <= 8).  Without it a NaN poisons its trajectory, as ever; +-Inf is never "missing".
    ``observed``: a bool mask of shape (T,), (B, T), (T, m) or (B, T, m), true where the entry was observed; it implies
    ``missing="nan"`` (see :func:`kalman_filter`).
    """
    torch = _torch()
    K = int(num_components)
    if K < 1:
        raise ValueError("num_components must be >= 1")

    def emission_dim():   # (m from the model dimensions)
        h = params.emission_function
        if not isinstance(h, DeviceFunction):   # a plain Python function: recorded on the host, as _Model does
            n0, _, dr0 = _param_dims(params)
            h = require_device_function(h, "emission", "params.emission_function", n0, dr0)
        return h.out_dim
    gaps, lib, emissions = _missing_route(missing, observed, emissions, device, emission_dim)
    k = _filter_call(_Model(params), emissions, K, "K",
                     (lambda: sample_initial_component_means(params, K)) if initial_means is None else initial_means,
                     params.initial_covariance if initial_covariances is None else initial_covariances, carry, inputs, fields,
                     layout, out, return_loglik, return_carry, device)
    B, T, n, od = k.B, k.T, k.mdl.n, k.od
    coll = ()
    if return_collapsed:
        coll = (torch.empty((B, T, n), dtype=torch.float32, device=k.y.device),
                torch.empty((B, T, n, n), dtype=torch.float32, device=k.y.device))
        od.coll_mean.ptr, od.coll_mean.sB, od.coll_mean.sK, od.coll_mean.sT, od.coll_mean.sE = coll[0].data_ptr(), T * n, 0, n, 1
        od.coll_cov.ptr, od.coll_cov.sB, od.coll_cov.sK, od.coll_cov.sT, od.coll_cov.sE = coll[1].data_ptr(), T * n * n, 0, n * n, 1
        coll = (tuple(k.unwrap(v) for v in coll),)
    # (_uparams: the unscented bank -- same carry / streams, sigma-point moment matching instead of Jacobians)
    if _uparams is None:
        c = k.mdl.c
        fn = getattr(lib, _gapped_route(_gapped_entry("gsf", c.n, c.m, c.dq, c.dr, bool(c.user), options), options)) if gaps else lib.bf_gsf_ekf_f32
        head = ()
    else:
        fn, head = (lib.bf_ugsf_ukf_missing_f32 if gaps else lib.bf_ugsf_ukf_f32), (C.byref(_uparams),)
    _lib.arm_call_options(lib, options)      # tuning options for THIS call only (bf_set_call_option)
    _lib.check(fn(C.byref(k.mdl.c), *head, C.byref(k.yd), C.byref(k.ud), B, T, K, C.byref(k.cr), C.byref(od),
                  C.c_void_p(k.stream)))
    return k.result(*coll)


def unscented_gaussian_sum_filter(params, uparams, emissions, num_components: int = 1, num_iter: int = 1, inputs=None, *,
                                  initial_means=None, initial_covariances=None, carry=None,
                                  fields: Sequence[str] = FULL5, layout: str = "reference", out=None,
                                  return_loglik: bool = False, return_carry: bool = False, device="cuda", options=None,
                                  missing=None, observed=None):
    """Unscented Gaussian-sum filter (bank of K unscented Kalman filters with non-additive noise +
    weight update), gaussfiltax/inference.py:379-456, on the HIP engine.

    Same positional signature as the reference (``uparams``: :class:`ParamsUKF`; ``num_iter`` ignored as
    there).  Sigma points follow ``utils._get_sigma_points`` (utils.py:247-254): the symmetric square root
    of blockdiag(P, noise covariance), recomputed on the device twice per step.  Shapes, ``initial_means``,
    ``carry`` / ``return_carry``, ``fields`` and ``return_loglik`` as in :func:`gaussian_sum_filter`.

    State, noise and observation dimensions up to 8 run with the state in registers (at most 256 components); anything larger
    runs on the run-time-dimension kernel (state in LDS, any number of components, bounded by 160 KiB of LDS: about n = 70 with
    n / 2 observations).  ``options={"ugsf_force_generic": 1}`` sends a small model through that kernel too.

    ``missing`` / ``observed``: NaN entries as gaps, as in :func:`gaussian_sum_filter` (``bf_ugsf_ukf_missing_f32``: the sigma
    points are those of the full augmented state, the update reads the observed rows only; every dimension <= 8).
    """
    return gaussian_sum_filter(params, emissions, num_components, num_iter, inputs, initial_means=initial_means,
                               initial_covariances=initial_covariances, carry=carry, fields=fields, layout=layout, out=out,
                               return_loglik=return_loglik, return_carry=return_carry, device=device, options=options,
                               _uparams=_ukf_params(uparams), missing=missing, observed=observed)


def speedy_augmented_gaussian_sum_filter(params, emissions, num_components, rng_key=None, num_iter: int = 1,
                                         opt_args=(0.1, 0.1), inputs=None, *, initial_means=None,
                                         initial_covariances=None, carry=None, return_carry: bool = False,
                                         return_leaf_indices: bool = False, device="cuda", options=None, _variant=0,
                                         _uparams=None):
    """"Speedy" augmented Gaussian-sum filter, gaussfiltax/inference.py:621-812, on the HIP engine.

    Same positional signature as the reference: ``num_components = (N0, N1, N2)``, ``rng_key`` defaults to
    ``PRNGKey(0)`` (the reference never advances it: the same normals at every step), ``num_iter`` is
    ignored as there, ``opt_args = (a0, a1)`` scale the sample covariances Delta = a0 P and Lambda = a1 P-.
    Returns ``(PosteriorGaussianSumFiltered(weights, means, covariances), aux)`` with arrays shaped
    (N0, T, ...) for ``emissions`` (T, m) -- or with a leading batch axis for (B, T, m); ``aux`` is a dict
    that holds ``'leaf_indices'`` (T, N0) when ``return_leaf_indices`` (the reference's per-step debugging
    outputs -- Deltas, Lambdas, Jacobians, gains -- are not materialised) and ``'carry'`` when
    ``return_carry``.  ``initial_means`` (N0, n) overrides the fixed ``MVN(m0, P0).sample(N0, PRNGKey(0))``
    draw (:799).  ``options``: tuning options for this call only, as in :func:`gaussian_sum_filter`.

    Limits.  While the state, noise and observation dimensions are all <= 8 a leaf lives in the registers of one lane:
    N0 * N1 * N2 <= 64 in general, <= 1024 for state_dim <= 4; a nonlinear registry model needs one of the compiled
    (state_dim, obs_dim) pairs.  Any dimension above 8 -- or ``options={"agsf_force_generic": 1}`` for a small model -- runs on
    the run-time-dimension kernel (the tree's nodes take turns in LDS): registry functions at any dimension the 160 KiB of LDS
    of a workgroup hold (n = 76 with n / 2 observations for extended nodes, n = 63 for unscented ones; the error names the
    bytes needed), N0 * N1 * N2 <= 256.  Functions from source and recorded Python functions stay at dimensions up to 8.
    """
    torch = _torch()
    lib = _lib.require_gpu()
    nc = np.ascontiguousarray(np.asarray(num_components, dtype=np.int32).reshape(-1))
    if nc.size != 3 or np.any(nc < 1):
        raise ValueError("num_components must hold three positive counts (N0, N1, N2)")
    N0 = int(nc[0])
    k = _filter_call(_Model(params), emissions, N0, "N0",
                     (lambda: sample_initial_component_means(params, N0)) if initial_means is None else initial_means,
                     params.initial_covariance if initial_covariances is None else initial_covariances, carry, inputs, FILTERED,
                     return_carry=return_carry, device=device)
    key = np.ascontiguousarray(np.asarray(PRNGKey(0) if rng_key is None else rng_key, dtype=np.uint32).reshape(2))
    opt = np.ascontiguousarray(np.asarray(opt_args, dtype=F32).reshape(2))
    leaf = torch.empty((k.B, k.T, N0), dtype=torch.int32, device=k.y.device) if return_leaf_indices else None
    fn, head = (lib.bf_agsf_ekf_f32, ()) if _uparams is None else (lib.bf_agsf_ukf_f32, (C.byref(_uparams),))
    _lib.arm_call_options(lib, options)      # tuning options for THIS call only (bf_set_call_option)
    _lib.check(fn(C.byref(k.mdl.c), *head, C.byref(k.yd), C.byref(k.ud), k.B, k.T, nc.ctypes.data_as(C.POINTER(C.c_int32)),
                  key.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(opt), C.byref(k.cr), C.byref(k.od),
                  C.c_void_p(leaf.data_ptr() if leaf is not None else None), int(_variant), C.c_void_p(k.stream)))
    aux = {}
    if return_leaf_indices:
        aux["leaf_indices"] = k.unwrap(leaf)
    if return_carry:
        aux["carry"] = k.c_out
    return k.result(aux=aux)


def augmented_gaussian_sum_filter(params, emissions, num_components, rng_key=None, num_iter: int = 1, opt_args=(0.1, 0.1),
                                  inputs=None, **kwargs):
    """Augmented Gaussian-sum filter, gaussfiltax/inference.py:458-620, on the HIP engine: the same tree
    as :func:`speedy_augmented_gaussian_sum_filter` with the branches drawn as ``containers._branches_from_tree1/2``
    draw them (containers.py:63-140: one key per node, ``jr.multivariate_normal`` per node, NaN samples
    replaced by the node mean).  The reference needs its module globals ``num_prt1`` / ``num_prt2``
    (containers.py:13-14) edited by hand to match ``num_components``; here they are ``num_components[1:]``.
    Same arguments, return value and keyword extensions as the speedy variant."""
    return speedy_augmented_gaussian_sum_filter(params, emissions, num_components, rng_key, num_iter, opt_args, inputs,
                                                _variant=1, **kwargs)


def speedy_unscented_agsf(params, uparams, emissions, num_components, rng_key=None, num_iter: int = 1, opt_args=(0.1, 0.1),
                          inputs=None, **kwargs):
    """Augmented Gaussian-sum filter with unscented nodes, gaussfiltax/inference.py:966-1156, on the HIP engine:
    :func:`speedy_augmented_gaussian_sum_filter` with ``_ukf_predict_nonadditive`` / ``_ukf_condition_on_nonadditive``
    at the tree nodes.  Same positional signature as the reference (``uparams``: :class:`ParamsUKF`)."""
    return speedy_augmented_gaussian_sum_filter(params, emissions, num_components, rng_key, num_iter, opt_args, inputs,
                                                _uparams=_ukf_params(uparams), **kwargs)


def unscented_agsf(params, uparams, emissions, num_components, rng_key=None, num_iter: int = 1, opt_args=(0.1, 0.1), inputs=None,
                   **kwargs):
    """gaussfiltax/inference.py:813-965: the unscented augmented filter with the container-based branches of
    :func:`augmented_gaussian_sum_filter`."""
    return speedy_augmented_gaussian_sum_filter(params, emissions, num_components, rng_key, num_iter, opt_args, inputs,
                                                _variant=1, _uparams=_ukf_params(uparams), **kwargs)


def augmented_gaussian_sum_filter_optimal(params, emissions, num_components, rng_key=None, num_iter: int = 1,
                                          opt_args=(0.1, 0.1), inputs=None, **kwargs):
    """gaussfiltax/inference.py:1157-1300 on the HIP engine: :func:`augmented_gaussian_sum_filter` with
    ``utils.optimal_resampling`` (utils.py:216-244) in place of ``jr.choice``: the N0 retained components carry
    unequal weights (``post.weights``).  ``_autocov1`` / ``_autocov2`` reduce to Delta = a0 P, Lambda = a1 P-
    as in the reference's active code (:300, :338)."""
    return speedy_augmented_gaussian_sum_filter(params, emissions, num_components, rng_key, num_iter, opt_args, inputs,
                                                _variant=2, **kwargs)


def optimal_resampling(weights, N: int, key, device="cuda"):
    """``utils.optimal_resampling(weights, N, key)`` (utils.py:216-244) on the device: weights (M,) or (B, M) with
    M <= 1024 -> (indices (N,), weights (N,)) or batched."""
    torch = _torch()
    lib = _lib.require_gpu()
    w = _dev_f32(weights, device).contiguous()
    squeeze = w.dim() == 1
    if squeeze:
        w = w.unsqueeze(0)
    B, M = int(w.shape[0]), int(w.shape[1])
    key = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
    idx = torch.empty((B, int(N)), dtype=torch.int32, device=w.device)
    wo = torch.empty((B, int(N)), dtype=torch.float32, device=w.device)
    stream = torch.cuda.current_stream(w.device).cuda_stream
    _lib.check(lib.bf_optimal_resample_f32(C.c_void_p(w.data_ptr()), key.ctypes.data_as(C.POINTER(C.c_uint32)), B, M, int(N),
                                           C.c_void_p(idx.data_ptr()), C.c_void_p(wo.data_ptr()), C.c_void_p(stream)))
    return (idx[0], wo[0]) if squeeze else (idx, wo)


class ParticleCarry(NamedTuple):
    """The scan carry (weights, particles, key) of inference.py:1364 at the end of a chunk."""
    weights: Any
    particles: Any
    key: Any


def bootstrap_particle_filter(params, emissions, num_particles: int, key=None, inputs=None,
                              ess_threshold: float = 0.5, *, resampler: str = "multinomial", output: str = "full",
                              carry=None, return_carry: bool = False, return_ancestors: bool = False, device="cuda", options=None,
                              missing=None, observed=None):
    """Bootstrap particle filter, gaussfiltax/inference.py:1302-1380, on the HIP engine.

    Same positional signature as the reference (``key`` defaults to ``PRNGKey(0)``).  Returns the
    reference's dict ``{'weights': (N, T), 'particles': (N, T, n)}`` for ``emissions`` of shape
    (T, m), or with a leading batch axis for (B, T, m).  ``output='summary'`` returns per-step
    summaries instead (``mean`` (T, n), ``ess``, ``logz``, ``resampled`` (T,)) -- the full history of a
    large run does not fit in HBM; ``output='both'`` returns everything.  ``resampler`` is
    'multinomial' (the reference's ``jr.choice``, utils.py:207-214) or 'systematic'.
    ``params.emission_distribution_log_prob`` must be a :class:`~.nonlinearities.GaussianLogProb`.

    ``missing="nan"``: a NaN entry of ``emissions`` is a component that was not observed at that step (``bf_bpf_missing_f32``,
    DESIGN.md 4c', on every kernel route).  Propagation and the keys a step consumes never change; with nothing missing the
    results are the plain call's bit for bit.  A Gaussian density (``gaussian_log_prob`` / ``stoch_vol_log_prob``) weighs a partly
    observed step by the density of its observed components, ``log N(y_o; h(x)_o, (R_lp)_oo)``.  A step with nothing observed
    gives every particle log-weight 0 and runs the unchanged reweight: the weights are the previous ones renormalised, ``logz``
    is within an ulp of 0 (not exactly 0), trailing gaps are a forecast, and ``sum_t logz`` is the log-evidence of the observed
    entries.  A density of the caller's (``user_log_prob`` source, or a recorded Python function) is not called at a wholly missing
    step; a PARTLY observed step is handed to it as it is, NaN entries included -- the package cannot marginalise a density it
    does not know, so only a function that treats NaN itself (per component ``y[a] != y[a] ? 0 : ...``) takes partial gaps.
    Without the keyword a NaN poisons its trajectory from that step on, as ever; +-Inf is never "missing".  ``observed``: a bool
    mask of shape (T,), (B, T), (T, m) or (B, T, m), true where the entry was observed; it implies ``missing="nan"`` and the
    filter runs on a device copy of the emissions with NaN where the mask is false (see :func:`kalman_filter`).
    """
    from .nonlinearities import GaussianLogProb, UserLogProb
    if not hasattr(params, "emission_distribution_log_prob"):
        raise TypeError("params must be a ParamsBPF (with an emission_distribution_log_prob); got " + type(params).__name__)
    torch = _torch()

    def emission_dim():   # (m from the model dimensions)
        n0, _, dr0 = _param_dims(params)
        return require_device_function(params.emission_function, "emission", "params.emission_function", n0, dr0).out_dim
    gaps, lib, emissions = _missing_route(missing, observed, emissions, device, emission_dim)
    NP = int(num_particles)
    if NP < 1:
        raise ValueError("num_particles must be >= 1")
    if resampler not in ("multinomial", "systematic"):
        raise ValueError("resampler must be 'multinomial' or 'systematic'")
    if output not in ("full", "summary", "both"):
        raise ValueError("output must be 'full', 'summary' or 'both'")
    lp = params.emission_distribution_log_prob
    if not isinstance(lp, (GaussianLogProb, UserLogProb)) and callable(lp):
        # a plain Python function of NumPy operations: recorded and compiled (nonlinearities.trace_log_prob)
        from .nonlinearities import trace_log_prob
        from .trace import TraceError
        n0, _, dr0 = _param_dims(params)
        h0 = require_device_function(params.emission_function, "emission", "params.emission_function", n0, dr0)
        try:
            lp = trace_log_prob(lp, n0, h0.out_dim)
        except TraceError as e:
            raise TypeError(f"params.emission_distribution_log_prob: {e}") from e
    if not isinstance(lp, (GaussianLogProb, UserLogProb)):
        raise TypeError("params.emission_distribution_log_prob must be a nonlinearities.GaussianLogProb (around a registry or "
                        "source emission function) or a nonlinearities.user_log_prob(source, ...): Python callables cannot run "
                        "inside the HIP kernels, and there is no CPU fallback.")
    user_lp = isinstance(lp, UserLogProb)
    if not user_lp and lp.emission_function is not params.emission_function and \
            (lp.emission_function.fn_id != params.emission_function.fn_id or
             not np.array_equal(lp.emission_function.theta, params.emission_function.theta) or
             getattr(lp.emission_function, "source", None) != getattr(params.emission_function, "source", None)):
        raise ValueError("the log-prob's emission function must be params.emission_function")
    mdl = _Model(params, lp.source if user_lp else None)
    n, m = mdl.n, mdl.m
    bm = _lib.bf_bpf_model()
    bm.ssm = mdl.c
    m0 = _host_f32(params.initial_mean).reshape(n)
    P0 = _host_f32(params.initial_covariance).reshape(n, n)
    if user_lp:      # the density is the caller's function: no covariance, its own parameters
        lpc = np.ascontiguousarray(np.eye(m, dtype=F32))
        rev = np.zeros(mdl.dr, F32)
        lpth = np.ascontiguousarray(lp.theta if lp.theta.size else np.zeros(1, F32))
        bm.lp_theta, bm.n_lp_theta = _fp(lpth), int(lp.theta.size)
    else:
        lpc = np.ascontiguousarray(lp.covariance.reshape(m, m))
        rev = np.ascontiguousarray(lp.r_eval.reshape(mdl.dr))
    bm.m0, bm.P0, bm.lp_cov, bm.r_eval = _fp(m0), _fp(P0), _fp(lpc), _fp(rev)

    y, yd, squeeze, B, T = _emissions_desc(emissions, m, device)   # (empty emissions: the C entry point refuses them)
    dev = y.device
    keep = []
    ud = _inputs_desc(inputs, B, T, device, keep)

    key = PRNGKey(0) if key is None else np.asarray(key, dtype=np.uint32).reshape(2)
    key_c = (C.c_uint32 * 2)(int(key[0]), int(key[1]))

    od = _lib.bf_bpf_out()
    res = {}
    if output in ("full", "both"):
        res["weights"] = torch.empty((B, NP, T), dtype=torch.float32, device=dev)
        res["particles"] = torch.empty((B, NP, T, n), dtype=torch.float32, device=dev)
        od.weights, (od.w_sB, od.w_sN, od.w_sT) = res["weights"].data_ptr(), res["weights"].stride()
        od.particles, (od.x_sB, od.x_sN, od.x_sT) = res["particles"].data_ptr(), res["particles"].stride()[:3]
    if return_ancestors:
        if output == "summary":
            raise ValueError("ancestors need output='full' or 'both'")
        res["ancestors"] = torch.empty((B, NP, T), dtype=torch.int32, device=dev)
        od.ancestors = res["ancestors"].data_ptr()
    if output in ("summary", "both"):
        res["mean"] = torch.empty((B, T, n), dtype=torch.float32, device=dev)
        for k in ("ess", "logz", "resampled"):
            res[k] = torch.empty((B, T), dtype=torch.float32, device=dev)
        od.mean, od.ess, od.logz, od.resampled = (res[k].data_ptr() for k in ("mean", "ess", "logz", "resampled"))

    cr = _lib.bf_bpf_carry()
    if carry is not None:
        w_in = _dev_f32(carry.weights, device).reshape(B, NP).contiguous()
        x_in = _dev_f32(carry.particles, device).reshape(B, NP, n).contiguous()
        k_in = torch.as_tensor(np.asarray(carry.key.cpu() if hasattr(carry.key, "cpu") else carry.key, dtype=np.int64)
                               .astype(np.uint32).view(np.int32).reshape(B, 2), device=dev)
        keep += [w_in, x_in, k_in]
        cr.x_in, cr.w_in, cr.key_in = x_in.data_ptr(), w_in.data_ptr(), k_in.data_ptr()
    c_out = None
    if return_carry:
        c_out = ParticleCarry(torch.empty((B, NP), dtype=torch.float32, device=dev),
                              torch.empty((B, NP, n), dtype=torch.float32, device=dev),
                              torch.empty((B, 2), dtype=torch.int32, device=dev))
        cr.w_out, cr.x_out, cr.key_out = c_out.weights.data_ptr(), c_out.particles.data_ptr(), c_out.key.data_ptr()

    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.arm_call_options(lib, options)      # tuning options for THIS call only (bf_set_call_option)
    entry = lib.bf_bpf_missing_f32 if gaps else lib.bf_bpf_f32
    _lib.check(entry(C.byref(bm), C.byref(yd), C.byref(ud), B, T, NP, key_c, float(ess_threshold),
                     1 if resampler == "systematic" else 0, C.byref(cr), C.byref(od), C.c_void_p(stream)))
    if squeeze:
        res = {k: v[0] for k, v in res.items()}
    if return_carry:
        c_out = ParticleCarry(c_out.weights, c_out.particles,
                              torch.as_tensor(c_out.key.cpu().numpy().view(np.uint32).astype(np.int64)))
        return res, c_out
    return res


def resample_indices(weights, keys, resampler: str = "multinomial"):
    """The index draw of ``_resample`` (gaussfiltax/utils.py:210) alone:
    ``jr.choice(key, N, (N,), p=weights)`` per row.  weights (B, N), keys (B, 2) uint32."""
    torch = _torch()
    lib = _lib.require_gpu()
    w = _dev_f32(weights, "cuda").contiguous()
    if w.dim() == 1:
        w = w.unsqueeze(0)
    B, NP = w.shape
    k = torch.as_tensor(np.asarray(keys, dtype=np.uint32).reshape(B, 2).view(np.int32), device=w.device)
    idx = torch.empty((B, NP), dtype=torch.int32, device=w.device)
    stream = torch.cuda.current_stream(w.device).cuda_stream
    _lib.check(lib.bf_resample_f32(w.data_ptr(), k.data_ptr(), B, NP, 1 if resampler == "systematic" else 0,
                                   idx.data_ptr(), C.c_void_p(stream)))
    return idx
