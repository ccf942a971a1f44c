"""Posterior sampler, no GPU: the float64 test oracle (``ffbs_f64``, the contract of csrc/ffbs_sampler.hpp) pinned against
the exact dense joint Gaussian of a linear model, its behaviour on rank-deficient conditional covariances, and the
argument checks of the Python and C entry points that fail before any device work."""
import ctypes as C

import numpy as np
import pytest

from tests import common as cm
from tests.test_smoother_cpu import kalman_f64, dense_posterior

F64 = np.float64
TAU = 2.0 ** -17


# ---- float64 oracle (the GPU tests import it) -------------------------------------------------------------------------
def psdchol_f64(S, d, pivots=None):
    """Left-looking Cholesky without pivoting of the lower triangle of S; a pivot not greater than TAU * d[j] zeroes
    column j, diagonal included.  ``pivots``: a list that receives (p_j / d_j, kept) for every pivot."""
    n = S.shape[0]
    L = np.zeros((n, n), F64)
    for j in range(n):
        p = S[j, j] - L[j, :j] @ L[j, :j]
        keep = p > TAU * d[j]
        if pivots is not None:
            pivots.append((p / d[j], bool(keep)))
        if keep:
            L[j, j] = np.sqrt(p)
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ffbs_f64(m, P, pm, pP, F, xi, carry=None, pivots=None):
    """The backward-sampling recursion of csrc/ffbs_sampler.hpp in float64 for ONE trajectory: m (T, n), P (T, n, n),
    predictions pm / pP at index t = m-_{t+1}, P-_{t+1}; F (T, n, n) or (n, n) the dynamics Jacobian of step t; xi
    (..., T, n) standard normals (leading axes = samples).  carry = x (..., n) at the step after the last one.
    ``pivots``: a list that receives one list of (p_j / d_j, kept) per factorised step, last step first.
    Returns x (..., T, n)."""
    m, P, pm, pP = (np.asarray(x, F64) for x in (m, P, pm, pP))
    F, xi = np.asarray(F, F64), np.asarray(xi, F64)
    T, n = m.shape
    x = np.empty(xi.shape, F64)

    def factor(Sig, d):
        rec = [] if pivots is not None else None
        L = psdchol_f64(Sig, d, rec)
        if pivots is not None:
            pivots.append(rec)
        return L

    if carry is None:
        L = factor(P[T - 1], np.diag(P[T - 1]))
        x[..., T - 1, :] = m[T - 1] + xi[..., T - 1, :] @ L.T
        nxt, t0 = x[..., T - 1, :], T - 2
    else:
        nxt, t0 = np.asarray(carry, F64), T - 1
    for t in range(t0, -1, -1):
        Ft = F[t] if F.ndim == 3 else F
        Lp = np.linalg.cholesky(pP[t])
        W = np.linalg.solve(Lp, Ft @ P[t])
        G = np.linalg.solve(Lp.T, W).T
        low = np.tril(P[t])
        Sig = low + np.tril(P[t], -1).T - W.T @ W   # the lower triangle of P_t, mirrored: symmetric by construction
        L = factor(Sig, np.diag(P[t]))
        nxt = m[t] + (nxt - pm[t]) @ G.T + xi[..., t, :] @ L.T
        x[..., t, :] = nxt
    return x


def affine_map(m, P, pm, pP, F):
    """xi -> x is affine: x0 (T n,) at xi = 0 and the matrix M (T n, T n) of the unit vectors."""
    T, n = np.asarray(m).shape
    xi = np.concatenate([np.zeros((1, T, n)), np.eye(T * n).reshape(T * n, T, n)])
    x = ffbs_f64(m, P, pm, pP, F, xi).reshape(T * n + 1, T * n)
    return x[0], (x[1:] - x[0]).T


def joint_blocks(M, T, n):
    Sig = M @ M.T
    blk = lambda t: slice(t * n, (t + 1) * n)
    return (np.stack([Sig[blk(t), blk(t)] for t in range(T)]),
            np.stack([Sig[blk(t), blk(t + 1)] for t in range(T - 1)]))


# ---- 1: the oracle against the exact joint posterior -----------------------------------------------------------------
@pytest.mark.parametrize("n,m,T,seed", [(3, 2, 6, 11), (4, 2, 5, 12)])
def test_ffbs_f64_matches_dense_joint_gaussian(n, m, T, seed):
    a = cm.random_stable_lgssm(n, m, seed=seed, bias=True)
    ys = cm.simulate_batch(a, 1, T, seed=seed)[0].astype(F64)
    kf = kalman_f64(a, ys, a["m0"], a["P0"])
    x0, M = affine_map(kf["m"], kf["P"], kf["pm"], kf["pP"], a["A"])
    dm, dP, dC = dense_posterior(a, ys, a["m0"], a["P0"])
    cov, cross = joint_blocks(M, T, n)
    assert np.max(np.abs(x0.reshape(T, n) - dm)) <= 1e-9 * max(1.0, np.max(np.abs(dm)))
    assert np.max(np.abs(cov - dP)) <= 1e-9 * max(1.0, np.max(np.abs(dP)))
    assert np.max(np.abs(cross - dC)) <= 1e-9 * max(1.0, np.max(np.abs(dC)))


# ---- 2: rank-deficient conditional covariances -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cv", "rs4dq2"])
def test_ffbs_f64_rank_deficient(name):
    if name == "cv":
        a, T = cm.cv_model_arrays(), 64
    else:
        a, T = cm.random_stable_lgssm(4, 2, seed=4, dq=2), 32
    n = 4
    ys = cm.simulate_batch(a, 1, T, seed=6)[0].astype(F64)
    kf = kalman_f64(a, ys, a["m0"], a["P0"])
    xi = np.random.default_rng(2).normal(size=(3, T, n))
    piv = []
    x = ffbs_f64(kf["m"], kf["P"], kf["pm"], kf["pP"], a["A"], xi, pivots=piv)
    assert np.all(np.isfinite(x))
    assert len(piv) == T
    assert all(k for _, k in piv[0])                       # P_{T-1} has full rank
    for rec in piv[1:]:                                     # G Q G^T has rank 2: Sigma_t = P_t - G_t P- G_t^T has rank 2
        assert sum(not k for _, k in rec) == 2, rec
    s = T // 2 + 3
    cut = lambda lo, hi: [kf[k][lo:hi] for k in ("m", "P", "pm", "pP")]
    late = ffbs_f64(*cut(s, T), a["A"], xi[:, s:])
    early = ffbs_f64(*cut(0, s), a["A"], xi[:, :s], carry=late[:, 0])
    np.testing.assert_allclose(np.concatenate([early, late], axis=1), x, rtol=1e-12, atol=1e-12)


# ---- 3: argument checks that need no device -----------------------------------------------------------------------------
def _posterior(B, K, T, n, pred=True):
    import torch
    import bayesianfiltering_amd as bfa
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return bfa.PosteriorGaussianSumFiltered(None, z(B, K, T, n), z(B, K, T, n, n), z(B, K, T, n) if pred else None,
                                            z(B, K, T, n, n) if pred else None)


def test_python_validation_without_device():
    import torch
    import bayesianfiltering_amd as bfa
    nl = bfa.nonlinearities
    lin = cm.product_params(cm.cv_model_arrays())
    key = bfa.PRNGKey(0)
    with pytest.raises(ValueError, match="one component"):
        bfa.posterior_sample(lin, _posterior(2, 3, 8, 4), 2, key=key)
    post = _posterior(2, 1, 8, 4)
    with pytest.raises(ValueError, match="exactly one"):
        bfa.posterior_sample(lin, post, 2)
    with pytest.raises(ValueError, match="exactly one"):
        bfa.posterior_sample(lin, post, 2, key=key, noise=torch.zeros(2, 2, 8, 4))
    with pytest.raises(ValueError, match="noise has shape"):
        bfa.posterior_sample(lin, post, 2, noise=torch.zeros(2, 3, 8, 4))
    with pytest.raises(ValueError, match="noise has shape"):
        bfa.posterior_sample(lin, post, 2, noise=torch.zeros(2, 8, 4))
    ext = bfa.ParamsNLSSM(np.zeros(3, np.float32), np.eye(3, dtype=np.float32), nl.lorenz63(), np.zeros(3, np.float32),
                          np.eye(3, dtype=np.float32), nl.linear_emission(np.eye(3, dtype=np.float32)),
                          np.zeros(3, np.float32), np.eye(3, dtype=np.float32))
    with pytest.raises(ValueError, match="predicted"):
        bfa.posterior_sample(ext, _posterior(2, 1, 8, 3, pred=False), 2, key=key)
    with pytest.raises(ValueError, match="state dimension"):
        bfa.posterior_sample(lin, _posterior(2, 1, 8, 3), 2, key=key)
    with pytest.raises(ValueError, match="num_samples"):
        bfa.posterior_sample(lin, post, 0, key=key)
    assert bfa.SamplerCarry._fields == ("states",)


def _c_args(n=3):
    from bayesianfiltering_amd import _lib
    keep = [np.zeros(64, np.float32) for _ in range(6)]
    fd = _lib.bf_out_desc()
    for name, buf in zip(("means", "covs", "pred_means", "pred_covs"), keep):
        s = getattr(fd, name)
        s.ptr, s.sB, s.sT, s.sE = buf.ctypes.data, 1, 1, 1
    sd = _lib.bf_sample_desc()
    sd.samples.ptr, sd.noise.ptr = keep[4].ctypes.data, keep[5].ctypes.data
    eye = np.eye(n, dtype=np.float32).ravel()
    theta = np.array([10.0, 28.0, 2.667, 0.01], np.float32)
    mdl = _lib.bf_model()
    mdl.dyn_id, mdl.emi_id, mdl.n, mdl.dq, mdl.m, mdl.dr = 2, 0, n, n, n, n
    mdl.dyn_theta, mdl.n_dyn_theta = theta.ctypes.data_as(_lib._FP), 4
    mdl.Q, mdl.R = eye.ctypes.data_as(_lib._FP), eye.ctypes.data_as(_lib._FP)
    lg = _lib.bf_lgssm()
    lg.n, lg.dq, lg.m, lg.dr = n, n, n, n
    lg.A, lg.Q, lg.Q_steps = eye.ctypes.data_as(_lib._FP), eye.ctypes.data_as(_lib._FP), 1
    return fd, sd, mdl, lg, (keep, eye, theta)


def test_c_entry_points_reject_before_launch():
    from bayesianfiltering_amd import _lib
    lib = _lib.load()
    fd, sd, mdl, lg, keep = _c_args()
    ud = _lib.bf_cstream()
    ext = lambda m_, f_, S_, c_, s_: lib.bf_effbs_sample_f32(C.byref(m_), C.byref(ud), C.byref(f_), 4, 8, S_, c_, C.byref(s_), None)
    lin = lambda f_, S_, c_, s_: lib.bf_ffbs_sample_f32(C.byref(lg), C.byref(f_), 4, 8, S_, c_, C.byref(s_), None)
    # functions given as source, legacy-class streams
    user = _lib.bf_model.from_buffer_copy(mdl)
    user.dyn_id = _lib.BF_FN_USER
    assert ext(user, fd, 2, None, sd) == _lib.BF_EUNSUPPORTED
    leg = _lib.bf_model.from_buffer_copy(mdl)
    leg.flags = _lib.BF_MODEL_PREDICT_FIRST
    assert ext(leg, fd, 2, None, sd) == _lib.BF_EUNSUPPORTED
    # NULL samples; neither noise nor keys; S <= 0; the extended entry point without predictions; one prediction only
    nos = _lib.bf_sample_desc.from_buffer_copy(sd)
    nos.samples.ptr = None
    non = _lib.bf_sample_desc.from_buffer_copy(sd)
    non.noise.ptr = None
    nopred = _lib.bf_out_desc.from_buffer_copy(fd)
    nopred.pred_means.ptr = nopred.pred_covs.ptr = None
    one = _lib.bf_out_desc.from_buffer_copy(fd)
    one.pred_means.ptr = None
    for call in (lambda *a_: ext(mdl, *a_), lin):
        assert call(fd, 2, None, nos) == _lib.BF_EINVAL and b"samples" in lib.bf_last_error()
        assert call(fd, 2, None, non) == _lib.BF_EINVAL and b"keys" in lib.bf_last_error()
        assert call(fd, 0, None, sd) == _lib.BF_EINVAL
        assert call(fd, -3, None, sd) == _lib.BF_EINVAL
        assert call(one, 2, None, sd) == _lib.BF_EINVAL
    assert ext(mdl, nopred, 2, None, sd) == _lib.BF_EINVAL and b"predicted" in lib.bf_last_error()
    # bf_sample_carry holds one array per direction, so x_in without x_out (or the reverse) is a valid carry and there is
    # no pair rule to break as in bf_smooth_carry; a half-filled carry does not mask the checks that follow it
    half = _lib.bf_sample_carry()
    half.x_in = keep[0][0].ctypes.data
    assert lin(fd, 0, C.byref(half), sd) == _lib.BF_EINVAL and b"samples S" in lib.bf_last_error()
    assert lin(fd, 2, C.byref(half), nos) == _lib.BF_EINVAL and b"samples stream" in lib.bf_last_error()
    # the linear entry point: no A; Q_steps neither 1 nor T on the recompute path
    noa = _lib.bf_lgssm.from_buffer_copy(lg)
    noa.A = None
    assert lib.bf_ffbs_sample_f32(C.byref(noa), C.byref(fd), 4, 8, 2, None, C.byref(sd), None) == _lib.BF_EINVAL
    lg.Q_steps = 5
    assert lin(nopred, 2, None, sd) == _lib.BF_EINVAL and b"Q_steps" in lib.bf_last_error()
    lg.Q_steps = 1
    assert lib.bf_set_call_option(b"ffbs_spl", 3) == _lib.BF_EINVAL
    assert lib.bf_set_option(b"ffbs_spl", 0) == _lib.BF_OK


def test_sampler_abi_check():
    from bayesianfiltering_amd import _lib
    lib = _lib.load()
    assert lib.bf_sampler_abi_check(C.sizeof(_lib.bf_sample_desc), C.sizeof(_lib.bf_sample_carry)) == _lib.BF_OK
    assert lib.bf_sampler_abi_check(0, 0) == _lib.BF_OK
    assert lib.bf_sampler_abi_check(C.sizeof(_lib.bf_stream), 0) == _lib.BF_EINVAL
    assert b"bf_sample_desc" in lib.bf_last_error()
    assert lib.bf_sampler_abi_check(0, 3 * 8) == _lib.BF_EINVAL
    assert b"bf_sample_carry" in lib.bf_last_error()
    assert C.sizeof(_lib.bf_sample_desc) == 2 * C.sizeof(_lib.bf_stream) + 8 and C.sizeof(_lib.bf_sample_carry) == 16


def test_sampler_struct_sizes_agree_with_a_c_compiler(tmp_path):
    import subprocess
    import os
    from bayesianfiltering_amd import _lib
    names = ["bf_sample_desc", "bf_sample_carry"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "bayesfilt.h"\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    sizes = dict(line.split() for line in out.strip().splitlines())
    for n in names:
        assert int(sizes[n]) == C.sizeof(getattr(_lib, n)), (n, sizes[n])
