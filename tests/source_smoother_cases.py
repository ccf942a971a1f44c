"""Models whose dynamics are given as source (or as a recorded Python function), with the analytic Jacobians the float64
oracles take: shared by tests/test_source_smoother_gpu.py and tests/test_source_sampler_gpu.py.  Every case is built and
filtered once (functools.lru_cache) and left unchanged."""
import functools
from typing import Any, NamedTuple

import numpy as np

F32 = np.float32
STREAMS = ("means", "covariances", "predicted_means", "predicted_covariances")

L63_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  const float s = th[0], r = th[1], b = th[2], dt = th[3];
  out[0] = dt * s * (x[1] - x[0]) + x[0] + q[0];
  out[1] = dt * (x[0] * r - x[1] - x[0] * x[2]) + x[1] + q[1];
  out[2] = dt * (x[0] * x[1] - b * x[2]) + x[2] + q[2];
}
"""
L63_THETA = [10.0, 28.0, 2.667, 0.01]

GROWTH_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  out[0] = x[0] / 2.0f + 25.0f * x[0] / (1.0f + x[0] * x[0]) + u + q[0];
}
"""

# Lorenz-96 ('matrix_power': (B x)_i = x_{i+1} - x_{i-2}) as a loop over the compile-time state dimension
L96_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  for (int i = 0; i < BF_N; ++i) {
    const T ax = x[(i + BF_N - 1) % BF_N];
    const T bx = x[(i + 1) % BF_N] - x[(i + 2 * BF_N - 2) % BF_N];
    out[i] = x[i] + th[3] * (th[0] * (ax * bx) - th[1] * x[i] + th[2]) + q[i];
  }
}
"""
L96_THETA = [1.0, 1.0, 8.0, 0.01]

# a dense linear map A x + G q with A | G in theta
LIN_SRC = """
template <class T> __device__ void dynamics(const T* x, const T* q, T u, const float* th, T* out) {
  for (int i = 0; i < BF_N; ++i) {
    T s = th[i * BF_N] * x[0];
    for (int k = 1; k < BF_N; ++k) s = s + th[i * BF_N + k] * x[k];
    for (int k = 0; k < BF_DQ; ++k) s = s + th[BF_N * BF_N + i * BF_DQ + k] * q[k];
    out[i] = s;
  }
}
"""

QUAD_EMI_SRC = """
template <class T> __device__ void emission(const T* x, const T* r, T u, const float* th, T* out) {
  out[0] = th[0] * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + r[0];
}
"""


class Case(NamedTuple):
    p: Any          # ParamsNLSSM with the dynamics from source
    post: Any       # the one-component gaussian_sum_filter posterior of p (FULL5 streams)
    jac: Any        # jac(b, means (T, n)) -> (T, n, n) analytic F_t, float32
    ys: Any
    u: Any
    B: int
    T: int
    n: int


def np_(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=F32), device="cuda")


def cut(post, lo, hi):
    return post._replace(**{k: getattr(post, k)[:, :, lo:hi].contiguous() for k in STREAMS})


def _simulate(f_host, m0, Q, R, H, B, T, u, seed=17):
    rng = np.random.default_rng(seed)
    n, dq = m0.size, Q.shape[0]
    x = m0 + rng.normal(size=(B, n)).astype(F32)
    xs = np.empty((B, T, n), F32)
    for t in range(T):
        ut = 0.0 if u is None else u[t]
        x = np.stack([f_host(x[b], rng.normal(size=dq).astype(F32) * np.sqrt(np.diag(Q)), ut) for b in range(B)])
        xs[:, t] = x
    hx = xs @ H.T
    return (hx + rng.normal(size=hx.shape) * np.sqrt(np.diag(R))).astype(F32)


def _filtered(p, ys, u, B, n, layout="reference"):
    import bayesianfiltering_amd as bfa
    return bfa.gaussian_sum_filter(p, ys, 1, inputs=u, initial_means=np.tile(p.initial_mean, (B, 1)).reshape(B, 1, n),
                                   layout=layout)


@functools.lru_cache(maxsize=None)
def case(kind, B, T, with_inputs=False):
    """kind: 'lorenz63' (n = 3), 'growth' (n = 1, inputs), 'lorenz96' (n = 10), 'pendulum' (n = 2, dq = 1, a recorded lambda)."""
    import bayesianfiltering_amd as bfa
    from oracle import models as om
    nl = bfa.nonlinearities
    u = None
    if kind == "lorenz63":
        n, reg, fo = 3, nl.lorenz63(), om.Lorenz63()
        f = nl.user_dynamics(L63_SRC, 3, theta=L63_THETA)
        m0, Q, R = np.array([1.0, 1.0, 1.0], F32), 1e-2 * np.eye(3, dtype=F32), 0.5 * np.eye(3, dtype=F32)
        if with_inputs:
            u = (0.5 * np.cos(1.2 * np.arange(T))).astype(F32)
    elif kind == "growth":
        n, reg, fo = 1, nl.growth(), om.Growth()
        f = nl.user_dynamics(GROWTH_SRC, 1)
        m0, Q, R = np.array([0.1], F32), np.eye(1, dtype=F32), np.eye(1, dtype=F32)
        u = (8 * np.cos(1.2 * np.arange(T))).astype(F32)
    elif kind == "lorenz96":
        n, reg, fo = 10, nl.lorenz96(10), om.Lorenz96(10)
        f = nl.user_dynamics(L96_SRC, 10, theta=L96_THETA)
        m0, Q, R = np.linspace(-1.0, 1.0, 10).astype(F32), 1e-2 * np.eye(10, dtype=F32), 0.5 * np.eye(10, dtype=F32)
    else:
        raise ValueError(kind)
    H = np.eye(n, dtype=F32)
    p = bfa.ParamsNLSSM(m0, np.eye(n, dtype=F32), f, np.zeros(n, F32), Q, nl.linear_emission(H), np.zeros(n, F32), R)
    ys = _simulate(reg, m0, Q, R, H, B, T, u)
    post = _filtered(p, ys, u, B, n)
    zq = np.zeros(n, F32)
    jac = lambda b, m: np.stack([fo.jac_x(m[t], zq, np.array([0.0 if u is None else u[t]], F32)) for t in range(T)])
    return Case(p, post, jac, ys, u, B, T, n)


G_PEND, DT_PEND = 9.81, 0.05


@functools.lru_cache(maxsize=None)
def pendulum_case(B=5, T=16):
    """The pendulum with scalar noise on the velocity row (dq = 1) and h = sin(x0), both plain Python functions."""
    import bayesianfiltering_amd as bfa
    f = lambda x, q, u: np.array([x[0] + DT_PEND * x[1], x[1] - DT_PEND * G_PEND * np.sin(x[0]) + q[0]])
    h = lambda x, r, u: np.array([np.sin(x[0])]) + r
    m0, Q, R = np.array([0.8, 0.0], F32), 1e-2 * np.eye(1, dtype=F32), 0.1 * np.eye(1, dtype=F32)
    p = bfa.ParamsNLSSM(m0, 0.1 * np.eye(2, dtype=F32), f, np.zeros(1, F32), Q, h, np.zeros(1, F32), R)
    rng = np.random.default_rng(23)
    x = m0 + 0.1 * rng.normal(size=(B, 2)).astype(F32)
    ys = np.empty((B, T, 1), F32)
    for t in range(T):
        x = np.stack([f(x[b], 0.1 * rng.normal(size=1), 0.0) for b in range(B)]).astype(F32)
        ys[:, t, 0] = np.sin(x[:, 0]) + np.sqrt(0.1) * rng.normal(size=B)
    post = _filtered(p, ys, None, B, 2)
    jac = lambda b, m: np.stack([np.array([[1.0, DT_PEND], [-DT_PEND * G_PEND * np.cos(np.float64(m[t, 0])), 1.0]])
                                 for t in range(T)])
    return Case(p, post, jac, ys, None, B, T, 2)
