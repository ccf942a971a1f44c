"""Yardsticks and cases of the parallel-in-time posterior sampler's tests (csrc/ffbs_pscan.hpp), float64 NumPy throughout.

* :func:`element`, :func:`combine`, :func:`apply_span` -- the sampling element of one step (shared E, one g per noise row), the
  associative combination of two spans and a span applied to the samples after it, restated from the header.
* The cases are those of ``tests/parallel_kalman_cases.py`` (``pk.case``, ``pk.model`` names); the yardsticks are ``ffbs_f64`` and
  ``psdchol_f64`` of ``tests/test_sampler_cpu.py`` and ``kalman_f64`` and ``dense_posterior`` of ``tests/test_smoother_cpu.py``,
  re-exported here.
"""
import numpy as np

from tests import parallel_kalman_cases as pk
from tests.parallel_smoother_cases import MODELS, terms  # noqa: F401  (the tests take them from here)
from tests.test_sampler_cpu import ffbs_f64, joint_blocks, psdchol_f64  # noqa: F401
from tests.test_smoother_cpu import dense_posterior, kalman_f64  # noqa: F401

case, model = pk.case, pk.model


def element(a, m, P, xi, pm=None, pP=None):
    """(E_t, g_t) of one step from its filtered m_t, P_t, the noise rows xi (S, n) and the predictions m-_{t+1}, P-_{t+1}
    (None: recomputed): E_t = G_t (n, n), g_t = m_t - G_t m-_{t+1} + L_t xi_{s,t} (S, n), with G_t and L_t as ffbs_factor
    forms them."""
    A, Qb, u = terms(a)
    m, P, xi = np.asarray(m, np.float64), np.asarray(P, np.float64), np.asarray(xi, np.float64)
    if pm is None:
        pm, pP = A @ m + u, A @ P @ A.T + Qb
    pm, pP = np.asarray(pm, np.float64), np.asarray(pP, np.float64)
    Lp = np.linalg.cholesky(pP)
    W = np.linalg.solve(Lp, A @ P)
    G = np.linalg.solve(Lp.T, W).T
    Sig = np.tril(P) + np.tril(P, -1).T - W.T @ W
    L = psdchol_f64(Sig, np.diag(P))
    return G, m - G @ pm + xi @ L.T


def combine(si, sj):
    """The earlier span si followed by the later span sj."""
    Ei, gi = si
    Ej, gj = sj
    return Ei @ Ej, gj @ Ei.T + gi


def apply_span(s, x):
    """The span s applied to the samples x (S, n) at the step after its last one."""
    E, g = s
    return x @ E.T + g
