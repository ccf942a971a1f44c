"""Yardsticks and cases of the parallel-in-time RTS smoother's tests (csrc/rts_pscan.hpp), float64 NumPy throughout.

* :func:`element`, :func:`combine`, :func:`apply_span` -- the smoothing element of one step, the associative combination of
  two spans and a span applied to a smoothed state, restated from the header.
* The cases are those of ``tests/parallel_kalman_cases.py`` (``pk.case``, ``pk.model`` names); the yardsticks are ``rts_f64`` and
  ``dense_posterior`` of ``tests/test_smoother_cpu.py``, re-exported here with its jitter-free ``kalman_f64``.
"""
import numpy as np

from tests import parallel_kalman_cases as pk
from tests.test_smoother_cpu import dense_posterior, kalman_f64, rts_f64  # noqa: F401  (the tests take them from here)

case, model = pk.case, pk.model
MODELS = ["1x1", "2x2", "3x1", "4x2", "4x4", "bias", "5x2", "6x3"]   # every built n; 'bias': noise biases, dq = 2 < n = 4


def _sym(X):
    return 0.5 * (X + X.T)


def terms(a):
    """A, Qb = G Q G^T and u = G q0 in float64 from the model's float32 arrays."""
    A, G, Q, q0 = (np.asarray(a[k], np.float64) for k in ("A", "G", "Q", "q0"))
    return A, G @ Q @ G.T, G @ q0


def element(a, m, P, pm=None, pP=None):
    """(E_t, g_t, L_t) of one step from its filtered m_t, P_t and the predictions m-_{t+1}, P-_{t+1} (None: recomputed)."""
    A, Qb, u = terms(a)
    m, P = np.asarray(m, np.float64), np.asarray(P, np.float64)
    if pm is None:
        pm, pP = A @ m + u, A @ P @ A.T + Qb
    pm, pP = np.asarray(pm, np.float64), np.asarray(pP, np.float64)
    L = np.linalg.cholesky(pP)
    G = np.linalg.solve(L.T, np.linalg.solve(L, A @ P)).T
    return G, m - G @ pm, _sym(P - G @ pP @ G.T)


def combine(si, sj):
    """The earlier span si followed by the later span sj."""
    Ei, gi, Li = si
    Ej, gj, Lj = sj
    return Ei @ Ej, Ei @ gj + gi, _sym(Ei @ Lj @ Ei.T + Li)


def apply_span(s, m, P):
    """The span s applied to the smoothed state (m, P) at the step after its last one."""
    E, g, L = s
    return E @ m + g, _sym(E @ P @ E.T + L)
