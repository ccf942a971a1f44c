"""Without a GPU: every configuration that test_agsf_generic_gpu.py runs on the device is a comparison that means something.

The device kernel (csrc/agsf_generic_device.hpp) is compared with the NumPy oracle by the leaves it draws at every step -- which
must be EQUAL -- and by the moments of the drawn leaves.  That is only a fair demand, and only a sharp one, if
  * the oracle's own run is finite;
  * the tree is not degenerate: on average at least 1.5 distinct leaves are drawn per step (one surviving leaf per step would
    make every index comparison trivially true);
  * the draw is decided with room to spare: multiplying the oracle's leaf weights alternately by 1 +- 1e-4 (both sign patterns)
    and renormalising leaves every drawn index unchanged, so a kernel whose weights agree with the oracle's to rounding (1e-6)
    must draw the same leaves.  jr.choice for variants 0 and 1, utils.optimal_resampling for variant 2.
A configuration that fails a condition is to be replaced by another seed, not excused.  These tests pass with or without the
kernel: they test the test."""
import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import agsf_generic_cases as ac

F32 = np.float32


def _trajectories():
    return [(name, b) for name, c in ac.CASES.items() for b in range(c["B"])]


@pytest.mark.parametrize("name,b", _trajectories())
def test_configuration_is_a_meaningful_comparison(name, b):
    c = ac.CASES[name]
    N0, M = c["nc"][0], int(np.prod(c["nc"]))
    post, aux = ac.reference(name, b)
    for k in ("weights", "means", "covariances"):
        assert np.isfinite(getattr(post, k)).all(), k
    pre = aux["pre_weights"]
    assert pre.shape == (c["T"], M) and np.isfinite(pre).all()
    idx = ac.oracle_leaf_indices(name, b)
    assert idx.shape == (c["T"], N0)
    assert np.array_equal(idx, aux["leaf_indices"])     # the recomputed draw is the oracle's own
    distinct = float(np.mean([np.unique(row).size for row in idx]))
    print(f"  {name}[{b}]: {distinct:.2f} distinct drawn leaves per step of {N0}")
    assert distinct >= 1.5, distinct
    signs = np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
    for pattern in (signs, -signs):
        for t in range(c["T"]):
            wp = (pre[t].astype(np.float64) * (1.0 + 1e-4 * pattern)).astype(F32)
            wp = (wp / go.sum_f32(wp)).astype(F32)
            assert np.array_equal(ac.draw(name, wp), idx[t]), (t, "the draw at this step hangs on the last digits of the weights")


def test_cases_cover_what_the_issue_lists():
    """The issue's table: tree, length, variant and node kind per case; and the paths they are there for."""
    want = {"a-v0": (12, (3, 2, 2), 12, 0, False), "a-v1": (12, (3, 2, 2), 12, 1, False), "a-v2": (12, (3, 2, 2), 12, 2, False),
            "a-v0-unscented": (12, (3, 2, 2), 12, 0, True), "b-v1": (20, (2, 2, 3), 8, 1, False), "c-v0": (9, (4, 3, 6), 8, 0, False),
            "d-v2": (12, (5, 5, 5), 6, 2, False)}
    for name, (n, nc, T, variant, unscented) in want.items():
        c = ac.CASES[name]
        assert (c["n"], c["nc"], c["T"], c["variant"], c["uparams"] is not None) == (n, nc, T, variant, unscented), name
    assert ac.CASES["b-v1"]["n"] > 16
    assert ac.CASES["e-v1-n40"]["n"] > 36 and ac.CASES["e-v1-n20-unscented"]["n"] > 16     # the four-wave geometry by dimension
    assert np.prod(ac.CASES["c-v0"]["nc"]) > 64             # more leaves than a wave
    assert np.prod(ac.CASES["d-v2"]["nc"]) == 125           # the reference's own test tree
