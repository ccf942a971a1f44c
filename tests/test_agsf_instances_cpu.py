"""Without a GPU: the case table of the every-instance sweep of the augmented Gaussian-sum register kernels tests itself.

(a) Every referenced trajectory of every case of tests/agsf_instance_cases.py is a comparison that means something, by the
    conditions and thresholds of test_agsf_generic_cpu.py: the oracle's run is finite; on average at least 1.5 distinct leaves are
    drawn per step; multiplying the leaf weights alternately by 1 +- 1e-4 (both sign patterns) and renormalising leaves every drawn
    index unchanged (jr.choice for variants 0 and 1, utils.optimal_resampling with the filter's own key for variant 2); with
    optimal resampling the oracle's emitted weights are not all 1 / N0 (what test_agsf_instances_gpu.py asserts of them), the
    best leaf's log-likelihood stays within 600 in magnitude (beyond it float32 cannot give the weights to the asserted 3e-4), and
    the draw must also survive one sign pattern per bit of the leaf index: it goes through the SORTED order of the weights, and
    the alternating pattern moves two leaves of equal parity together, so it cannot see a near-tie between them.  A case
    that misses a condition is replaced in the case table (another seed, a smaller spread, a shorter T), never excused.
(b) The set of (node kind, instance, waves per trajectory) the cases reach EQUALS the compiled set, read from the BF_CASE rows of
    csrc/agsf_scan.hip and csrc/agsf_ukf.hip and the BF_GEOM rows of csrc/agsf_scan.hpp: an instance or a geometry added later
    without a case fails here.
These tests pass with or without the kernels: they test the test."""
import re

import numpy as np
import pytest

from oracle import gaussfilt_oracle as go
from tests import agsf_instance_cases as ic
from tests import common as cm

F32 = np.float32


def _trajectories():
    return [(name, b) for name, c in ic.CASES.items() for b in c["refs"]]


@pytest.mark.parametrize("name,b", _trajectories())
def test_case_is_a_meaningful_comparison(name, b):
    c = ic.CASES[name]
    N0, M = c["nc"][0], int(np.prod(c["nc"]))
    post, aux = ic.reference(name, b)
    for k in ("weights", "means", "covariances"):
        assert np.isfinite(getattr(post, k)).all(), k
    if c["variant"] == 2:      # the point of the variant: the GPU test demands unequal reference weights, the case has to have them
        assert not np.allclose(post.weights, 1.0 / N0)
        # ... within rtol 3e-4.  A leaf's weight is exp(ll - max ll) times its parent's, and a float32 ll of magnitude L is known to
        # L * 1.2e-7 (one ulp) at best, a few ulps after the quadratic form: that absolute error IS the weight's relative error.
        # 4 ulps within 3e-4 is L <= 600.  (The linear (4, 2) row at (100, 2, 2) had its best leaf at ll = -3896, one ulp 2.4e-4;
        # the device drew the oracle's leaves and missed the oracle's weights by 2.4e-3.)
        L = float(np.max(np.abs(aux["best_loglik"])))
        print(f"  {name}[{b}]: largest |log-likelihood| of a step's best leaf {L:.0f}")
        assert L <= 600.0, L
    pre = aux["pre_weights"]
    assert pre.shape == (c["T"], M) and np.isfinite(pre).all()
    idx = ic.oracle_leaf_indices(name, b)
    assert idx.shape == (c["T"], N0)
    assert np.array_equal(idx, aux["leaf_indices"])     # the recomputed draw is the oracle's own
    distinct = float(np.mean([np.unique(row).size for row in idx]))
    print(f"  {name}[{b}]: {distinct:.2f} distinct drawn leaves per step of {N0}")
    assert distinct >= 1.5, distinct
    for pattern in ic.margin_patterns(name):
        for t in range(c["T"]):
            wp = (pre[t].astype(np.float64) * (1.0 + 1e-4 * pattern)).astype(F32)
            wp = (wp / go.sum_f32(wp)).astype(F32)
            assert np.array_equal(ic.draw(name, wp), idx[t]), (t, "the draw at this step hangs on the last digits of the weights")


def compiled_kernels():
    """{(node kind, instance, waves per trajectory)} as the sources compile them: every instance with one wave per trajectory, the
    instances up to the state dimension of launch_agsf_nodes' ``if constexpr`` also with the multi-wave geometries."""
    hpp = cm.read_csrc("agsf_scan.hpp")
    body = hpp[hpp.index("#define BF_GEOM("):hpp.index("#undef BF_GEOM")]
    head, bound, tail = re.split(r"if constexpr \(N <= (\d+)\)", body, maxsplit=1)
    geom = lambda s: [int(x) for x in re.findall(r"^\s*(?:if \(L\.nw == \d+\) )?BF_GEOM\((\d+)\);", s, re.M)]
    always, small = geom(head), geom(tail)
    assert always == [1] and small == [2, 4, 8, 16], (always, small)
    out = set()
    for kind, src in (("ekf", "agsf_scan.hip"), ("ukf", "agsf_ukf.hip")):
        rows = cm.instance_rows(src)
        assert rows and len(set(rows)) == len(rows), src
        for inst in rows:
            out |= {(kind, inst, nw) for nw in always + (small if inst[0] <= int(bound) else [])}
    return out


# What the suite launched on this table before this sweep, read from the test files: (file, node kind, instance, trees, compared
# with the oracle).  The run-time builds (functions from source, linear models at uncompiled shapes) are not in the table.
# A snapshot, transcribed by hand when this sweep was added: it does not follow later changes of those files, and only the printed
# list and ``older <= compiled`` depend on it.
BF, BR = (4, 2), (4, 2, 2, 2)
EARLIER = [
    ("test_agsf_gpu.py", "ekf", BF, [(2, 2, 2), (3, 2, 2), (4, 4, 4), (5, 1, 3), (2, 5, 5), (4, 2, 3), (3, 2, 3), (5, 5, 5), (3, 5, 7), (70, 1, 1),
                                     (3, 10, 10), (100, 2, 2), (130, 2, 3)], True),
    ("test_agsf_gpu.py", "ekf", (8, 4), [(2, 2, 2)], True),
    ("test_agsf_gpu.py", "ukf", BR, [(2, 5, 5), (3, 2, 3), (20, 3, 3), (100, 2, 2)], True),
    ("test_reference_smoke_gpu.py", "ekf", (4, 1), [(5, 3, 2), (2, 5, 5), (5, 5, 5), (5, 2, 2)], True),
    ("test_reference_smoke_gpu.py", "ukf", (4, 2, 1, 1), [(2, 5, 5)], True),
    ("test_agsf_generic_gpu.py", "ekf", (8, 4), [(2, 2, 2)], True),
    ("test_agsf_generic_gpu.py", "ekf", BF, [(2, 2, 2)], True),
    ("test_user_model_gpu.py", "ekf", BF, [(4, 3, 2), (4, 2, 2)], True),
    ("test_user_model_gpu.py", "ukf", BR, [(4, 3, 2)], True),
    ("test_user_model_gpu.py", "ekf", BF, [(20, 3, 3)], False),      # against its run-time-built twin only
    ("test_user_model_gpu.py", "ukf", BR, [(20, 3, 3)], False),
    ("test_edge_cases_gpu.py", "ekf", BF, [(16, 8, 8)], False),      # shapes and finiteness only
]


def test_cases_reach_every_compiled_kernel():
    compiled = compiled_kernels()
    reached = {ic.kernel_of(c["row"], c["nc"]) for c in ic.CASES.values()}
    n_e, n_u = (sum(1 for k in compiled if k[0] == kind) for kind in ("ekf", "ukf"))
    print(f"  compiled: {n_e} extended + {n_u} unscented = {len(compiled)} kernels; reached by the cases: {len(reached & compiled)}")
    assert (n_e, n_u) == (36, 25)
    assert reached == compiled, (sorted(compiled - reached), sorted(reached - compiled))
    # the variants the issue sets per (row, tier)
    for rname, r in ic.ROWS.items():
        for tname in ic.TIERS:
            have = sorted(c["variant"] for c in ic.CASES.values() if c["row"] == rname and c["tier"] == tname)
            if r["inst"][0] > 4 and tname not in ic.ONE_WAVE:
                assert have == []
                continue
            want = [0] + ([2] if r["kind"] == "ekf" else []) + ([1] if tname == "G1a" else [])
            assert have == sorted(want), (rname, tname, have)
    # the launch shapes the tiers are there for
    assert [ic.geometry(t[0]) for t in ic.TIERS.values()] == [(16, 1), (64, 1), (128, 2), (256, 4), (512, 8), (1024, 16)]
    for nc, B, T, refs in ic.TIERS.values():
        MP, nw = ic.geometry(nc)
        if nw == 1:
            per = 256 // MP
            assert B > per and B % per != 0 and max(refs) == B - 1      # full workgroups and a ragged tail, its last trajectory referenced
    # what the older tests reached
    older = {(kind, inst, ic.geometry(nc)[1]) for _, kind, inst, trees, _ in EARLIER for nc in trees}
    older_oracle = {(kind, inst, ic.geometry(nc)[1]) for _, kind, inst, trees, oracle in EARLIER if oracle for nc in trees}
    assert older <= compiled
    print(f"  the older tests launch {len(older)} of {len(compiled)} kernels, {len(older_oracle)} of them against the oracle:")
    for k in sorted(older):
        print(f"    {k[0]} {k[1]} NW={k[2]}{'' if k in older_oracle else '   (not against the oracle)'}")
