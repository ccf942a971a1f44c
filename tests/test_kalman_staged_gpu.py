"""Every compiled instance of the register Kalman kernel (csrc/kf_scan_group.hpp) on its LDS-staged emitter, the route any
batch of at least one wave takes: the observation blocks fetched one block ahead by LDS-DMA, the counted wait behind them, the
per-wave tiles that transpose time with their chunk-limited last flush, the LDS carve that depends on the enabled streams and
the split launch (whole waves staged, the ragged tail strided) all depend on the instance (n, m, lanes), on the horizon and on
the stream subset.  Cases, geometry and references: tests/kalman_staged_cases.py (validated without a GPU by
tests/test_kalman_staged_cpu.py).  B = 5 CPW + 3 everywhere: five whole waves staged, a tail of three strided.

Every option goes through ``options=`` on the call.  kf_emit_mode = 2 is refused by launch_nml when the layout is not eligible,
so a forced call that returns is the witness that the staged kernel ran; kf_emit_mode = 0 is the strided emitter, the same
arithmetic with one dword store per element.

  1. horizon sweep     every eligible T up to T_max: staged == strided bit for bit on the six outputs and the carry, and
                       == the first T steps of the T_max run (every remainder of T against each tile depth and against the
                       observation block; T = 1, 2, 3 at n = 4, 8; with T % 4 != 0 the scalar streams leave as dwords)
  2. float64           the T_max run against the batched float64 recursion: streams and carry 1e-5 norm-wise, log-likelihood
                       2e-5 (the tolerances of tests/test_kalman_gpu.py), weights exactly 1
  3. stream subsets    the twelve subsets of tests/test_output_contract_gpu.py, with and without the log-likelihood, staged,
                       at T_max and, where T_max % 4 != 0, also at the largest T % 4 == 0 (scalar-stream tiles carved)
  4. per-step tables   Q_t and / or R_t: staged == strided bit for bit and against float64, at T_max and the smallest T
  5. unaligned chunks  T_max cut at a step that is a multiple of neither YS nor a tile depth == the one-shot run bit for bit
                       (both chunks staged at n = 1, 2, 4, 8 and (6, 1), (6, 2); at n = 3, 5, 7 and (6, 3), (6, 4) no such cut
                       is eligible and the chunks leave strided: there the test checks the carry hand-off only)
"""
import functools

import numpy as np
import pytest
import torch

from tests import common as cm
from tests import kalman_staged_cases as ks
from tests.test_output_contract_gpu import TWELVE

pytestmark = pytest.mark.gpu
FULL5, STREAMS = ks.FULL5, ks.STREAMS
IDS = [ks.case_id(i) for i in ks.INSTANCES]
STAGED, STRIDED = 2, 0


class Case:
    """One instance with its inputs on the device (uploaded once) and its runs."""

    def __init__(self, inst):
        self.inst, self.g = inst, ks.geometry(inst)
        self.n, self.m, self.lanes_opt = inst
        a = dict(ks.model(inst))
        ys, m0s, P0s = ks.data(inst)
        self.pp = cm.product_params(a)
        self.y = torch.as_tensor(ys.copy(), device="cuda")      # (the cases are read-only arrays)
        self.m0 = torch.as_tensor(m0s.copy(), device="cuda")
        self.P0 = torch.as_tensor(P0s.copy(), device="cuda")

    def params(self, variant, T):
        if variant == "const":
            return self.pp
        Qt, Rt = ks.variant_tables(self.inst, variant)
        kw = {}
        if Qt is not None:
            kw["dynamics_noise_covariance"] = Qt[:T]
        if Rt is not None:
            kw["emission_noise_covariance"] = Rt[:T]
        return self.pp._replace(**kw)

    def run(self, T, mode, fields=FULL5, loglik=True, variant="const", t0=0, carry=None):
        """(posterior, log-likelihood or None, carry) of steps t0 .. t0 + T - 1 from the priors (or ``carry``)."""
        import bayesianfiltering_amd as bfa
        opts = {"kf_lanes": self.lanes_opt}
        if mode is not None:
            opts["kf_emit_mode"] = mode
        start = dict(carry=carry) if carry is not None else dict(initial_means=self.m0, initial_covariances=self.P0)
        res = bfa.kalman_filter(self.params(variant, T), self.y[:, t0:t0 + T], fields=fields, return_loglik=loglik,
                                return_carry=True, options=opts, **start)
        assert len(res) == 2 + bool(loglik)      # the log-likelihood is returned exactly when it was asked for
        return res[0], (res[1] if loglik else None), res[-1]

    @functools.cached_property
    def full(self):
        """The staged T_max run with everything enabled, never modified."""
        return self.run(self.g["t_max"], STAGED)


@functools.lru_cache(maxsize=None)
def case(inst):
    return Case(inst)


def _assert_same_bits(got, want, what, T=None):
    """Posterior, log-likelihood and (T = None) carry of two runs bit for bit; with T, ``want`` is cut to its first T steps."""
    for k in FULL5:
        w = getattr(want[0], k)
        assert torch.equal(getattr(got[0], k), w if T is None else w[:, :, :T]), (what, k)
    assert torch.equal(got[1], want[1] if T is None else want[1][:, :, :T]), (what, "loglik")
    if T is None:
        for x, y_, nm in zip(got[2], want[2], ("weights", "means", "covariances")):
            assert torch.equal(x, y_), (what, "carry." + nm)


def _errors_vs_float64(c, res, variant, T):
    """{stream / loglik / carry_*: norm-wise error of a run of T steps against the float64 reference's first T steps}."""
    ref = ks.reference_f64(c.inst, variant)
    post, ll, carry = res
    e = {k: cm.rel_err(getattr(post, k).cpu().numpy(), ref[k][:, :, :T]) for k in STREAMS}
    e["loglik"] = cm.rel_err(ll.cpu().numpy(), ref["loglik"][:, :, :T])
    e["carry_means"] = cm.rel_err(carry.means.cpu().numpy(), ref["predicted_means"][:, :, T - 1])
    e["carry_covariances"] = cm.rel_err(carry.covariances.cpu().numpy(), ref["predicted_covariances"][:, :, T - 1])
    return e


def _assert_meets_float64(c, res, variant, T, what):
    e = _errors_vs_float64(c, res, variant, T)
    print(f"  {ks.case_id(c.inst)} {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    cm.record(f"kalman_staged_vs_float64[{ks.case_id(c.inst)}-{what}]", **e)
    for k, v in e.items():
        assert v < (ks.TOL_LL if k == "loglik" else ks.TOL), (what, k, v)
    assert bool((res[0].weights == 1.0).all()) and bool((res[2].weights == 1.0).all()), what
    shape = (c.g["B"], 1, T)
    assert tuple(res[0].means.shape) == shape + (c.n,) and tuple(res[0].covariances.shape) == shape + (c.n, c.n)


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_horizon_sweep(inst):
    c = case(inst)
    full = c.full
    for T in c.g["horizons"]:
        staged = c.run(T, STAGED)
        _assert_same_bits(staged, c.run(T, STRIDED), f"T={T} staged vs strided")
        _assert_same_bits(staged, full, f"T={T} vs the first steps of T_max={c.g['t_max']}", T=T)
        # the carry is the last prediction
        assert torch.equal(staged[2].means, staged[0].predicted_means[:, :, -1]), T
        assert torch.equal(staged[2].covariances, staged[0].predicted_covariances[:, :, -1]), T


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_float64(inst):
    c = case(inst)
    _assert_meets_float64(c, c.full, "const", c.g["t_max"], "const")


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_stream_subsets(inst):
    """The LDS carve (a disabled stream aliases the observation tile) and the counted wait behind the observation DMA
    (launch_nml: nP / nM / nW / wscalar / vm_younger) depend on the subset: stores change, arithmetic does not."""
    c = case(inst)
    for T in c.g["subset_horizons"]:        # T_max, and a T % 4 == 0 with the scalar streams' tiles carved where T_max has none
        assert T >= 3 * c.g["ys"]
        full = c.full if T == c.g["t_max"] else c.run(T, STAGED)
        for fields in TWELVE:
            for want_ll in (True, False):
                post, ll, carry = c.run(T, STAGED, fields=fields, loglik=want_ll)
                for k in FULL5:
                    if k not in fields:
                        assert getattr(post, k) is None, (T, fields, want_ll, k)
                    else:
                        assert torch.equal(getattr(post, k), getattr(full[0], k)), (T, fields, want_ll, k)
                assert (ll is None) == (not want_ll)
                if want_ll:
                    assert torch.equal(ll, full[1]), (T, fields, "loglik")
                for x, y_, nm in zip(carry, full[2], ("weights", "means", "covariances")):
                    assert torch.equal(x, y_), (T, fields, want_ll, "carry." + nm)


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_per_step_tables(inst):
    """kf_scan_group_kernel<..., EMIT_STAGED, TV = true>: step t predicts with Q_t and updates with R_t."""
    c = case(inst)
    const = c.full
    for variant in ks.TABLE_VARIANTS:
        for T in (c.g["t_max"], c.g["t_min"]):
            staged = c.run(T, STAGED, variant=variant)
            _assert_same_bits(staged, c.run(T, STRIDED, variant=variant), f"{variant} T={T} staged vs strided")
            _assert_meets_float64(c, staged, variant, T, f"{variant}-T{T}")
        assert not torch.equal(staged[0].predicted_covariances, const[0].predicted_covariances[:, :, :T]), variant


@pytest.mark.parametrize("inst", ks.INSTANCES, ids=IDS)
def test_unaligned_chunks(inst):
    c = case(inst)
    T, cut = c.g["t_max"], c.g["cut"]
    whole = c.run(T, None)
    _assert_same_bits(whole, c.full, "default emit mode vs staged")
    first = c.run(cut, None)
    second = c.run(T - cut, None, t0=cut, carry=first[2])
    for k in FULL5:
        parts = torch.cat([getattr(first[0], k), getattr(second[0], k)], dim=2)
        assert torch.equal(parts, getattr(whole[0], k)), (cut, k)
    assert torch.equal(torch.cat([first[1], second[1]], dim=2), whole[1]), (cut, "loglik")
    for x, y_, nm in zip(second[2], whole[2], ("weights", "means", "covariances")):
        assert torch.equal(x, y_), (cut, "carry." + nm)
