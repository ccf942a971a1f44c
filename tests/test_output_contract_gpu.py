"""The output contract of the five-stream filters on every kernel family: WHERE the kernels write, and what happens when
a caller asks for less than everything.

(a) every subset of ``fields`` (with and without the log-likelihood) returns None for what was not asked and, for what was,
    the bits of the full run -- stream pointers are run-time arguments that change stores, never arithmetic;
(b) guard bands: each stream is a view into a larger buffer filled with one NaN bit pattern, passed through ``out=``; the
    views equal a plain run bit for bit and every element outside them still holds the pattern (whole buffers as int32);
(c) the same observations contiguous, time-major and as a slice of a wider buffer give the same bits;
(d) layout='batch_inner' on the matrix-core Gaussian-sum routes equals the reference layout bit for bit;
(e) an ``out=`` tensor that is not float32 on the call's device is refused before anything is launched.

Routes (csrc/bf_api.hip: bf_kalman_filter_f32, bf_gsf_ekf_f32; csrc/ugsf_scan.hip: launch_ugsf_ukf):
  kf-reg       n <= 8: launch_kf_group -> kf_scan_group_kernel (state in registers).  kf_emit_mode 2 = LDS-staged dwordx4
               rows with the ragged batch tail on a second, strided launch; 0 = strided stores; batch_inner = strided.
               kf_lanes 1 and 4 exist for (4, 2) only (csrc/kf_group_*.hip) -- elsewhere that option would fall through to
               the run-time-dimension kernel, which kf-generic covers -- so they run on the cv model.
  kf-bf32      (12, 10): 9 <= n <= 32 with m > 8 -> launch_kf_bf32, one wave per trajectory on padded 32 x 32 tiles
  kf-mfma      (33, 7) padded and (64, 32) native -> launch_kf_mfma, four waves per trajectory
  kf-generic   (9, 2): n < 16 and m <= 8 miss the matrix-core test, launch_kf_group has no n = 9 -> launch_kf_generic
  gsf-reg      n <= 8: launch_gsf_ekf -> gsf_scan_kernel.  Lorenz-63 (n = 3) has no staged tiles (rows of 9 floats do not
               divide the 32-float tile row: GsfCfg::STAGED_OK is false, kf_emit_mode = 2 is refused), so it runs in modes -1
               and 0 and the staged emitter runs on the cv model with K = 4 and B = 32 (it takes whole waves only).
  gsf-multi    linear (16, 8), K = 3 -> launch_kf_bf32 with MULTI
  gsf-chain    Lorenz-96 + pick_even, n = 16, K = 3 -> launch_kf_bf32 with extended chains (dyn_kind = 1)
  gsf-generic  Lorenz-96, n = 12 (m = 6 <= 8, n < 16) -> launch_gsf_ekf has no instance -> launch_gsf_generic
  ugsf-reg     Lorenz-63 + quadratic, K = 4 -> launch_ugsf<3, 3, 1, 1>
  ugsf-generic Lorenz-96, n = 12 -> launch_ugsf_generic (state in LDS)
Where an option can force the run-time-dimension kernel, one test per family proves the default route is another kernel
(the two round differently).

Tolerances against the oracle are the families' own: streams 1e-5 norm-wise (gsf-reg also 3e-5 element-wise, as
tests/test_gsf_gpu.py), weights 2e-5 absolute, log-likelihood 2e-5 (kf-reg, gsf-multi, gsf-chain, gsf-generic), 1e-5
(gsf-reg), 5e-5 (kf-bf32, kf-mfma, kf-generic, ugsf-*).

Different-arithmetic exceptions to (a): none."""
import contextlib
import functools
import time

import numpy as np
import pytest
import torch

from oracle import gaussfilt_oracle as go, models as om, threefry as otf, c_oracle
from tests import common as cm
from tests.test_stream_desc_cpu import assert_guards_intact, event_shapes, guarded, sentinel_buffer

pytestmark = pytest.mark.gpu
F32 = np.float32
FULL5 = ("weights", "means", "covariances", "predicted_means", "predicted_covariances")
STREAMS = FULL5[1:]
UP = (1.0, 0.0, 0.0)

ALL_SUBSETS = [tuple(f for i, f in enumerate(FULL5) if mask >> i & 1) for mask in range(32)]
TWELVE = [()] + [(f,) for f in FULL5] + [tuple(g for g in FULL5 if g != f) for f in FULL5] + [FULL5]


def _bfa():
    import bayesianfiltering_amd as bfa
    return bfa


@contextlib.contextmanager
def _options(**kv):
    """bf_set_option for the duration of the block (as tests/test_kalman_gpu.py: _run); defaults restored whatever happens."""
    from bayesianfiltering_amd import _lib
    defaults = {"kf_emit_mode": -1, "kf_lanes": 0, "force_generic": 0, "ugsf_force_generic": 0}
    lib = _lib.require_gpu()
    try:
        for k, v in kv.items():
            _lib.check(lib.bf_set_option(k.encode(), int(v)))
        yield
    finally:
        for k in kv:
            lib.bf_set_option(k.encode(), defaults[k])


class Case:
    """One model with its data, its oracle (computed once, never modified) and its family's tolerances."""

    def __init__(self, kind, pp, ys, init, K, n, oracle, ll_tol, inputs=None, elem_tol=None, force=None):
        self.kind, self.pp, self.ys, self.init, self.K, self.n, self.inputs = kind, pp, ys, init, K, n, inputs
        self.B, self.T, self.m = ys.shape
        self._oracle, self.ll_tol, self.elem_tol, self.force = oracle, ll_tol, elem_tol, force

    @functools.cached_property
    def y_dev(self):
        return torch.as_tensor(self.ys, device="cuda")

    @functools.cached_property
    def ref(self):
        r = self._oracle()
        for v in r.values():
            v.setflags(write=False)
        return r

    def run(self, emissions=None, inputs="same", **kw):
        bfa = _bfa()
        y = self.y_dev if emissions is None else emissions
        u = self.inputs if isinstance(inputs, str) else inputs
        if self.kind == "kf":
            return bfa.kalman_filter(self.pp, y, initial_means=self.init, **kw)
        if self.kind == "gsf":
            return bfa.gaussian_sum_filter(self.pp, y, self.K, 1, u, initial_means=self.init, **kw)
        return bfa.unscented_gaussian_sum_filter(self.pp, bfa.ParamsUKF(*UP), y, self.K, 1, u, initial_means=self.init, **kw)

    def check_oracle(self, post, ll):
        ref = self.ref
        for k in STREAMS:
            got = getattr(post, k).cpu().numpy()
            assert got.shape == ref[k].shape, k
            e = cm.both_err(got, ref[k], k)
            print(f"  {k}: rel {e[0]:.2e} elem {e[1]:.2e}")
            assert e[0] < 1e-5, (k, e)
            if self.elem_tol is not None:
                assert e[1] < self.elem_tol, (k, e)
        ew = float(np.max(np.abs(post.weights.cpu().numpy() - ref["weights"])))
        el = cm.rel_err(ll.cpu().numpy(), ref["loglik"])
        print(f"  weights: abs {ew:.2e}   loglik: rel {el:.2e}")
        assert ew < 2e-5, ew
        assert el < self.ll_tol, el


def _stack(posts_lls):
    out = {k: np.stack([getattr(p, k) for p, _ in posts_lls]) for k in FULL5}
    out["loglik"] = np.stack([ll for _, ll in posts_lls])
    return out


def _kf_case(a, B, T, seed, oracle, ll_tol, force="force_generic"):
    ys = cm.simulate_batch(a, B, T, seed=seed)
    n = a["A"].shape[0]
    init = (np.tile(a["m0"], (B, 1)) + 0.1 * np.random.default_rng(seed).normal(size=(B, n))).astype(F32)
    orc = (lambda: cm.oracle_kalman_batch(a, ys, init)) if oracle == "numpy" else (lambda: dict(c_oracle.kalman_filter(a, ys, init)))
    return Case("kf", cm.product_params(a), ys, init, 1, n, orc, ll_tol, force=force)


def _gsf_case(po, pp, B, T, K, n, init, ll_tol, sampler_inputs=None, inputs=None, kind="gsf", **kw):
    u2 = None if sampler_inputs is None else sampler_inputs.reshape(T, 1)
    ys = np.stack([go.sample_ssm(po, otf.PRNGKey(10 + b), T, u2)[1] for b in range(B)]).astype(F32)
    if kind == "gsf":
        orc = lambda: _stack([go.gaussian_sum_filter(po, ys[b], K, initial_means=init[b], inputs=u2, return_ll=True) for b in range(B)])
    else:
        orc = lambda: _stack([go.unscented_gaussian_sum_filter(po, go.ParamsUKF(*UP), ys[b], K, initial_means=init[b], inputs=u2,
                                                               return_ll=True) for b in range(B)])
    return Case(kind, pp, ys, init, K, n, orc, ll_tol, inputs=inputs, **kw)


def _l63():
    nl = _bfa().nonlinearities
    m0 = np.array([0.0, 1.0, 1.05], F32)
    args = (m0, np.eye(3, dtype=F32))
    noise = (np.zeros(3, F32), 0.1 * np.eye(3, dtype=F32)), (np.zeros(1, F32), np.eye(1, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Lorenz63(), *noise[0], om.Quadratic(3, 0.05), *noise[1])
    pp = _bfa().ParamsNLSSM(*args, nl.lorenz63(), *noise[0], nl.quadratic(3, 0.05), *noise[1])
    return po, pp, m0


def _l96(n, m0):
    nl = _bfa().nonlinearities
    m = n // 2
    args = (m0, np.eye(n, dtype=F32))
    noise = (np.zeros(n, F32), 1e-2 * np.eye(n, dtype=F32)), (np.zeros(m, F32), 1e-1 * np.eye(m, dtype=F32))
    po = go.ParamsNLSSM(*args, om.Lorenz96(n), *noise[0], om.PickEven(n), *noise[1])
    pp = _bfa().ParamsNLSSM(*args, nl.lorenz96(n), *noise[0], nl.pick_even(n), *noise[1])
    return po, pp


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    # kf-reg.  B = 130: two full waves at one lane per trajectory plus a tail of 2 for the strided launch.  T = 72: rows
    # 16-byte aligned, not a multiple of the staging depth; (3, 1) at T = 40: masked tiles (vm_younger forced to 0); cv at
    # T = 50: the scalar streams leave the staged path (wscalar) while means and covariances stay on it
    if name in ("kf-cv-T72", "kf-cv-T50"):
        return _kf_case(cm.cv_model_arrays(), 130, int(name[-2:]), 1, "numpy", 2e-5)
    if name == "kf-3x1-T40":
        return _kf_case(cm.random_stable_lgssm(3, 1, seed=31, bias=True), 130, 40, 3, "numpy", 2e-5)
    if name == "kf-8x4-T72":
        return _kf_case(cm.random_stable_lgssm(8, 4, seed=84, bias=True), 130, 72, 8, "numpy", 2e-5)
    if name == "kf-bf32-12x10":
        return _kf_case(cm.random_stable_lgssm(12, 10, seed=130, dq=9, dr=10, bias=True), 5, 14, 2, "c", 5e-5)
    if name == "kf-mfma-33x7":
        return _kf_case(cm.random_stable_lgssm(33, 7, seed=370, dq=30, dr=6, bias=True), 5, 12, 4, "c", 5e-5)
    if name == "kf-mfma-64x32":
        return _kf_case(cm.random_stable_lgssm(64, 32, seed=645, bias=True), 5, 12, 5, "c", 5e-5)
    if name == "kf-generic-9x2":
        return _kf_case(cm.random_stable_lgssm(9, 2, seed=92, dq=7, dr=2, bias=True), 5, 13, 6, "c", 5e-5, force=None)
    if name == "gsf-l63":       # ragged: B = 5 trajectories of K = 4 chains do not fill a wave
        po, pp, m0 = _l63()
        B, T, K = 5, 16, 4
        return _gsf_case(po, pp, B, T, K, 3, (m0 + 0.5 * rng.normal(size=(B, K, 3))).astype(F32), 1e-5, elem_tol=3e-5, force="force_generic")
    if name == "gsf-cv-staged":  # tests/test_gsf_gpu.py: test_staged_partial_rows_and_single_trajectory_waves
        a = cm.cv_model_arrays()
        B, T, K = 32, 20, 4
        return _gsf_case(cm.oracle_params(a), cm.product_params(a), B, T, K, 4, rng.normal(size=(B, K, 4)).astype(F32), 1e-5,
                         elem_tol=3e-5, force="force_generic")
    if name == "gsf-bot-inputs":  # tests/test_gsf_gpu.py: test_bot_with_inputs_nonpow2_components -- the model that reads its inputs
        nl = _bfa().nonlinearities
        B, T, K = 3, 24, 5
        mu0, S0 = np.array([2.0, 0.3, 3.0, -0.2], F32), np.diag([0.1, 0.005, 0.1, 0.01]).astype(F32)
        Q, R = 1e-3 * np.eye(2, dtype=F32), np.diag([1e-3, 1e-2]).astype(F32)
        u = np.array([1] * 8 + [0] * 8 + [2] * 8, F32)
        po = go.ParamsNLSSM(mu0, S0, om.ManeuverBOT(), np.zeros(2, F32), Q, om.BearingRange(), np.zeros(2, F32), R)
        pp = _bfa().ParamsNLSSM(mu0, S0, nl.maneuver_bot(), np.zeros(2, F32), Q, nl.bearing_range(), np.zeros(2, F32), R)
        return _gsf_case(po, pp, B, T, K, 4, (mu0 + 0.05 * rng.normal(size=(B, K, 4))).astype(F32), 1e-5, sampler_inputs=u, inputs=u,
                         elem_tol=3e-5)
    if name in ("gsf-multi-16x8", "gsf-multi-64x32"):
        n, m, K = (16, 8, 3) if name.endswith("16x8") else (64, 32, 2)
        a = cm.random_stable_lgssm(n, m, seed=n + m + K, dq=n - 2, dr=m, bias=True)
        B, T = 5, 14
        return _gsf_case(cm.oracle_params(a), cm.product_params(a), B, T, K, n, (a["m0"] + 0.5 * rng.normal(size=(B, K, n))).astype(F32),
                         2e-5, force="force_generic")
    if name in ("gsf-chain-l96-16", "gsf-generic-l96-12"):
        n, K, B, T = int(name[-2:]), 3, 5, 14
        m0 = 8 * np.ones(n, F32)
        po, pp = _l96(n, m0)
        return _gsf_case(po, pp, B, T, K, n, (m0 + 0.5 * rng.normal(size=(B, K, n))).astype(F32), 2e-5,
                         force="force_generic" if n == 16 else None)
    if name == "ugsf-l63":
        po, pp, m0 = _l63()
        B, T, K = 5, 20, 4
        return _gsf_case(po, pp, B, T, K, 3, (m0 + rng.normal(size=(B, K, 3))).astype(F32), 5e-5, kind="ugsf", force="ugsf_force_generic")
    if name == "ugsf-generic-l96-12":
        n, K, B, T = 12, 3, 5, 12
        po, pp = _l96(n, np.zeros(n, F32))
        return _gsf_case(po, pp, B, T, K, n, rng.normal(size=(B, K, n)).astype(F32), 5e-5, kind="ugsf")
    raise KeyError(name)


# (case, options): every way a family is run.  kf-reg: three emit modes x the lane counts compiled for the model
KF_REG = [(c, layout, mode, lanes)
          for c, lane_set in (("kf-cv-T72", (0, 1, 4)), ("kf-cv-T50", (0, 1, 4)), ("kf-3x1-T40", (0,)), ("kf-8x4-T72", (0,)))
          for layout, mode in (("reference", 2), ("reference", 0), ("batch_inner", -1)) for lanes in lane_set]
GSF_REG = [("gsf-l63", "reference", -1), ("gsf-l63", "reference", 0), ("gsf-l63", "batch_inner", -1),
           ("gsf-cv-staged", "reference", 2), ("gsf-cv-staged", "reference", 0)]
OTHERS = ["kf-bf32-12x10", "kf-mfma-33x7", "kf-mfma-64x32", "kf-generic-9x2", "gsf-multi-16x8", "gsf-chain-l96-16",
          "gsf-generic-l96-12", "ugsf-l63", "ugsf-generic-l96-12"]
# one representative run per case for (b) and (c): the staged emitter for the register kernels
DEFAULT_RUNS = [("kf-cv-T72", 2), ("kf-cv-T50", 2), ("kf-3x1-T40", 2), ("kf-8x4-T72", 2), ("gsf-l63", -1), ("gsf-cv-staged", 2)] + \
               [(c, -1) for c in OTHERS]


def _ids(rows):
    return ["-".join(str(x) for x in (r if isinstance(r, tuple) else (r,))) for r in rows]


# ---------------------------------------------------------------------------------------------------------------------
# (a) every subset of streams
def _subsets_equal_the_full_run(c, subsets, layout="reference", **opts):
    t0 = time.perf_counter()
    with _options(**opts):
        full, ll, carry = c.run(fields=FULL5, layout=layout, return_loglik=True, return_carry=True)
        c.check_oracle(full, ll)
        for fields in subsets:
            for want_ll in (True, False):
                res = c.run(fields=fields, layout=layout, return_loglik=want_ll, return_carry=True)
                post, cr = res[0], res[-1]
                for k in FULL5:
                    if k not in fields:
                        assert getattr(post, k) is None, (fields, want_ll, k)
                    else:
                        assert torch.equal(getattr(post, k), getattr(full, k)), (fields, want_ll, k)
                if want_ll:
                    assert torch.equal(res[1], ll), (fields, "loglik")
                for x, y_, nm in zip(cr, carry, ("weights", "means", "covariances")):
                    assert torch.equal(x, y_), (fields, want_ll, "carry." + nm)
    torch.cuda.synchronize()
    print(f"  {2 * len(subsets) + 1} runs in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name,layout,mode,lanes", KF_REG, ids=_ids(KF_REG))
def test_kf_reg_every_subset_of_streams(name, layout, mode, lanes):
    """All 32 subsets x {with, without} the log-likelihood: the LDS carve of the staged emitter, the aliasing of a disabled
    stream onto the observation tile and the counted wait behind the LDS-DMA observation block all depend on the subset
    (csrc/kf_scan_group.hpp: launch_nml, nP / nM / nW / wscalar / vm_younger)."""
    _subsets_equal_the_full_run(case(name), ALL_SUBSETS, layout, kf_emit_mode=mode, kf_lanes=lanes)


@pytest.mark.parametrize("name,layout,mode", GSF_REG, ids=_ids(GSF_REG))
def test_gsf_reg_every_subset_of_streams(name, layout, mode):
    """All 32 subsets on the register EKF bank (csrc/gsf_scan.hpp: launch_gsf, the same carve with K chains per trajectory)."""
    _subsets_equal_the_full_run(case(name), ALL_SUBSETS, layout, kf_emit_mode=mode)


@pytest.mark.parametrize("name", OTHERS)
@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
def test_twelve_subsets_of_streams(name, layout):
    """The empty set, the five singletons, the five leave-one-out sets and the full set."""
    _subsets_equal_the_full_run(case(name), TWELVE, layout)


def test_staged_emitter_is_refused_where_it_has_no_tiles():
    """Lorenz-63 on the register EKF bank: rows of 9 floats do not divide the tile row, kf_emit_mode = 2 must say so."""
    from bayesianfiltering_amd import _lib
    c = case("gsf-l63")
    with _options(kf_emit_mode=2), pytest.raises(_lib.BayesFiltError) as e:
        c.run()
    assert e.value.code == _lib.BF_EINVAL


# (the cv model is left out: its A, G and H hold only 0, 0.5 and 1, and the register and run-time-dimension kernels then round
# alike -- their outputs are equal bit for bit, which proves nothing either way; kf-3x1 / kf-8x4 and gsf-l63 stand for the families)
ROUTED = [n for n, _ in DEFAULT_RUNS if n not in ("kf-cv-T72", "kf-cv-T50", "gsf-cv-staged")]


@pytest.mark.parametrize("name", ROUTED)
def test_default_route_is_not_the_run_time_dimension_kernel(name):
    from bayesianfiltering_amd import _lib
    c = case(name)
    fast = c.run()
    if c.force is None:     # the generic families: forcing changes nothing, the default IS that kernel
        with _options(force_generic=1, ugsf_force_generic=1):
            forced = c.run()
        assert all(torch.equal(getattr(fast, k), getattr(forced, k)) for k in FULL5)
        return
    if name == "ugsf-l63":  # the LDS kernel has no Lorenz-63 (csrc/ugsf_generic.hip): it refuses the model, so the default run was not it
        with _options(ugsf_force_generic=1), pytest.raises(_lib.BayesFiltError) as e:
            c.run()
        assert e.value.code == _lib.BF_EUNSUPPORTED
        return
    with _options(**{c.force: 1}):
        forced = c.run()
    assert not torch.equal(fast.covariances, forced.covariances)        # (the two kernels round differently)


# ---------------------------------------------------------------------------------------------------------------------
# (b) guard bands
def _guarded_out(c, geometry, fields):
    bufs, views, carves = {}, {}, {}
    for k in fields:
        numel, carve = guarded(geometry, c.B, c.K, c.T, event_shapes(c.n)[k])
        bufs[k] = sentinel_buffer(numel, "cuda")
        views[k], carves[k] = carve(bufs[k]), carve
    return bufs, views, carves, _bfa().PosteriorGaussianSumFiltered(**views)


def _guard_case(c, geometry, fields=FULL5, **opts):
    plain = c.run(fields=fields)
    bufs, views, carves, out = _guarded_out(c, geometry, fields)
    with _options(**opts):
        post = c.run(fields=fields, out=out)
    for k in FULL5:
        if k not in fields:
            assert getattr(post, k) is None
            continue
        assert getattr(post, k).data_ptr() == views[k].data_ptr(), k
        assert torch.equal(views[k], getattr(plain, k)), (geometry, k)
    assert_guards_intact(bufs, carves)


GUARD_RUNS = [(n, g, m if g == "slice" else -1) for n, m in DEFAULT_RUNS for g in ("slice", "misaligned", "foreign", "batch_inner")]


@pytest.mark.parametrize("name,geometry,mode", GUARD_RUNS, ids=_ids(GUARD_RUNS))
def test_nothing_outside_the_given_views_is_written(name, geometry, mode):
    """slice: the contiguous reference slice keeps the staged emitter eligible (forced with kf_emit_mode = 2 where the family
    has one: dwordx4 rows masked at the end of T, the ragged batch tail on the strided launch) -- the guard trajectories on
    both sides must survive.  misaligned: the same slice 4 bytes off, the launcher has to fall back to strided stores
    (stream_is_reference tests ptr % 16).  foreign: padded batch, components, time and event.  batch_inner with guards."""
    c = case(name)
    opts = {"kf_emit_mode": mode} if mode != -1 else {}
    _guard_case(c, geometry, **opts)
    if geometry == "slice" and mode == 2:    # and with some streams off: a disabled stream's tile is aliased, not carved
        _guard_case(c, geometry, fields=("means", "predicted_covariances"), **opts)
        _guard_case(c, geometry, fields=("weights", "covariances"), **opts)


@pytest.mark.parametrize("lanes", [1, 4])
def test_staged_slice_at_every_lane_count_of_the_cv_model(lanes):
    _guard_case(case("kf-cv-T72"), "slice", kf_emit_mode=2, kf_lanes=lanes)
    _guard_case(case("kf-cv-T50"), "slice", kf_emit_mode=2, kf_lanes=lanes)


@pytest.mark.parametrize("name", ["kf-cv-T72", "kf-3x1-T40", "kf-8x4-T72", "gsf-cv-staged"])
def test_forced_staged_emitter_refuses_misaligned_streams_and_writes_nothing(name):
    from bayesianfiltering_amd import _lib
    c = case(name)
    for fields in [FULL5] + [(f,) for f in FULL5]:      # every enabled stream is tested for alignment
        bufs, views, carves, out = _guarded_out(c, "misaligned", fields)
        with _options(kf_emit_mode=2), pytest.raises(_lib.BayesFiltError) as e:
            c.run(fields=fields, out=out)
        assert e.value.code == _lib.BF_EINVAL, fields
        torch.cuda.synchronize()
        assert_guards_intact({k: b for k, b in bufs.items()}, carves, written=False)


# ---------------------------------------------------------------------------------------------------------------------
# (c) strided emissions (and inputs)
def _emission_forms(c):
    B, T, m = c.B, c.T, c.m
    nan = float("nan")
    tm = torch.full((T, B, m), nan, device="cuda").permute(1, 0, 2)
    tm.copy_(c.y_dev)
    wide = torch.full((B, T + 5, 2 * m), nan, device="cuda")[:, 2:T + 2, ::2]
    wide.copy_(c.y_dev)
    cont = c.y_dev.contiguous()
    assert cont.stride() == (T * m, m, 1)
    assert tm.stride() == (m, B * m, 1) and wide.stride() == ((T + 5) * 2 * m, 2 * m, 2)
    assert len({cont.stride(), tm.stride(), wide.stride()}) == 3
    return cont, tm, wide


@pytest.mark.parametrize("name,mode", DEFAULT_RUNS, ids=_ids(DEFAULT_RUNS))
def test_strided_emissions_give_the_same_bits(name, mode):
    """Contiguous, time-major and a slice of a wider buffer (element stride 2, padded T).  kf-reg runs staged: the LDS-DMA
    addresses of the observation blocks are built from y.sT and y.sE."""
    c = case(name)
    opts = {"kf_emit_mode": mode} if mode != -1 else {}
    res = []
    with _options(**opts):
        for y in _emission_forms(c):
            res.append(c.run(emissions=y, return_loglik=True, return_carry=True))
    c.check_oracle(res[0][0], res[0][1])
    for other in res[1:]:
        for k in FULL5:
            assert torch.equal(getattr(other[0], k), getattr(res[0][0], k)), k
        assert torch.equal(other[1], res[0][1])
        for x, y_ in zip(other[2], res[0][2]):
            assert torch.equal(x, y_)


@pytest.mark.parametrize("name", ["gsf-bot-inputs", "gsf-l63", "gsf-multi-16x8", "gsf-chain-l96-16", "gsf-generic-l96-12"])
def test_inputs_as_a_slice_of_a_longer_time_axis(name):
    """inputs (B, T, d) cut out of a longer time axis (the binding fixes the element stride at 1).  Only the manoeuvring-target
    model reads its inputs: there the run must also differ from one without them."""
    c = case(name)
    B, T = c.B, c.T
    u = np.zeros(T, F32) if c.inputs is None else c.inputs
    cont = torch.as_tensor(np.broadcast_to(u.reshape(1, T, 1), (B, T, 1)).copy(), device="cuda")
    longer = torch.full((B, T + 7, 1), float("nan"), device="cuda")[:, 4:T + 4]
    longer.copy_(cont)
    assert cont.stride() != longer.stride() and longer.stride(0) == T + 7
    a = c.run(inputs=cont, return_loglik=True)
    b = c.run(inputs=longer, return_loglik=True)
    c.check_oracle(a[0], a[1])
    for k in FULL5:
        assert torch.equal(getattr(a[0], k), getattr(b[0], k)), k
    assert torch.equal(a[1], b[1])
    if c.inputs is not None:
        assert not torch.equal(c.run(inputs=None).means, a[0].means)


# ---------------------------------------------------------------------------------------------------------------------
# (d) batch_inner on the matrix-core Gaussian-sum routes
@pytest.mark.parametrize("name", ["gsf-multi-16x8", "gsf-chain-l96-16", "gsf-multi-64x32"])
def test_batch_inner_on_the_matrix_core_gaussian_sum_routes(name):
    c = case(name)
    ref, ll = c.run(return_loglik=True)
    c.check_oracle(ref, ll)
    bi, llb = c.run(layout="batch_inner", return_loglik=True)
    for k in FULL5:
        v = getattr(bi, k)
        assert v.stride(0) == 1 and tuple(v.shape) == tuple(getattr(ref, k).shape), k
        assert torch.equal(v, getattr(ref, k)), k
    assert torch.equal(llb, ll)
    with _options(force_generic=1):
        forced = c.run()
    assert not torch.equal(forced.covariances, ref.covariances)          # (another kernel did run: the two round differently)


# ---------------------------------------------------------------------------------------------------------------------
# (e) out= must be float32 on the call's device
@pytest.mark.parametrize("name", ["kf-cv-T72", "gsf-l63", "ugsf-l63"])
def test_out_of_another_dtype_or_device_is_refused_before_any_launch(name):
    c = case(name)
    shape = (c.B, c.K, c.T, c.n)
    bfa = _bfa()
    f64 = torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"out\.means.*float32.*float64"):
        c.run(out=bfa.PosteriorGaussianSumFiltered(means=f64))
    torch.cuda.synchronize()
    assert bool((f64 == 7.0).all())          # nothing was launched into it
    host = torch.full(shape, 7.0, dtype=torch.float32)
    with pytest.raises(ValueError, match=r"out\.means.*cpu"):
        c.run(out=bfa.PosteriorGaussianSumFiltered(means=host))
    assert bool((host == 7.0).all())
    with pytest.raises(ValueError, match=r"out\.predicted_covariances"):
        c.run(out=bfa.PosteriorGaussianSumFiltered(predicted_covariances=torch.zeros((c.B, c.K, c.T, c.n, c.n), dtype=torch.float16, device="cuda")))
    # and a good one is still taken
    good = torch.empty(shape, dtype=torch.float32, device="cuda")
    post = c.run(out=bfa.PosteriorGaussianSumFiltered(means=good))
    assert post.means.data_ptr() == good.data_ptr() and torch.equal(good, c.run().means)
