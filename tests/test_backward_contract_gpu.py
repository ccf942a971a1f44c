"""What the passes that run AFTER a filter read and write, per kernel route: the smoother (csrc/rts_smoother.hpp, .hip), the
posterior sampler (csrc/ffbs_sampler.hpp, .hip) and the particle smoother (csrc/pf_sampler.hpp, .hip).  The counterpart of
tests/test_output_contract_gpu.py, whose guard-band builders (tests/test_stream_desc_cpu.py) it shares.

(a) parity with the family's float64 oracle on the GPU's own filtered streams, at the family's tolerance: ``_check`` of
    tests/test_smoother_gpu.py (1e-5 norm-wise) and tests/test_sampler_gpu.py (1e-5 of the sample scale), the teacher-forced
    parity of tests/test_particle_sampler_gpu.py (tau measured, at most 1e-4).  No tolerance is introduced here;
(b) guard bands on everything a call WRITES: smoothed means / covariances / cross-covariances and samples go in through
    ``out=`` as views of buffers filled with one NaN bit pattern, in the geometries slice, misaligned, foreign, batch_inner (and
    mixed across the smoother's three streams); each view equals a plain run bit for bit and everything outside still holds the
    pattern.  Without a carry the cross-covariances are the (B, 1, T-1, n, n) view the call returns, so entry T-1 is guard;
(c) guard bands on everything a call READS: the four filtered streams and the noise as views of such buffers (the history of
    the particle smoother time-major and as a [:, :N] slice of N + 8 particle slots whose extras hold the pattern).  One element
    read outside a view brings a NaN in and breaks the bit-for-bit comparison; the buffers are unchanged afterwards;
(d) the carries equal the first time slot of the chunk's own output, and two chunks writing into one guarded full-length
    buffer through the carry reproduce the one-shot run bit for bit;
(e) an ``out`` that is not float32, not on the device, or not exactly the shape the call returns is refused before any launch.

Routes (the dispatch was read in csrc/backward_host.hpp: backward_dispatch, csrc/rts_smoother.hip: RtsProduct::regs / generic,
csrc/ffbs_sampler.hip: FfbsProduct::regs / generic, csrc/pf_sampler.hip: launch_pfs_n / launch_pfs_inst):
  rts-staged      n <= 4, B >= 64, every stream in the contiguous reference layout with 16-byte aligned rows ->
                  rts_reg_kernel<N, RTS_STAGED> on the whole waves, <N, RTS_STRIDED> on the B % 64 tail.  ``rts_load_mode = 2``
                  forces it and is refused (-1) where it cannot serve, so a forced run that returns DID take it.
                  rts-cv: (4, 2), B = 130 (two waves + 2), T = 23 (TC = 2: a last chunk of one step, where without a carry no
                  cross-covariance leaves the tile).  rts-n3: rows of 9 floats, B = 70, T = 24 -- T * 9 must be a multiple of 4
                  for the rows to be 16-byte aligned, so with TC = 4 no partial chunk exists at n = 3; for the same reason a
                  contiguous (T-1)-step cross-covariance buffer is never aligned at n = 3 and is refused by the forced option,
                  while the T-1 leading steps of a T-step buffer (what the call itself returns) are served.
  rts-reg-strided rts-n3 with ``rts_load_mode = 0``; rts-n7 (RtsStage<7>::OK is false); any geometry but slice
  rts-generic     n = 12 > 8 -> rts_generic_kernel, kinds RTS_LIN (rts-g12), RTS_LIN_RECOMPUTE (rts-g12-recompute: no predicted
                  streams) and RTS_LIN_RECOMPUTE with a (T, dq, dq) table (rts-g12-qtable)
  eks-reg         Lorenz-63, B = 66, T = 24 -> rts_reg_kernel<3, ., RTS_EXT>: staged by default (one wave and a tail of 2, the
                  alignment rule of rts-n3), and with ``rts_load_mode`` 0 and 2
  eks-generic     Lorenz-96, n = 12, even-state emission (tests/test_backward_contract_cpu.py: L96) -> rts_generic_kernel, RTS_EXT
  ffbs-reg        n = 4, S = 5 -> ffbs_reg_kernel<4, SPL> for ffbs_spl = 1, 2, 4, 8 (0 picks 8 at S = 5: three idle slots per
                  lane); n = 7, S = 3 -> SPL = 4 (one idle slot)
  ffbs-generic    n = 12, S = 5: one sample block in LDS; n = 24, S = 100: 2048 / 24 = 85 samples per block, two blocks, x_{t+1}
                  read back through the strides of ``out``
  effbs-reg / effbs-generic   the two extended cases above, S = 5
  pfs-backward    N = 100, n = 3 -> pfs_backward_kernel<3, 16, 16>; N = 1100, n = 2 -> <2, 64, 8> (N > 1024); Lorenz-96 n = 12,
                  N = 64 -> <12, 16, 16> with the model read from memory (N > 8 in launch_pfs_inst)
  pfs-genealogy   N = 100, n = 3 -> pfs_trace_kernel
(The register and the run-time-dimension smoothers round alike at n = 3 -- their outputs are equal bit for bit -- so comparing a
default run with a ``force_generic`` one proves nothing about the route: (a) only holds the forced run to the same oracle.)

Measured on an MI355X (``cm.record``; the ``force_generic`` runs gave the same figures to the last digit).  Smoother, means /
covariances / cross-covariances against 1e-5: rts-cv 7.6e-8 / 1.9e-6 / 2.2e-6, rts-n3 1.2e-7 / 2.8e-7 / 3.2e-7, rts-n7 3.2e-7 /
8.8e-7 / 7.3e-7, rts-g12 3.0e-7 / 9.1e-7 / 8.7e-7, rts-g12-recompute 3.1e-7 / 9.7e-7 / 8.0e-7, rts-g12-qtable 3.5e-7 / 7.5e-7 /
9.7e-7, eks-l63 9.4e-8 / 1.5e-6 / 8.1e-7, eks-l96 1.0e-7 / 3.0e-7 / 3.7e-7.  Sampler against 1e-5: ffbs-n4 4.8e-7, ffbs-n7 6.2e-7,
ffbs-g12 5.2e-7, ffbs-g24 2.6e-6, effbs-l63 8.8e-8, effbs-l96 2.5e-7.  Particle smoother, tau against 1e-4: pfs-16row 8.3e-6,
pfs-64row 1.7e-5, pfs-n12 2.0e-5."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import threefry as otf
from tests import common as cm
from tests import test_backward_contract_cpu as bc
from tests import test_particle_sampler_cpu as ps
from tests import test_particle_sampler_gpu as pg
from tests import test_sampler_gpu as fg
from tests import test_smoother_gpu as sg
from tests.test_stream_desc_cpu import SENTINEL_BITS, assert_guards_intact, guarded, sentinel_buffer

pytestmark = pytest.mark.gpu
F32 = np.float32
GEOMETRIES = ("slice", "misaligned", "foreign", "batch_inner")
STREAMS = fg.STREAMS
SMOOTHED = ("smoothed_means", "smoothed_covariances", "smoothed_cross_covariances")


def _bfa():
    import bayesianfiltering_amd as bfa
    return bfa


class Guarded:
    """One (B, K, T, *ev) stream as a view of a sentinel buffer.  ``keep``: only the first ``keep`` steps belong to the view
    (the T-1 cross-covariances inside a T-step buffer).  ``fill``: a tensor copied into the view."""

    def __init__(self, geometry, shape, keep=None, fill=None):
        numel, carve = guarded(geometry, shape[0], shape[1], shape[2], tuple(shape[3:]))
        self.carve = carve if keep is None else (lambda flat: carve(flat)[:, :, :keep])
        self.buf = sentinel_buffer(numel, "cuda")
        self.view = self.carve(self.buf)
        if fill is not None:
            self.view.copy_(fill)

    def bits(self):
        return self.buf.view(torch.int32).clone()


def _intact(gs, written=True):
    torch.cuda.synchronize()
    assert_guards_intact({k: g.buf for k, g in gs.items()}, {k: g.carve for k, g in gs.items()}, written=written)


def _guarded_inputs(geometry, tensors):
    """name -> Guarded copy of every tensor that is not None, and the bits of the whole buffers."""
    gs = {k: Guarded(geometry, tuple(t.shape), fill=t) for k, t in tensors.items() if t is not None}
    return gs, {k: g.bits() for k, g in gs.items()}


def _unchanged(gs, before):
    torch.cuda.synchronize()
    for k, g in gs.items():
        assert torch.equal(g.buf.view(torch.int32), before[k]), f"input buffer {k} was modified"


def _cut(post, lo, hi):
    """Steps lo ... hi-1 of every stream, as views (their own strides)."""
    return post._replace(**{k: getattr(post, k)[:, :, lo:hi] for k in STREAMS if getattr(post, k) is not None})


# =====================================================================================================================
# the smoother
class SmCase:
    def __init__(self, name, p, post, ref, inputs=None, bare=False, modes=(-1,)):
        self.name, self.p, self.full_post, self._ref, self.inputs, self.modes = name, p, post, ref, inputs, modes
        self.post = post._replace(predicted_means=None, predicted_covariances=None) if bare else post
        self.B, _, self.T, self.n = (int(v) for v in post.means.shape)

    @functools.cached_property
    def ref(self):
        return self._ref()

    def run(self, post=None, mode=-1, **kw):
        opts = dict(kw.pop("options", None) or {})
        if mode != -1:
            opts["rts_load_mode"] = mode
        kw.setdefault("cross_covariances", True)
        kw.setdefault("return_carry", True)        # False: (posterior, None), the carry-out pointers are NULL in the kernel
        if not kw["return_carry"]:
            return _bfa().rts_smoother(self.p, self.post if post is None else post, inputs=self.inputs, options=opts or None, **kw), None
        return _bfa().rts_smoother(self.p, self.post if post is None else post, inputs=self.inputs,
                                   options=opts or None, **kw)

    @functools.cached_property
    def carry_in(self):
        """A smoothed state to start a chunk from: the one-shot run's own state at step 0."""
        return self.run()[1]

    def serves_staged(self, geometry, with_carry):
        """Can rts_load_mode = 2 serve out= views of this geometry (inputs contiguous)?  Only reference rows that start on 16
        bytes: slice, and of the cross-covariances without a carry either the leading T-1 steps of a T-step buffer (tail) or a
        (T-1)-step buffer whose rows of (T-1) n n floats are a multiple of 4 long."""
        if 2 not in self.modes or geometry not in ("slice", "tail"):
            return False
        return with_carry or geometry == "tail" or ((self.T - 1) * self.n * self.n) % 4 == 0


def _recomputed(a, post, q_table=None):
    """The posterior the recompute kernels see: the GPU's filtered streams and, for the oracle, their predictions formed in
    float64 (m- = A m + G q0, P- = A P A^T + G Q_t G^T)."""
    m, P = (sg._np(getattr(post, k)).astype(np.float64) for k in ("means", "covariances"))
    A, G, q0 = (np.asarray(a[k], np.float64) for k in ("A", "G", "q0"))
    Q = np.asarray(a["Q"] if q_table is None else q_table, np.float64)
    GQG = np.einsum("ij,...jk,lk->...il", G, Q, G)                      # (n, n) or (T, n, n)
    pm = m @ A.T + G @ q0
    pP = np.einsum("ij,bktjl,ml->bktim", A, P, A) + GQG
    return types.SimpleNamespace(means=post.means, covariances=post.covariances, predicted_means=torch.from_numpy(pm),
                                 predicted_covariances=torch.from_numpy(pP))


@functools.lru_cache(maxsize=None)
def sm_case(name):
    bfa = _bfa()
    if name in ("rts-cv", "rts-n3", "rts-n7", "rts-g12", "rts-g12-recompute"):
        n, m, B, T, seed = {"rts-cv": (4, 2, 130, 23, 3), "rts-n3": (3, 2, 70, 24, 33), "rts-n7": (7, 2, 70, 9, 47),
                            "rts-g12": (12, 2, 5, 12, 52), "rts-g12-recompute": (12, 2, 5, 12, 52)}[name]
        a = cm.cv_model_arrays() if name == "rts-cv" else cm.random_stable_lgssm(n, m, seed=seed, bias=True)
        _, post = sg._filter(a, B, T, seed=seed)
        bare = name.endswith("recompute")
        ref = (lambda: sg._oracle(_recomputed(a, post), a["A"])) if bare else (lambda: sg._oracle(post, a["A"]))
        modes = {"rts-cv": (-1, 2), "rts-n3": (-1, 0, 2)}.get(name, (-1,))
        return SmCase(name, cm.product_params(a), post, ref, bare=bare, modes=modes)
    if name == "rts-g12-qtable":
        n, B, T = 12, 5, 12
        a = cm.random_stable_lgssm(n, 2, seed=52, bias=True)
        rng = np.random.default_rng(1)
        table = np.stack([a["Q"] * F32(0.5 + rng.random()) for _ in range(T)]).astype(F32)
        ys = cm.simulate_batch(a, B, T, seed=52)
        p = cm.product_params(dict(a, Q=table))
        post = bfa.kalman_filter(p, ys, initial_means=np.tile(a["m0"], (B, 1)))
        return SmCase(name, p, post, lambda: sg._oracle(_recomputed(a, post, table), a["A"]), bare=True)
    if name == "eks-l63":
        p, fo, ys, u, B, T, n = sg._ext_case("lorenz63")
        post = bfa.gaussian_sum_filter(p, ys, 1, inputs=u, initial_means=np.tile(p.initial_mean, (B, 1)).reshape(B, 1, n))
        zq = np.zeros(n, F32)
        jac = lambda b, m: np.stack([fo.jac_x(m[t], zq, np.zeros(1, F32)) for t in range(T)])
        c = SmCase(name, p, post, lambda: sg._oracle(post, None, jac), modes=(-1, 0, 2))
        c.jac = jac
        return c
    if name == "eks-l96":
        ys, init = bc.l96_data()
        p = bc.l96_product_params()
        post = bfa.gaussian_sum_filter(p, ys, 1, initial_means=init)
        jac = lambda b, m: bc.l96_jacobians(m)
        c = SmCase(name, p, post, lambda: sg._oracle(post, None, jac))
        c.jac = jac
        return c
    raise KeyError(name)


SM_CASES = ["rts-cv", "rts-n3", "rts-n7", "rts-g12", "rts-g12-recompute", "rts-g12-qtable", "eks-l63", "eks-l96"]


def _equal_smoothed(got, want, label):
    for k in SMOOTHED:
        assert torch.equal(getattr(got[0], k), getattr(want[0], k)), (label, k)
    for x, y in zip(got[1], want[1]):
        assert torch.equal(x, y), (label, "carry")


def _carry_is_the_first_slot(res, label):
    sm, carry = res
    assert torch.equal(carry.means, sm.smoothed_means[:, 0, 0]), label
    assert torch.equal(carry.covariances, sm.smoothed_covariances[:, 0, 0]), label


@pytest.mark.parametrize("name", SM_CASES)
def test_smoother_parity_and_route(name):
    c = sm_case(name)
    assert tuple(c.post.means.shape) == (c.B, 1, c.T, c.n) and (c.post.predicted_means is None) == name.startswith("rts-g12-")
    plain = c.run()
    assert tuple(plain[0].smoothed_cross_covariances.shape) == (c.B, 1, c.T - 1, c.n, c.n)
    sg._check(plain[0], c.ref, name="_contract_" + name)
    _carry_is_the_first_slot(plain, name)
    for mode in c.modes[1:]:           # the forced data paths round alike
        _equal_smoothed(c.run(mode=mode), plain, (name, mode))
    forced = c.run(options={"force_generic": 1})      # n <= 8: the run-time-dimension kernel on the same streams
    sg._check(forced[0], c.ref, name="_contract_generic_" + name)


SM_GEOMETRIES = GEOMETRIES + ("tail", "mixed")


@pytest.mark.parametrize("with_carry", [False, True], ids=["nocarry", "carry"])
@pytest.mark.parametrize("geometry", SM_GEOMETRIES)
@pytest.mark.parametrize("name", SM_CASES)
def test_smoother_writes_nothing_outside_its_views(name, geometry, with_carry):
    """tail: the slice geometry, the cross-covariances being the leading T-1 steps of a T-step buffer (what a call returns and
    may be handed back); mixed: means foreign, covariances batch_inner, cross-covariances misaligned."""
    bfa = _bfa()
    c = sm_case(name)
    B, T, n = c.B, c.T, c.n
    carry = c.carry_in if with_carry else None
    plain = c.run(carry=carry)
    cT = T if with_carry else T - 1
    assert plain[0].smoothed_cross_covariances.shape[2] == cT
    gm, gP, gC = {"mixed": ("foreign", "batch_inner", "misaligned"), "tail": ("slice",) * 3}.get(geometry, (geometry,) * 3)

    def fresh():
        gs = {"smoothed_means": Guarded(gm, (B, 1, T, n)), "smoothed_covariances": Guarded(gP, (B, 1, T, n, n))}
        if geometry == "tail" and not with_carry:
            gs["smoothed_cross_covariances"] = Guarded(gC, (B, 1, T, n, n), keep=T - 1)
        else:
            gs["smoothed_cross_covariances"] = Guarded(gC, (B, 1, cT, n, n))
        return gs, bfa.PosteriorGaussianSmoothed(**{k: g.view for k, g in gs.items()})

    for mode in c.modes:
        gs, out = fresh()
        if mode == 2 and not c.serves_staged(geometry, with_carry):
            with pytest.raises(bfa.BayesFiltError) as e:
                c.run(carry=carry, out=out, mode=2)
            assert e.value.code == -1, (geometry, e.value)
            _intact(gs, written=False)
            continue
        got = c.run(carry=carry, out=out, mode=mode)
        for k in SMOOTHED:
            assert getattr(got[0], k).data_ptr() == gs[k].view.data_ptr() and tuple(getattr(got[0], k).shape) == tuple(gs[k].view.shape), k
        _equal_smoothed(got, plain, (name, geometry, mode))
        _carry_is_the_first_slot(got, (name, geometry, mode))
        _intact(gs)
        # and without a carry going out (what kalman_smoother and every plain call run): the same bits, the same guards
        gs, out = fresh()
        bare = c.run(carry=carry, out=out, mode=mode, return_carry=False)
        assert bare[1] is None
        for k in SMOOTHED:
            assert getattr(bare[0], k).data_ptr() == gs[k].view.data_ptr() and torch.equal(gs[k].view, getattr(plain[0], k)), (name, geometry, mode, k)
        _intact(gs)


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", SM_CASES)
def test_smoother_reads_nothing_outside_its_views(name, geometry):
    """The staged path (forced on slice, where it is eligible) overwrites its inputs in LDS only."""
    c = sm_case(name)
    plain = c.run()
    gs, before = _guarded_inputs(geometry, {k: getattr(c.post, k) for k in STREAMS})
    post = c.post._replace(**{k: g.view for k, g in gs.items()})
    for mode in c.modes:
        if mode == 2 and geometry != "slice":
            continue
        _equal_smoothed(c.run(post=post, mode=mode), plain, (name, geometry, mode))
        _equal_smoothed(c.run(post=post, mode=mode, carry=c.carry_in), c.run(carry=c.carry_in), (name, geometry, mode, "carry"))
    _unchanged(gs, before)


@pytest.mark.parametrize("geometry", ["slice", "foreign"])
@pytest.mark.parametrize("name", ["rts-cv", "rts-g12", "eks-l96"])
def test_smoother_two_chunks_into_one_guarded_buffer(name, geometry):
    """(On rts-cv the chunks' views have the pitch of the full-length buffer, which is not the contiguous reference layout of a
    chunk: the strided kernel serves them and must reproduce the one-shot staged run.)"""
    bfa = _bfa()
    c = sm_case(name)
    B, T, n = c.B, c.T, c.n
    s = T // 2 + 1
    full = c.run()
    gs = {"smoothed_means": Guarded(geometry, (B, 1, T, n)), "smoothed_covariances": Guarded(geometry, (B, 1, T, n, n)),
          "smoothed_cross_covariances": Guarded(geometry, (B, 1, T - 1, n, n))}
    part = lambda lo, hi: bfa.PosteriorGaussianSmoothed(**{k: g.view[:, :, lo:hi] for k, g in gs.items()})
    late, carry = c.run(post=_cut(c.post, s, T), out=part(s, T))
    _carry_is_the_first_slot((late, carry), name)
    assert tuple(late.smoothed_cross_covariances.shape) == (B, 1, T - s - 1, n, n)
    early, first = c.run(post=_cut(c.post, 0, s), out=part(0, s), carry=carry)
    assert tuple(early.smoothed_cross_covariances.shape) == (B, 1, s, n, n)
    for k in SMOOTHED:
        assert torch.equal(gs[k].view, getattr(full[0], k)), k
    for x, y in zip(first, full[1]):
        assert torch.equal(x, y)
    _intact(gs)


def _bad_outs(shape):
    """kind -> a tensor that must be refused where a float32 device tensor of ``shape`` is expected: another dtype, the host, an
    event one element too long, the second axis missing."""
    return {"float64": torch.full(shape, 7.0, dtype=torch.float64, device="cuda"),
            "bfloat16": torch.full(shape, 7.0, dtype=torch.bfloat16, device="cuda"),
            "cpu": torch.full(shape, 7.0, dtype=torch.float32),
            "event": torch.full(shape[:-1] + (shape[-1] + 1,), 7.0, dtype=torch.float32, device="cuda"),
            "axis": torch.full(shape[:1] + shape[2:], 7.0, dtype=torch.float32, device="cuda")}


def _refused(call, bad):
    before = bad.contiguous().view(torch.uint8).clone()
    with pytest.raises(ValueError):
        call(bad)
    torch.cuda.synchronize()
    assert torch.equal(bad.contiguous().view(torch.uint8), before)


@pytest.mark.parametrize("field", SMOOTHED)
def test_smoother_refuses_a_wrong_out_before_any_launch(field):
    bfa = _bfa()
    c = sm_case("rts-n3")
    B, T, n = c.B, c.T, c.n
    shape = {"smoothed_means": (B, 1, T, n), "smoothed_covariances": (B, 1, T, n, n), "smoothed_cross_covariances": (B, 1, T - 1, n, n)}[field]
    bads = _bad_outs(shape)
    bads["steps"] = torch.full(shape[:2] + (T if field.endswith("cross_covariances") else T - 1,) + shape[3:], 7.0, dtype=torch.float32, device="cuda")
    if len(shape) == 5:
        bads["event"] = torch.full(shape[:3] + (n + 1, n + 1), 7.0, dtype=torch.float32, device="cuda")
    for kind, bad in bads.items():
        _refused(lambda t: c.run(out=bfa.PosteriorGaussianSmoothed(**{field: t})), bad)
    # a returned posterior is taken back as out, cross-covariances included (the docstring's promise)
    first = c.run()[0]
    want = {k: getattr(first, k).clone() for k in SMOOTHED}
    for k in SMOOTHED:
        getattr(first, k).fill_(-3.0)
    again = c.run(out=first, cross_covariances=False)[0]
    for k in SMOOTHED:
        assert getattr(again, k).data_ptr() == getattr(first, k).data_ptr() and torch.equal(getattr(again, k), want[k]), k
    # T = 1 without a carry: the cross-covariances have no step; the empty tensor a call returned is taken back and nothing is stored
    one = _cut(c.post, 0, 1)
    single = c.run(post=one)[0]
    assert tuple(single.smoothed_cross_covariances.shape) == (B, 1, 0, n, n)
    back = c.run(post=one, out=single)[0]
    assert tuple(back.smoothed_cross_covariances.shape) == (B, 1, 0, n, n)
    assert torch.equal(back.smoothed_means, one.means) and torch.equal(back.smoothed_covariances, one.covariances)


# =====================================================================================================================
# the posterior sampler
class FfCase:
    def __init__(self, name, p, post, S, F=None, jac=None, inputs=None, spls=(0,), seed=0):
        self.name, self.p, self.post, self.S, self.inputs, self.spls = name, p, post, S, inputs, spls
        self.B, _, self.T, self.n = (int(v) for v in post.means.shape)
        self.xi = fg._noise((self.B, S, self.T, self.n), 500 + seed)
        self.xi.setflags(write=False)
        self.F, self.jac = F, jac

    @functools.cached_property
    def z(self):
        return fg._dev(self.xi)

    @functools.cached_property
    def ref(self):
        r = fg._oracle(self.post, self.F, self.xi, inputs_F=self.jac)
        r.setflags(write=False)
        return r

    def run(self, post=None, noise=None, spl=0, **kw):
        opts = dict(kw.pop("options", None) or {})
        if spl:
            opts["ffbs_spl"] = spl
        kw.setdefault("return_carry", True)        # False: (samples, None), x_out is NULL in the kernel
        if not kw["return_carry"]:
            return _bfa().posterior_sample(self.p, self.post if post is None else post, self.S, noise=self.z if noise is None else noise,
                                           inputs=self.inputs, options=opts or None, **kw), None
        return _bfa().posterior_sample(self.p, self.post if post is None else post, self.S, noise=self.z if noise is None else noise,
                                       inputs=self.inputs, options=opts or None, **kw)

    @functools.cached_property
    def carry_in(self):
        return self.run()[1]


@functools.lru_cache(maxsize=None)
def ff_case(name):
    if name in ("ffbs-n4", "ffbs-n7", "ffbs-g12", "ffbs-g24"):
        n, S, B, T, spls = {"ffbs-n4": (4, 5, 70, 9, (0,) + fg.SPLS), "ffbs-n7": (7, 3, 70, 9, (0,)),
                            "ffbs-g12": (12, 5, 3, 9, (0,)), "ffbs-g24": (24, 100, 3, 9, (0,))}[name]
        a = cm.random_stable_lgssm(n, max(1, n // 2), seed=n)
        _, post = fg._filter(a, B, T, seed=n)
        return FfCase(name, cm.product_params(a), post, S, F=a["A"], spls=spls, seed=n)
    if name in ("effbs-l63", "effbs-l96"):
        c = sm_case("eks" + name[5:])
        return FfCase(name, c.p, c.post, 5, jac=c.jac, inputs=c.inputs, seed=len(name))
    raise KeyError(name)


FF_CASES = ["ffbs-n4", "ffbs-n7", "ffbs-g12", "ffbs-g24", "effbs-l63", "effbs-l96"]


@pytest.mark.parametrize("name", FF_CASES)
def test_sampler_parity_and_route(name):
    c = ff_case(name)
    plain = c.run()
    assert tuple(plain[0].shape) == (c.B, c.S, c.T, c.n)
    fg._check(plain[0], c.ref, c.post, "contract_" + name)
    assert torch.equal(plain[1].states, plain[0][:, :, 0])
    for spl in c.spls[1:]:          # the samples per lane change the mapping, not a sample's arithmetic
        x, carry = c.run(spl=spl)
        assert torch.equal(x, plain[0]) and torch.equal(carry.states, plain[1].states), spl
    forced = c.run(options={"force_generic": 1})[0]
    fg._check(forced, c.ref, c.post, "contract_generic_" + name)


@pytest.mark.parametrize("with_carry", [False, True], ids=["nocarry", "carry"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", FF_CASES)
def test_sampler_writes_nothing_outside_its_view(name, geometry, with_carry):
    """ffbs-n4 at every samples-per-lane count: S = 5 leaves 1 (SPL = 2), 3 (SPL = 4, 8) idle slots in a trajectory's last
    lane, which must store nothing -- sample S would be the next trajectory's sample 0 or a guard.  ffbs-g24: the second sample
    block reads x_{t+1} back through these strides."""
    c = ff_case(name)
    carry = c.carry_in if with_carry else None
    plain = c.run(carry=carry)
    for spl in c.spls:
        g = Guarded(geometry, (c.B, c.S, c.T, c.n))
        x, cr = c.run(carry=carry, out=g.view, spl=spl)
        assert x.data_ptr() == g.view.data_ptr()
        assert torch.equal(g.view, plain[0]) and torch.equal(cr.states, plain[1].states), (name, geometry, spl)
        assert torch.equal(cr.states, g.view[:, :, 0])
        _intact({"samples": g})
        g = Guarded(geometry, (c.B, c.S, c.T, c.n))         # and with no carry going out
        x, cr = c.run(carry=carry, out=g.view, spl=spl, return_carry=False)
        assert cr is None and x.data_ptr() == g.view.data_ptr() and torch.equal(g.view, plain[0]), (name, geometry, spl)
        _intact({"samples": g})


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", FF_CASES)
def test_sampler_reads_nothing_outside_its_views(name, geometry):
    c = ff_case(name)
    gs, before = _guarded_inputs(geometry, dict({k: getattr(c.post, k) for k in STREAMS}, noise=c.z))
    post = c.post._replace(**{k: gs[k].view for k in STREAMS})
    for carry in (None, c.carry_in):
        plain = c.run(carry=carry)
        for spl in c.spls:
            x, cr = c.run(post=post, noise=gs["noise"].view, carry=carry, spl=spl)
            assert torch.equal(x, plain[0]) and torch.equal(cr.states, plain[1].states), (name, geometry, spl, carry is not None)
    _unchanged(gs, before)


@pytest.mark.parametrize("geometry", ["slice", "foreign", "batch_inner"])
def test_sampler_two_chunks_into_one_guarded_buffer(geometry):
    """Two sample blocks (n = 24, S = 100): the early chunk starts from the carry, both chunks read their x_{t+1} back from the
    chunk's own part of the full-length buffer."""
    c = ff_case("ffbs-g24")
    s = 4
    full = c.run()
    g = Guarded(geometry, (c.B, c.S, c.T, c.n))
    late, carry = c.run(post=_cut(c.post, s, c.T), noise=c.z[:, :, s:], out=g.view[:, :, s:])
    assert torch.equal(carry.states, late[:, :, 0])
    early, first = c.run(post=_cut(c.post, 0, s), noise=c.z[:, :, :s], out=g.view[:, :, :s], carry=carry)
    assert torch.equal(g.view, full[0]) and torch.equal(first.states, full[1].states)
    _intact({"samples": g})


def test_sampler_refuses_a_wrong_out_before_any_launch():
    c = ff_case("ffbs-n4")
    for kind, bad in _bad_outs((c.B, c.S, c.T, c.n)).items():
        _refused(lambda t: c.run(out=t), bad)


# =====================================================================================================================
# the particle smoother
class PfCase:
    B, S, T = 3, 5, 8

    def __init__(self, name, pp, mean_fn, Linv, N, method="backward", seed=0):
        bfa = _bfa()
        self.name, self.pp, self.mean_fn, self.Linv, self.N, self.method = name, pp, mean_fn, Linv, N, method
        ys = pg._simulate(pp, self.B, self.T, seed=60 + seed)
        self.hist = bfa.bootstrap_particle_filter(pp, ys, N, otf.PRNGKey(seed), None, 0.5, return_ancestors=True)
        self.hist = {k: self.hist[k] for k in ("weights", "particles", "ancestors")}
        self.n = int(self.hist["particles"].shape[3])
        self.v = pg._uniforms((self.B, self.S, self.T), 70 + seed)

    def run(self, hist=None, noise=None, **kw):
        """(samples, indices, carry); carry is None with return_carry=False (x_out / a_out are NULL in the kernel)"""
        kw.setdefault("return_carry", True)
        if not kw["return_carry"]:
            return _bfa().particle_posterior_sample(self.pp, self.hist if hist is None else hist, self.S, method=self.method,
                                                    noise=self.v if noise is None else noise, return_indices=True, **kw) + (None,)
        return _bfa().particle_posterior_sample(self.pp, self.hist if hist is None else hist, self.S, method=self.method,
                                                noise=self.v if noise is None else noise, return_indices=True, **kw)

    @functools.cached_property
    def carry_in(self):
        return self.run()[2]


@functools.lru_cache(maxsize=None)
def pf_case(name):
    if name in ("pfs-16row", "pfs-genealogy"):
        return PfCase(name, pg._l63_params(), ps.mean_lorenz63(), ps.whitener(0.1 * np.eye(3)), 100,
                      method="genealogy" if name == "pfs-genealogy" else "backward", seed=1)
    if name == "pfs-64row":
        a = ps.law_model()
        return PfCase(name, pg._linear_params(a), ps.mean_linear(a["A"]), ps.whitener(a["Q"]), 1100, seed=2)
    if name == "pfs-n12":
        return PfCase(name, pg._l96_params(12), ps.mean_lorenz96(), ps.whitener(0.1 * np.eye(12)), 64, seed=3)
    raise KeyError(name)


PF_CASES = ["pfs-16row", "pfs-64row", "pfs-n12", "pfs-genealogy"]


def _equal_pf(got, want, label):
    assert pg._bits_equal(got[0].cpu().numpy(), want[0].cpu().numpy()), label
    assert torch.equal(got[1], want[1]), label
    assert pg._bits_equal(got[2].states.cpu().numpy(), want[2].states.cpu().numpy()), label
    if want[2].slots is not None:
        assert torch.equal(got[2].slots, want[2].slots), label


@pytest.mark.parametrize("name", PF_CASES)
def test_particle_sampler_parity(name):
    c = pf_case(name)
    xs, idx, carry = c.run()
    assert tuple(xs.shape) == (c.B, c.S, c.T, c.n) and tuple(c.hist["particles"].shape) == (c.B, c.N, c.T, c.n)
    if c.method == "backward":
        tau = pg._check_parity(c.hist, xs, idx, c.v, c.mean_fn, c.Linv, label="contract_" + name)
        cm.record("particle_sampler_contract_" + name, tau=tau)
    else:
        pg._check_trace(c.hist, xs, idx, c.v)
    assert torch.equal(carry.states, xs[:, :, 0])
    _slots_follow_the_first_step(c, idx, carry)


def _slots_follow_the_first_step(c, idx, carry, hist=None):
    """The genealogy's carried slot is the parent of the chunk's first drawn particle, a[j_0, 0] (csrc/pf_sampler.hpp: the carry
    is the slot of the step BEFORE the chunk, so it is not idx[:, :, 0] itself but follows from it and the call's own ancestors)."""
    if c.method != "genealogy":
        assert carry.slots is None
        return
    anc0 = (c.hist if hist is None else hist)["ancestors"][:, :, 0]
    assert torch.equal(carry.slots, torch.gather(anc0, 1, idx[:, :, 0].long()))


@pytest.mark.parametrize("with_carry", [False, True], ids=["nocarry", "carry"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", PF_CASES)
def test_particle_sampler_writes_nothing_outside_its_view(name, geometry, with_carry):
    c = pf_case(name)
    carry = c.carry_in if with_carry else None
    plain = c.run(carry=carry)
    g = Guarded(geometry, (c.B, c.S, c.T, c.n))
    got = c.run(carry=carry, out=g.view)
    assert got[0].data_ptr() == g.view.data_ptr()
    _equal_pf(got, plain, (name, geometry))
    assert torch.equal(got[2].states, g.view[:, :, 0])
    _slots_follow_the_first_step(c, got[1], got[2])
    _intact({"samples": g})
    g = Guarded(geometry, (c.B, c.S, c.T, c.n))             # and with no carry going out
    bare = c.run(carry=carry, out=g.view, return_carry=False)
    assert bare[2] is None and bare[0].data_ptr() == g.view.data_ptr()
    assert pg._bits_equal(g.view.cpu().numpy(), plain[0].cpu().numpy()) and torch.equal(bare[1], plain[1]), (name, geometry)
    _intact({"samples": g})


def _wide_history(c, time_major):
    """The history as a [:, :N] slice of N + 8 particle slots, every extra slot holding the sentinel; physical (B, N + 8, T, ...)
    or, time-major, (B, T, N + 8, ...).  Returns (history, buffers)."""
    B, N, T, n = c.B, c.N, c.T, c.n
    hist, bufs = {}, {}
    for k, ev in (("weights", ()), ("particles", (n,)), ("ancestors", ())):
        phys = ((B, T, N + 8) if time_major else (B, N + 8, T)) + ev
        flat = torch.full((int(np.prod(phys)),), SENTINEL_BITS, dtype=torch.int32, device="cuda")
        buf = flat if k == "ancestors" else flat.view(torch.float32)
        full = buf.view(phys)
        if time_major:
            full = full.permute((0, 2, 1) + ((3,) if ev else ()))
        hist[k] = full[:, :N]
        hist[k].copy_(c.hist[k])
        bufs[k] = flat
    return hist, bufs


@pytest.mark.parametrize("form", ["time_major", "wide", "wide_time_major"])
@pytest.mark.parametrize("name", PF_CASES)
def test_particle_sampler_reads_nothing_outside_its_history(name, form):
    c = pf_case(name)
    if form == "time_major":
        hist = {k: t.permute((0, 2, 1) + ((3,) if t.dim() == 4 else ())).contiguous().permute((0, 2, 1) + ((3,) if t.dim() == 4 else ()))
                for k, t in c.hist.items()}
        bufs = {}
    else:
        hist, bufs = _wide_history(c, form == "wide_time_major")
        assert hist["weights"].stride() == hist["ancestors"].stride() and hist["particles"].stride(3) == 1
    assert hist["particles"].stride() != c.hist["particles"].stride()
    before = {k: b.clone() for k, b in bufs.items()}
    for carry in (None, c.carry_in):
        _equal_pf(c.run(hist=hist, carry=carry), c.run(carry=carry), (name, form, carry is not None))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert torch.equal(b, before[k]), k


def test_particle_sampler_refuses_a_strided_state_axis():
    c = pf_case("pfs-16row")
    x = torch.zeros((c.B, c.N, c.T, 2 * c.n), device="cuda")[..., ::2]
    x.copy_(c.hist["particles"])
    with pytest.raises(ValueError, match="contiguous"):
        c.run(hist=dict(c.hist, particles=x))


@pytest.mark.parametrize("geometry", ["slice", "foreign"])
@pytest.mark.parametrize("name", ["pfs-16row", "pfs-genealogy"])
def test_particle_sampler_two_chunks_into_one_guarded_buffer(name, geometry):
    c = pf_case(name)
    s = 3
    full = c.run()
    g = Guarded(geometry, (c.B, c.S, c.T, c.n))
    cut = lambda lo, hi: {k: t[:, :, lo:hi] for k, t in c.hist.items()}
    late = c.run(hist=cut(s, c.T), noise=c.v[:, :, s:], out=g.view[:, :, s:])
    assert torch.equal(late[2].states, late[0][:, :, 0])
    _slots_follow_the_first_step(c, late[1], late[2], hist=cut(s, c.T))
    early = c.run(hist=cut(0, s), noise=c.v[:, :, :s], out=g.view[:, :, :s], carry=late[2])
    assert pg._bits_equal(g.view.cpu().numpy(), full[0].cpu().numpy())
    assert torch.equal(torch.cat([early[1], late[1]], dim=2), full[1])
    assert pg._bits_equal(early[2].states.cpu().numpy(), full[2].states.cpu().numpy())
    _intact({"samples": g})


@pytest.mark.parametrize("name", ["pfs-16row", "pfs-genealogy"])
def test_particle_sampler_refuses_a_wrong_out_before_any_launch(name):
    c = pf_case(name)
    for kind, bad in _bad_outs((c.B, c.S, c.T, c.n)).items():
        _refused(lambda t: c.run(out=t), bad)
