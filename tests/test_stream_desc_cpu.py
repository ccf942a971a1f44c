"""The stream descriptors of the five-stream filters, no GPU: ``_alloc_stream`` and ``_stream_desc`` of
bayesianfiltering_amd/inference.py on CPU tensors.  A kernel addresses element (b, k, t, e) of a stream as
``ptr + 4 (b sB + k sK + t sT + e sE)`` with e the row-major index into the event (include/bayesfilt.h: bf_stream), so the
descriptor of a view is right exactly when that address is the view's own element -- checked here for both layouts, for 0-,
1- and 2-dimensional events and for the guarded views of tests/test_output_contract_gpu.py and
tests/test_backward_contract_gpu.py, which import the builders below (``SENTINEL_BITS``, ``sentinel_buffer``, ``guarded``,
``assert_guards_intact``) and rely on these descriptors."""
import itertools

import numpy as np
import pytest
import torch

from bayesianfiltering_amd import inference as inf

SENTINEL_BITS = 0x7FC0BEEF      # a quiet NaN with a recognisable payload: no filter output has these bits
GEOMETRIES = ("slice", "misaligned", "foreign", "batch_inner")
GUARD = 4                       # guard trajectories on each side: 4 K T E floats are a multiple of 16 bytes whatever K, T, E


def event_shapes(n):
    return {"weights": (), "means": (n,), "covariances": (n, n), "predicted_means": (n,), "predicted_covariances": (n, n)}


def sentinel_buffer(numel, device):
    """Flat float32 buffer whose every element holds SENTINEL_BITS."""
    return torch.full((numel,), SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def guarded(geometry, B, K, T, ev, g=GUARD):
    """(numel, carve): ``carve(flat)`` cuts the logical (B, K, T, *ev) view out of a flat buffer of ``numel`` elements.
    slice       [g : g + B] of a contiguous (B + 2g, K, T, *ev) buffer: guard trajectories on both sides, 16-byte aligned
    misaligned  the same slice carved at element offset 1 of the flat buffer: contiguous, but 4 bytes off 16-byte alignment
    foreign     every dimension padded: batch as above, one guard component on each side, time [3 : T + 3] of T + 6, a
                vector event [1 : n + 1] of n + 2, a matrix event the [..., 0] plane of (n, n, 2)
    batch_inner a physical (K, T, *ev, B + 2g) buffer sliced [..., g : g + B] and permuted as _alloc_stream does"""
    ev = tuple(ev)
    E = int(np.prod(ev, dtype=np.int64)) if ev else 1
    if geometry in ("slice", "misaligned"):
        off = 1 if geometry == "misaligned" else 0
        core = (B + 2 * g) * K * T * E
        return core + (4 if off else 0), lambda flat: flat[off:off + core].view((B + 2 * g, K, T) + ev)[g:g + B]
    if geometry == "foreign":
        pev = {0: (), 1: tuple(d + 2 for d in ev), 2: ev + (2,)}[len(ev)]
        full = (B + 2 * g, K + 2, T + 6) + pev
        cut = {0: (), 1: (slice(1, 1 + ev[0]),) if ev else (), 2: (slice(None), slice(None), 0)}[len(ev)]
        return int(np.prod(full)), lambda flat: flat.view(full)[(slice(g, g + B), slice(1, K + 1), slice(3, T + 3)) + cut]
    if geometry == "batch_inner":
        full = (K, T) + ev + (B + 2 * g,)
        nd = len(full)
        return int(np.prod(full)), lambda flat: flat.view(full)[..., g:g + B].permute((nd - 1,) + tuple(range(nd - 1)))
    raise ValueError(geometry)


def assert_guards_intact(bufs, carves, written=True):
    """bufs / carves: stream name -> flat buffer made by sentinel_buffer / its carve.  Every element outside the views must
    still hold SENTINEL_BITS (whole buffers, compared as int32) and, if ``written``, no element inside them may."""
    for k, buf in bufs.items():
        chk = buf.view(torch.int32).clone()
        if written:
            assert not bool((carves[k](chk) == SENTINEL_BITS).any()), f"{k}: part of the view was never written"
            carves[k](chk).fill_(SENTINEL_BITS)
        touched = (chk != SENTINEL_BITS).nonzero().flatten()
        assert touched.numel() == 0, f"{k}: {touched.numel()} elements outside the view overwritten, first at flat index {touched[:8].tolist()}"


def _address_check(view, nev):
    """Every element's address follows from the descriptor."""
    s = inf._stream_desc(view, nev)
    ev = tuple(view.shape[3:])
    assert s.ptr == view.data_ptr()
    for b, k, t in itertools.product(*(sorted({0, d - 1}) for d in view.shape[:3])):
        for e, idx in enumerate(itertools.product(*(range(d) for d in ev))):
            want = view[(b, k, t) + idx].data_ptr()
            assert s.ptr + 4 * (b * s.sB + k * s.sK + t * s.sT + e * s.sE) == want, (b, k, t, idx)
    return s


@pytest.mark.parametrize("ev", [(), (3,), (3, 3)])
def test_alloc_stream_shapes_and_strides_in_both_layouts(ev):
    B, K, T = 5, 2, 7
    E = int(np.prod(ev)) if ev else 1
    ref = inf._alloc_stream((B, K, T), ev, "reference", "cpu")
    assert tuple(ref.shape) == (B, K, T) + ev and ref.dtype == torch.float32 and ref.is_contiguous()
    s = _address_check(ref, len(ev))
    assert (s.sB, s.sK, s.sT, s.sE) == (K * T * E, T * E, E, 1)
    bi = inf._alloc_stream((B, K, T), ev, "batch_inner", "cpu")
    assert tuple(bi.shape) == (B, K, T) + ev and bi.dtype == torch.float32
    s = _address_check(bi, len(ev))
    assert (s.sB, s.sK, s.sT, s.sE) == (1, T * E * B, E * B, B if ev else 1)      # physical [K][T][E][B]; a scalar event has no sE


def test_missing_stream_is_the_null_descriptor():
    s = inf._stream_desc(None, 2)
    assert not s.ptr and (s.sB, s.sK, s.sT, s.sE) == (0, 0, 0, 0)


def test_unknown_layout_raises():
    with pytest.raises(ValueError, match="unknown layout"):
        inf._alloc_stream((2, 1, 3), (4,), "time_inner", "cpu")


def test_matrix_views_that_do_not_flatten_with_one_stride_are_refused():
    n = 3
    wide = torch.zeros(2, 1, 4, n, n + 1)[..., :n]               # rows n + 1 apart, elements 1 apart
    with pytest.raises(ValueError, match="row-major-flattenable"):
        inf._stream_desc(wide, 2)
    with pytest.raises(ValueError, match="row-major-flattenable"):
        inf._stream_desc(torch.zeros(2, 1, 4, n, n).transpose(-1, -2), 2)   # column-major matrices
    tall = torch.zeros(2, 1, 4, n + 1, n)[..., :n, :]            # padded rows BETWEEN matrices only: flattens, accepted
    s = _address_check(tall, 2)
    assert (s.sT, s.sE) == ((n + 1) * n, 1)


@pytest.mark.parametrize("name", list(event_shapes(3)))
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_guarded_views_are_accepted_with_the_expected_strides(geometry, name):
    n, B, K, T, g = 3, 5, 2, 7, GUARD
    ev = event_shapes(n)[name]
    E = int(np.prod(ev)) if ev else 1
    numel, carve = guarded(geometry, B, K, T, ev)
    flat = sentinel_buffer(numel, "cpu")
    assert flat.data_ptr() % 16 == 0
    view = carve(flat)
    assert tuple(view.shape) == (B, K, T) + ev
    s = _address_check(view, len(ev))
    got = (s.sB, s.sK, s.sT, s.sE)
    if geometry in ("slice", "misaligned"):
        assert got == (K * T * E, T * E, E, 1)
        assert (s.ptr - flat.data_ptr()) % 16 == (4 if geometry == "misaligned" else 0)
    elif geometry == "foreign":
        pE, sE = {0: (1, 1), 1: (n + 2, 1), 2: (2 * n * n, 2)}[len(ev)]      # padded event size, element stride
        assert got == ((K + 2) * (T + 6) * pE, (T + 6) * pE, pE, sE)
    else:
        assert got == (1, T * E * (B + 2 * g), E * (B + 2 * g), B + 2 * g if ev else 1)
    # the view and its guards partition the buffer: writing the view leaves exactly numel - B K T E sentinels
    view.fill_(0.0)
    assert int((flat.view(torch.int32) == SENTINEL_BITS).sum()) == numel - B * K * T * E
    again = flat.view(torch.int32).clone()
    carve(again).fill_(SENTINEL_BITS)
    assert bool((again == SENTINEL_BITS).all())


@pytest.mark.parametrize("geometry", ["slice", "misaligned", "foreign"])
def test_the_guard_check_sees_a_store_one_row_too_far(geometry):
    """What the GPU tests must catch, replayed on the CPU: a matrix store whose row mask reads ``row <= n`` instead of
    ``row < n`` writes elements n n .. n n + n - 1 of every (b, k, t) through the descriptor.  Inside a contiguous stream most
    of these land on the next step's matrix and are overwritten by it; the ones after the last step of the last trajectory
    land in the guard rows (slice), and with padded time or a strided event they land in the padding of every trajectory
    (foreign).  A correct store passes the same check.  (In the batch-inner buffer the event is not the innermost axis: the
    stray row of the last step falls behind the buffer, where no guard can see it.)"""
    n, B, K, T = 3, 5, 2, 7
    ev = (n, n)
    for rows, ok in ((n, True), (n + 1, False)):
        numel, carve = guarded(geometry, B, K, T, ev)
        flat = sentinel_buffer(numel, "cpu")
        view = carve(flat)
        s = inf._stream_desc(view, 2)
        base = (s.ptr - flat.data_ptr()) // 4
        for b, k, t in itertools.product(range(B), range(K), range(T)):      # the kernel's order: steps ascending
            for e in range(rows * n):
                flat[base + b * s.sB + k * s.sK + t * s.sT + e * s.sE] = float(e)
        if ok:
            assert_guards_intact({"covariances": flat}, {"covariances": carve})
        else:
            with pytest.raises(AssertionError, match="outside the view overwritten"):
                assert_guards_intact({"covariances": flat}, {"covariances": carve})


def _replay(flat, view, nev, elements):
    """Store float(e) at every (b, k, t, e) of ``elements`` through the view's descriptor, as a kernel would."""
    s = inf._stream_desc(view, nev)
    base = (s.ptr - flat.data_ptr()) // 4
    for b, k, t, e in elements:
        flat[base + b * s.sB + k * s.sK + t * s.sT + e * s.sE] = float(e)


@pytest.mark.parametrize("geometry", ["slice", "foreign"])
def test_the_guard_check_sees_a_cross_covariance_in_slot_T_minus_1_and_a_sample_in_slot_S(geometry):
    """The two stores tests/test_backward_contract_gpu.py must catch, replayed on the CPU.
    (1) Without a carry the smoother's cross-covariances are a (B, 1, T-1, n, n) view: a kernel that also writes entry T-1
    (the staged flush of the last time chunk with ``vs`` rows instead of ``vs - 1``) lands on the next trajectory's entry 0,
    which that trajectory overwrites -- except behind the last trajectory, in the guard rows (slice) -- and in the time
    padding of every trajectory (foreign).
    (2) The samples are (B, S, T, n) with the sample axis in the K position: a register sampler whose idle sample slots
    (ffbs_spl = 8 at S = 5) are not masked writes sample S, the next trajectory's sample 0 (slice) or the guard component
    behind the view (foreign).  Correct stores pass the same check."""
    n, B, T, S = 3, 5, 7, 5
    for steps, ok in ((T - 1, True), (T, False)):
        numel, carve = guarded(geometry, B, 1, T - 1, (n, n))
        flat = sentinel_buffer(numel, "cpu")
        _replay(flat, carve(flat), 2, itertools.product(range(B), range(1), range(steps), range(n * n)))   # trajectories ascending
        if ok:
            assert_guards_intact({"cross": flat}, {"cross": carve})
        else:
            with pytest.raises(AssertionError, match="outside the view overwritten"):
                assert_guards_intact({"cross": flat}, {"cross": carve})
    for slots, ok in ((S, True), (S + 1, False)):
        numel, carve = guarded(geometry, B, S, T, (n,))
        flat = sentinel_buffer(numel, "cpu")
        _replay(flat, carve(flat), 1, itertools.product(range(B), range(slots), range(T), range(n)))
        if ok:
            assert_guards_intact({"samples": flat}, {"samples": carve})
        else:
            with pytest.raises(AssertionError, match="outside the view overwritten"):
                assert_guards_intact({"samples": flat}, {"samples": carve})
