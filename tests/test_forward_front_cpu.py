"""The front half of the five-stream filters (inference._filter_call and its pieces) on CPU tensors: what the descriptors
point at, how initial states are expanded, what ``out=`` reuses and refuses, every error text, and how the result is
unwrapped.  No GPU: the front half never touches one, and no kernel is called.  Every expected value follows from the
tensors themselves or is an error text as the filters raised it before they shared this code."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesianfiltering_amd import _lib, inference as inf
from bayesianfiltering_amd.inference import FULL5, FILTERED, FilterCarry, PosteriorGaussianSumFiltered
from tests import common as cm

N, M, T = 3, 2, 5
A = cm.random_stable_lgssm(N, M, seed=3)
EVENT = {"weights": (), "means": (N,), "covariances": (N, N), "predicted_means": (N,), "predicted_covariances": (N, N)}
DESC = {"weights": "weights", "means": "means", "covariances": "covs", "predicted_means": "pred_means",
        "predicted_covariances": "pred_covs"}


@pytest.fixture(scope="module")
def mdl():
    return inf._Model(cm.product_params(A))


def emissions(B):
    y = torch.arange((B or 1) * T * M, dtype=torch.float32)
    return y.reshape(T, M) if B is None else y.reshape(B, T, M)


def front(mdl, B, K, **kw):
    kw.setdefault("initial_means", torch.zeros(K, N))
    kw.setdefault("initial_covariances", torch.eye(N))
    im, ic = kw.pop("initial_means"), kw.pop("initial_covariances")
    return inf._filter_call(mdl, kw.pop("y", None) if "y" in kw else emissions(B), K, "K", im, ic, device="cpu", **kw)


def strides_of(s):
    return (s.ptr, s.sB, s.sK, s.sT, s.sE)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [None, 1, 4])
@pytest.mark.parametrize("layout", ["reference", "batch_inner"])
def test_descriptors_point_at_the_tensors(mdl, B, K, layout):
    k = front(mdl, B, K, layout=layout, return_loglik=True, return_carry=True)
    Bb = B or 1
    assert (k.B, k.T, k.K, k.squeeze) == (Bb, T, K, B is None)
    assert strides_of(k.yd) == (k.y.data_ptr(), k.y.stride(0), 0, k.y.stride(1), k.y.stride(2))
    assert k.ud.ptr is None and k.keep == []
    for name in FULL5:
        t = k.bufs[name]
        assert tuple(t.shape) == (Bb, K, T) + EVENT[name] and t.dtype == torch.float32
        st = t.stride()
        sE = 1 if not EVENT[name] else st[-1]
        assert strides_of(getattr(k.od, DESC[name])) == (t.data_ptr(), st[0], st[1], st[2], sE)
        if layout == "batch_inner":
            assert st[0] == 1            # [K][T][E][B]: the batch axis is innermost
        else:
            assert t.is_contiguous()
    assert strides_of(k.od.loglik) == (k.ll.data_ptr(),) + tuple(k.ll.stride()) + (1,)
    assert k.od.coll_mean.ptr is None and k.od.coll_cov.ptr is None
    w_in, m_in, P_in = k.carry_in
    assert w_in is None and k.cr.w_in is None
    assert (k.cr.m_in, k.cr.P_in) == (m_in.data_ptr(), P_in.data_ptr())
    assert isinstance(k.c_out, FilterCarry)
    assert [tuple(t.shape) for t in k.c_out] == [(Bb, K), (Bb, K, N), (Bb, K, N, N)]
    assert (k.cr.w_out, k.cr.m_out, k.cr.P_out) == tuple(t.data_ptr() for t in k.c_out)


def test_emissions_that_are_a_transposed_view(mdl):
    base = torch.arange(4 * T * M, dtype=torch.float32).reshape(T, 4, M)
    y = base.transpose(0, 1)             # (B, T, m) with strides (m, B m, 1): not contiguous
    assert not y.is_contiguous()
    k = front(mdl, 4, 1, y=y)
    assert strides_of(k.yd) == (base.data_ptr(), M, 0, 4 * M, 1)
    y2 = torch.arange(T * M, dtype=torch.float32).reshape(M, T).t()   # unbatched (T, m) with strides (1, T)
    k = front(mdl, None, 1, y=y2)
    assert k.squeeze and strides_of(k.yd) == (y2.data_ptr(), k.y.stride(0), 0, 1, T)


def test_fields_not_asked_for_have_null_descriptors(mdl):
    k = front(mdl, 4, 3, fields=("means",))
    for name in FULL5:
        d = getattr(k.od, DESC[name])
        assert (k.bufs[name] is None) == (name != "means") and (d.ptr is None) == (name != "means")
    assert k.ll is None and k.od.loglik.ptr is None and k.c_out is None
    assert (k.cr.w_out, k.cr.m_out, k.cr.P_out) == (None, None, None)
    k = front(mdl, 4, 3, fields=())
    assert all(v is None for v in k.bufs.values())


@pytest.mark.parametrize("shape, sB", [((T,), 0), ((T, 2), 0), ((1, T, 2), 0), ((4, T, 2), T * 2)])
def test_inputs(mdl, shape, sB):
    u = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    k = front(mdl, 4, 1, inputs=u)
    d = shape[-1] if len(shape) > 1 else 1
    assert (k.ud.ptr, k.ud.sB, k.ud.sT, k.ud.sE) == (u.data_ptr(), sB, d, 1)
    assert len(k.keep) == 1 and k.keep[0].data_ptr() == u.data_ptr()


@pytest.mark.parametrize("K", [1, 3])
def test_initial_state_is_expanded_over_the_batch(mdl, K):
    B = 4
    m_k = torch.arange(K * N, dtype=torch.float32).reshape(K, N)
    P_k = torch.stack([(i + 1) * torch.eye(N) for i in range(K)])
    full_m = torch.arange(B * K * N, dtype=torch.float32).reshape(B, K, N)
    full_P = torch.arange(B * K * N * N, dtype=torch.float32).reshape(B, K, N, N)
    for im, want in [(m_k, m_k.expand(B, K, N)), (m_k[None], m_k.expand(B, K, N)), (full_m, full_m)]:
        m_in = front(mdl, B, K, initial_means=im).carry_in[1]
        assert tuple(m_in.shape) == (B, K, N) and m_in.is_contiguous() and torch.equal(m_in, want)
    assert front(mdl, B, K, initial_means=full_m).carry_in[1].data_ptr() == full_m.data_ptr()     # passed through
    for ic, want in [(2 * torch.eye(N), (2 * torch.eye(N)).expand(B, K, N, N)), (P_k, P_k.expand(B, K, N, N)), (full_P, full_P)]:
        P_in = front(mdl, B, K, initial_covariances=ic).carry_in[2]
        assert tuple(P_in.shape) == (B, K, N, N) and P_in.is_contiguous() and torch.equal(P_in, want)
    assert front(mdl, B, K, initial_covariances=full_P).carry_in[2].data_ptr() == full_P.data_ptr()
    # a default given as a function is called when there is no carry, and only then
    assert torch.equal(front(mdl, B, K, initial_means=lambda: m_k).carry_in[1], m_k.expand(B, K, N))
    carry = FilterCarry(torch.full((B, K), 1.0 / K), full_m, full_P)
    k = front(mdl, B, K, initial_means=lambda: 1 / 0, carry=carry)
    assert [t.data_ptr() for t in k.carry_in] == [t.data_ptr() for t in carry]
    assert k.cr.w_in == carry.weights.data_ptr()


def test_kalman_front(mdl):
    params = cm.product_params(A)
    k = inf._kalman_call(params, emissions(4), None, None, None, FULL5, "reference", None, False, False, "cpu")
    assert isinstance(k.mdl, inf._Lgssm) and (k.K, k.B, k.T) == (1, 4, T)
    assert torch.equal(k.carry_in[1], torch.as_tensor(A["m0"]).expand(4, 1, N))
    assert torch.equal(k.carry_in[2], torch.as_tensor(A["P0"]).expand(4, 1, N, N))
    # its carry's weights come back as (B, 1) whatever shape they were handed in
    carry = FilterCarry(torch.ones(4), torch.zeros(4, 1, N), torch.eye(N).expand(4, 1, N, N))
    k = inf._kalman_call(params, emissions(4), None, None, carry, FULL5, "reference", None, False, False, "cpu")
    assert tuple(k.carry_in[0].shape) == (4, 1)
    with pytest.raises(ValueError, match=r"initial means / covariances do not match \(B, 1, n\) / \(B, 1, n, n\)"):
        inf._kalman_call(params, emissions(4), torch.zeros(3, N), None, None, FULL5, "reference", None, False, False, "cpu")


def test_out_reuse(mdl):
    first = front(mdl, 4, 3)
    post = PosteriorGaussianSumFiltered(**first.bufs)
    again = front(mdl, 4, 3, out=post)
    assert all(again.bufs[name] is first.bufs[name] for name in FULL5)
    part = front(mdl, 4, 3, fields=FILTERED, out=post)
    assert part.bufs["means"] is first.bufs["means"] and part.bufs["predicted_means"] is None
    with pytest.raises(ValueError, match=r"out\.predicted_covariances has shape \(4, 3, 5, 3, 3\), expected \(2, 3, 5, 3, 3\)"):
        inf._filter_call(mdl, emissions(2), 3, "K", torch.zeros(3, N), torch.eye(N), fields=("predicted_covariances",), out=post,
                         device="cpu")
    with pytest.raises(ValueError, match=r"out\.means must be float32; got torch\.float64"):
        front(mdl, 4, 3, out=post._replace(means=post.means.double()))
    with pytest.raises(ValueError, match=r"out\.weights must be a torch tensor; got ndarray"):
        front(mdl, 4, 3, out=post._replace(weights=post.weights.numpy()))
    with pytest.raises(ValueError, match=r"out\.covariances must be on cpu; got a tensor on meta"):
        front(mdl, 4, 3, out=post._replace(covariances=post.covariances.to("meta")))


def test_error_texts(mdl):
    with pytest.raises(ValueError, match=r"emissions must be \(T,2\) or \(B,T,2\); got \(4, 5, 3\)"):
        front(mdl, 4, 1, y=torch.zeros(4, T, 3))
    with pytest.raises(ValueError, match=r"emissions must be \(T,2\) or \(B,T,2\); got \(1, 1, 5, 2\)"):
        front(mdl, 4, 1, y=torch.zeros(1, 1, T, M))
    for y in (torch.zeros(0, M), torch.zeros(0, T, M), torch.zeros(4, 0, M)):
        with pytest.raises(ValueError, match=r"^empty emissions$"):
            front(mdl, 4, 1, y=y)
    assert inf._emissions_desc(torch.zeros(4, 0, M), M, "cpu")[3:] == (4, 0)     # the piece itself lets them pass
    with pytest.raises(ValueError, match=r"inputs must be \(T,\), \(T,d\) or \(B,T,d\); got \(3, 5, 1\)"):
        front(mdl, 4, 1, inputs=torch.zeros(3, T, 1))
    with pytest.raises(ValueError, match=r"inputs must be \(T,\), \(T,d\) or \(B,T,d\); got \(4, 6, 1\)"):
        front(mdl, 4, 1, inputs=torch.zeros(4, T + 1, 1))
    with pytest.raises(ValueError, match=r"initial means / covariances do not match \(B, K, n\) / \(B, K, n, n\)"):
        front(mdl, 4, 3, initial_means=torch.zeros(2, 3, N))
    with pytest.raises(ValueError, match=r"initial means / covariances do not match \(B, N0, n\) / \(B, N0, n, n\)"):
        inf._filter_call(mdl, emissions(4), 3, "N0", torch.zeros(3, N), torch.eye(N).expand(2, 3, N, N), device="cpu")
    with pytest.raises(ValueError, match=r"unknown layout 'rows'"):
        front(mdl, 4, 1, layout="rows")


def test_result_unwraps_an_unbatched_call(mdl):
    k = front(mdl, None, 3, return_loglik=True, return_carry=True)
    post, ll, carry = k.result()
    for name in FULL5:
        assert tuple(getattr(post, name).shape) == (3, T) + EVENT[name]
        assert getattr(post, name).data_ptr() == k.bufs[name].data_ptr()
    assert tuple(ll.shape) == (3, T) and carry is k.c_out
    k = front(mdl, 1, 3, return_loglik=True)
    post, ll = k.result()
    assert all(getattr(post, name) is k.bufs[name] for name in FULL5) and ll is k.ll
    k = front(mdl, 4, 3, fields=FILTERED)
    post = k.result()
    assert isinstance(post, PosteriorGaussianSumFiltered) and post.means is k.bufs["means"] and post.predicted_means is None
    extra = (torch.zeros(T, N), torch.zeros(T, N, N))
    assert front(mdl, 4, 3).result(extra)[1] is extra
    # the augmented filters' form: (posterior, aux), with the carry inside aux
    k = front(mdl, None, 3, fields=FILTERED, return_carry=True)
    post, aux = k.result(aux={"carry": k.c_out})
    assert tuple(post.weights.shape) == (3, T) and aux == {"carry": k.c_out}
    assert front(mdl, 4, 3).result(aux={})[1] == {}


def test_ukf_params():
    up = inf._ukf_params((0.5, 2, 1))
    assert isinstance(up, _lib.bf_ukf_params) and (up.alpha, up.beta, up.kappa) == (0.5, 2.0, 1.0)
    up = inf._ukf_params(inf.ParamsUKF())
    assert (up.alpha, up.beta, up.kappa) == (C.c_float(1e-3).value, 2.0, 0.0)
    with pytest.raises(ValueError, match="uparams selects the unscented route; it cannot be combined with extended=True"):
        inf._ukf_params(inf.ParamsUKF(), True)
