"""dmd_linear with operands in either storage order (dmd_linear_params.trans_a / trans_w) and a masked K tail: BITWISE the plain call
on materialised copies -- `.t().contiguous()`, zero-padded along K to a multiple of 16 -- which is what the LSTM backward used to
make before every weight / data gradient GEMM.  Same 16-wide steps, same four MFMAs per step, same split-K rule on the rounded K.

Shapes: (5, 512, 256) and (2048, 1024, 256) are the head and LSTM weight-gradient GEMMs on the route without split-K; (17, 33, 72)
has a K tail (72 = 3 burn-in frames x 24 slots) and ragged M / N; (256, 2048, 528) and (40, 512, 1024) take split-K (528 rounds
to 528 = 33 x 16: NOT a multiple of 64, so it stays on the plain route -- the rule is the padded copy's; 1024 splits).
The interpreter twin (no GPU) runs the small shapes between inaccessible pages: a read past an operand faults."""
import numpy as np
import pytest
import torch

SHAPES = [(5, 512, 256), (2048, 1024, 256), (17, 33, 72), (256, 2048, 528), (40, 512, 1024)]
MODES = [(1, 0), (0, 1), (1, 1)]


def _pad16(k):
    return (k + 15) // 16 * 16


def _operands(rng, m, n, k, ta, tw, wide):
    """logical A (M, K), W (N, K) as numpy views of their storage: transposed -> stored (K, rows [+ 3]); else (rows, K [+ 4])"""
    def one(rows, trans):
        if trans:
            st = rng.standard_normal((k, rows + (3 if wide else 0))).astype(np.float32)
            return st, st[:, :rows].T
        st = rng.standard_normal((rows, k + (4 if wide else 0))).astype(np.float32)
        return st, st[:, :k]
    sa, a = one(m, ta)
    sw, w = one(n, tw)
    return sa, a, sw, w


def _materialised(x, k):
    out = np.zeros((x.shape[0], _pad16(k)), dtype=np.float32)
    out[:, :k] = x
    return out


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["tight", "wide-ld"])
@pytest.mark.parametrize("ta,tw", MODES, ids=["A^T", "W^T", "A^T-W^T"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_transposed_operands_bitwise_the_materialised_call_gpu(m, n, k, ta, tw, wide):
    from diamond_amd import engine as E

    rng = np.random.default_rng(m * 7 + n * 3 + k + 2 * ta + tw)
    sa, a, sw, w = _operands(rng, m, n, k, ta, tw, wide)
    dsa, dsw = torch.from_numpy(sa).cuda(), torch.from_numpy(sw).cuda()
    da = dsa[:, :m].t() if ta else dsa[:, :k]
    dw = dsw[:, :n].t() if tw else dsw[:, :k]
    assert tuple(da.shape) == (m, k) and tuple(dw.shape) == (n, k)
    ca, cw = torch.from_numpy(_materialised(a, k)).cuda(), torch.from_numpy(_materialised(w, k)).cuda()
    bias = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    c0 = torch.from_numpy(rng.standard_normal((m, n)).astype(np.float32)).cuda()

    got, want = E.linear(da, dw), E.linear(ca, cw)
    assert torch.equal(got, want), f"max diff {float((got - want).abs().max()):.3e}"
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    # with bias, accumulated onto an existing C
    got, want = E.linear(da, dw, bias, out=c0.clone(), accumulate=True), E.linear(ca, cw, bias, out=c0.clone(), accumulate=True)
    assert torch.equal(got, want), f"bias + accumulate: max diff {float((got - want).abs().max()):.3e}"
    # and it is the product: against float64
    ref = torch.from_numpy(a.astype(np.float64) @ w.astype(np.float64).T).cuda()
    assert float((E.linear(da, dw).double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.gpu
def test_lstm_heads_backward_on_the_operands_where_they_lie_gpu():
    """LstmHeadsFn.backward hands dmd_linear transposed VIEWS (no copies): dW_heads bitwise the GEMM on materialised copies, every
    gradient against torch's LSTMCell + Linear autograd."""
    from diamond_amd import engine as E
    from diamond_amd import lstm_native as LN

    g = torch.Generator().manual_seed(5)
    b, f, hd, na = 6, 64, 32, 4
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).cuda().requires_grad_()
    x, hx, cx = mk(b, f), mk(b, hd), mk(b, hd)
    w_ih, w_hh, b_ih, b_hh, w_heads, b_heads = mk(4 * hd, f), mk(4 * hd, hd), mk(4 * hd), mk(4 * hd), mk(na + 1, hd), mk(na + 1)
    heads, h, c = LN.LstmHeadsFn.apply(E.PackCache(), x, hx, cx, w_ih, w_hh, b_ih, b_hh, w_heads, b_heads)
    dheads, dh = torch.randn(b, na + 1, generator=g).cuda(), torch.randn(b, hd, generator=g).cuda()
    leaves = [x, hx, w_ih, w_hh, w_heads]
    got = torch.autograd.grad([heads, h], leaves, [dheads, dh])

    pad = lambda t: torch.nn.functional.pad(t.contiguous(), (0, _pad16(t.shape[1]) - t.shape[1]))
    assert torch.equal(got[4], E.linear(pad(dheads.t()), pad(h.detach().t())))  # the old route: contiguous copies, K zero-padded

    gates = x @ w_ih.t() + b_ih + hx @ w_hh.t() + b_hh
    i_, f_, g_, o_ = gates.chunk(4, 1)
    c2 = torch.sigmoid(f_) * cx + torch.sigmoid(i_) * torch.tanh(g_)
    h2 = torch.sigmoid(o_) * torch.tanh(c2)
    want = torch.autograd.grad([h2 @ w_heads.t() + b_heads, h2], leaves, [dheads, dh])
    for name, a_, b_ in zip(("dx", "dhx", "dw_ih", "dw_hh", "dw_heads"), got, want):
        assert float((a_ - b_).abs().max()) <= 2e-5 * max(1.0, float(b_.abs().max())), name


# ---- the interpreter twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,ta,tw", [(5, 512, 256, 1, 1), (17, 33, 72, 1, 0), (17, 33, 72, 0, 1), (17, 33, 72, 1, 1), (40, 512, 1024, 1, 1),
                                         (9, 20, 5, 0, 1)])
def test_transposed_operands_bitwise_the_materialised_call_interpreter(m, n, k, ta, tw):
    from diamond_amd import native as nv
    from tests.simt import loader as S
    from tests.simt.fence import fenced as G

    rng = np.random.default_rng(m + n + k)
    sa, a, sw, w = _operands(rng, m, n, k, ta, tw, False)
    bias = G(rng.standard_normal(n).astype(np.float32))
    c0 = rng.standard_normal((m, n)).astype(np.float32)

    def run(A, lda, W, ldw, ta_, tw_):
        A, W, c = G(A), G(W), G(c0.copy())
        p = nv.LinearParams()
        p.M, p.N, p.K, p.A, p.lda, p.W, p.ldw, p.bias, p.C, p.ldc = m, n, k, S.ptr(A), lda, S.ptr(W), ldw, S.ptr(bias), S.ptr(c), n
        p.accumulate, p.trans_a, p.trans_w = 1, ta_, tw_
        S.check(S.lib().dmd_linear(p, None), "dmd_linear")
        return np.array(c)

    got = run(sa, sa.shape[1], sw, sw.shape[1], ta, tw)
    ca, cw = _materialised(a, k), _materialised(w, k)
    p_k = _pad16(k)
    A, W, c = G(ca), G(cw), G(c0.copy())
    p = nv.LinearParams()
    p.M, p.N, p.K, p.A, p.lda, p.W, p.ldw, p.bias, p.C, p.ldc = m, n, p_k, S.ptr(A), p_k, S.ptr(W), p_k, S.ptr(bias), S.ptr(c), n
    p.accumulate = 1
    S.check(S.lib().dmd_linear(p, None), "dmd_linear")
    assert got.tobytes() == np.array(c).tobytes()
    ref = a.astype(np.float64) @ w.astype(np.float64).T + np.asarray(bias) + c0
    assert np.abs(got - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max()) * max(1.0, np.sqrt(k) / 4)
