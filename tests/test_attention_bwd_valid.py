"""dmd_attention_bwd_valid: the gradient of dmd_attention_valid over the (valid_h, valid_w) part of an (H, W) token grid, against
float64 torch autograd of the attention of the CROPPED tensors.  The buffer margins of qkv, y and dy hold huge values and NaN (what
torch.empty may hand the kernel): none of them may reach a result, and dqkv is exactly zero outside the extent.  With the extent
the whole grid the result is bitwise dmd_attention_bwd's, whichever way the whole grid is written: (H, W, H, W) or one row of H W
tokens, (1, H W, 1, H W), which is how dmd_attention_bwd launches the scalar pair.  On the SIMT interpreter (CPU) and on the device
(-m gpu)."""
import numpy as np
import pytest
import torch

CASES = [(16, 16, 9, 9), (16, 16, 9, 10), (32, 32, 18, 20), (64, 64, 36, 36)]
C, N = 64, 2


def make_inputs(h, w, vh, vw, seed, N=N, C=C):
    """qkv / y / dy (N, H, W, .) float32 with garbage margins, and the float64 reference dqkv of the valid tokens"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(N, h, w, 3 * C, generator=g, dtype=torch.float64) * 1.5
    dy = torch.randn(N, h, w, C, generator=g, dtype=torch.float64)
    q32 = qkv.float()
    crop = q32[:, :vh, :vw].reshape(N, vh * vw, 3 * C).double().requires_grad_(True)
    heads = lambda t: t.reshape(N, vh * vw, C // 8, 8).transpose(1, 2)
    q, k, v = (heads(crop[..., i * C:(i + 1) * C]) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(8.0), dim=-1)
    y64 = (p @ v).transpose(1, 2).reshape(N, vh, vw, C)
    dy32 = dy.float()
    y64.backward(dy32[:, :vh, :vw].double())
    want = crop.grad.reshape(N, vh, vw, 3 * C)
    y = torch.empty(N, h, w, C)
    y[:, :vh, :vw] = y64.detach().float()
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[:vh, :vw] = True
    garbage = lambda t: t.masked_fill(~inside[None, :, :, None], float("nan")).masked_fill(
        (~inside[None, :, :, None]) & (torch.arange(t.shape[-1]) % 2 == 0), 3e38)
    return garbage(q32), garbage(y), garbage(dy32), want, inside


def check(dqkv, want, inside, vh, vw):
    got = dqkv[:, :vh, :vw].double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 2e-5, err
    out = dqkv[:, ~inside]
    assert bool((out == 0).all()) and not bool(torch.signbit(out).any()), "dqkv outside the valid extent is not zero"


def run_simt(qkv, y, dy, h, w, vh, vw, full=False):
    N, C = qkv.shape[0], qkv.shape[-1] // 3
    from tests.simt import loader as S
    from tests.simt.fence import fenced as G

    L = S.lib()
    a = [G(t.numpy()) for t in (qkv, y, dy)]
    ws = G(np.full(L.dmd_attention_bwd_workspace_floats(N, h * w, C), np.nan, dtype=np.float32))
    dqkv = G(np.full(tuple(qkv.shape), np.nan, dtype=np.float32))
    if full:
        S.check(L.dmd_attention_bwd(*(S.ptr(x) for x in a), S.ptr(dqkv), S.ptr(ws), N, h * w, C, 8, None), "dmd_attention_bwd")
    else:
        S.check(L.dmd_attention_bwd_valid(*(S.ptr(x) for x in a), S.ptr(dqkv), S.ptr(ws), N, h, w, vh, vw, C, 8, None),
                "dmd_attention_bwd_valid")
    return torch.from_numpy(np.array(dqkv))


def run_gpu(qkv, y, dy, h, w, vh, vw, full=False):
    N, C = qkv.shape[0], qkv.shape[-1] // 3
    from diamond_amd import native as nv

    a = [t.cuda().contiguous() for t in (qkv, y, dy)]
    ws = torch.full((int(nv.lib().dmd_attention_bwd_workspace_floats(N, h * w, C)),), float("nan"), device="cuda")
    dqkv = torch.full(tuple(qkv.shape), float("nan"), device="cuda")
    if full:
        nv.check(nv.lib().dmd_attention_bwd(*(nv.fptr(x) for x in a), nv.fptr(dqkv), nv.fptr(ws), N, h * w, C, 8, nv.stream()),
                 "dmd_attention_bwd")
    else:
        nv.check(nv.lib().dmd_attention_bwd_valid(*(nv.fptr(x) for x in a), nv.fptr(dqkv), nv.fptr(ws), N, h, w, vh, vw, C, 8,
                                                  nv.stream()), "dmd_attention_bwd_valid")
    return dqkv.cpu()


RUNNERS = {"simt": run_simt, "gpu": pytest.param(run_gpu, marks=pytest.mark.gpu)}


@pytest.mark.parametrize("run", RUNNERS.values(), ids=RUNNERS.keys())
@pytest.mark.parametrize("h,w,vh,vw", CASES)
def test_attention_bwd_valid_vs_fp64_autograd(run, h, w, vh, vw):
    qkv, y, dy, want, inside = make_inputs(h, w, vh, vw, seed=h + vh + vw)
    check(run(qkv, y, dy, h, w, vh, vw), want, inside, vh, vw)


@pytest.mark.parametrize("run", RUNNERS.values(), ids=RUNNERS.keys())
@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_attention_bwd_valid_over_the_whole_grid_is_bitwise_attention_bwd(run, h, w):
    qkv, y, dy, want, inside = make_inputs(h, w, h, w, seed=h)
    got = run(qkv, y, dy, h, w, h, w)
    check(got, want, inside, h, w)
    assert torch.equal(got, run(qkv, y, dy, h, w, h, w, full=True))


@pytest.mark.parametrize("run", RUNNERS.values(), ids=RUNNERS.keys())
@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_attention_bwd_valid_over_the_whole_grid_as_one_row_of_tokens_is_bitwise_the_same(run, h, w):
    """(H, W, H, W) against (1, H W, 1, H W): the extent dmd_attention_bwd gives the scalar pair"""
    qkv, y, dy, want, inside = make_inputs(h, w, h, w, seed=h)
    got = run(qkv, y, dy, h, w, h, w)
    check(got, want, inside, h, w)
    one_row = lambda t: t.reshape(N, 1, h * w, -1)
    assert torch.equal(one_row(got), run(one_row(qkv), one_row(y), one_row(dy), 1, h * w, 1, h * w))


@pytest.mark.parametrize("run", RUNNERS.values(), ids=RUNNERS.keys())
def test_attention_bwd_with_a_partial_last_workgroup(run):
    """T = 100: the second workgroup of 64 threads holds 36 tokens"""
    qkv, y, dy, want, inside = make_inputs(1, 100, 1, 100, seed=100, N=1, C=16)
    check(run(qkv, y, dy, 1, 100, 1, 100, full=True), want, inside, 1, 100)


@pytest.mark.parametrize("run", RUNNERS.values(), ids=RUNNERS.keys())
def test_attention_bwd_valid_rejects_an_extent_outside_the_grid(run):
    qkv, y, dy, _, _ = make_inputs(16, 16, 9, 9, seed=1)
    with pytest.raises(RuntimeError, match="valid extent"):
        run(qkv, y, dy, 16, 16, 17, 9)
