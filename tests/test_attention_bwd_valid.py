"""dmd_attention_bwd_valid: the gradient of dmd_attention_valid over the (valid_h, valid_w) part of an (H, W) token grid, against
float64 torch autograd of the attention of the CROPPED tensors.  The buffer margins of qkv, y and dy hold huge values and NaN (what
torch.empty may hand the kernel): none of them may reach a result, and dqkv is exactly zero outside the extent.  With the extent
the whole grid the result is bitwise dmd_attention_bwd's, whichever way the whole grid is written: (H, W, H, W) or one row of H W
tokens, (1, H W, 1, H W), which is how dmd_attention_bwd launches the scalar pair.  On the SIMT interpreter (CPU) and on the device
(-m gpu)."""
import pytest
import torch

from tests import abi
from tests.attention_cases import EXTENT_CASES as CASES, EXTENT_N as N, check_extent_grad as check, extent_inputs as make_inputs


def launch(run, qkv, y, dy, h, w, vh, vw, full=False):
    """dmd_attention_bwd_valid on the (vh, vw) extent of the (h, w) grid; full=True: dmd_attention_bwd over all of its tokens"""
    c = qkv.shape[-1] // 3
    got = abi.attention_bwd(run, qkv, y, dy, c) if full else abi.attention_bwd(run, qkv, y, dy, c, "dmd_attention_bwd_valid", (h, w, vh, vw))
    return torch.from_numpy(got)


@pytest.mark.parametrize("run", abi.RUNNERS)
@pytest.mark.parametrize("h,w,vh,vw", CASES)
def test_attention_bwd_valid_vs_fp64_autograd(run, h, w, vh, vw):
    qkv, y, dy, want, inside = make_inputs(h, w, vh, vw, seed=h + vh + vw)
    check(launch(run, qkv, y, dy, h, w, vh, vw), want, inside, vh, vw)


@pytest.mark.parametrize("run", abi.RUNNERS)
@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_attention_bwd_valid_over_the_whole_grid_is_bitwise_attention_bwd(run, h, w):
    qkv, y, dy, want, inside = make_inputs(h, w, h, w, seed=h)
    got = launch(run, qkv, y, dy, h, w, h, w)
    check(got, want, inside, h, w)
    assert torch.equal(got, launch(run, qkv, y, dy, h, w, h, w, full=True))


@pytest.mark.parametrize("run", abi.RUNNERS)
@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_attention_bwd_valid_over_the_whole_grid_as_one_row_of_tokens_is_bitwise_the_same(run, h, w):
    """(H, W, H, W) against (1, H W, 1, H W): the extent dmd_attention_bwd gives the scalar pair"""
    qkv, y, dy, want, inside = make_inputs(h, w, h, w, seed=h)
    got = launch(run, qkv, y, dy, h, w, h, w)
    check(got, want, inside, h, w)
    one_row = lambda t: t.reshape(N, 1, h * w, -1)
    assert torch.equal(one_row(got), launch(run, one_row(qkv), one_row(y), one_row(dy), 1, h * w, 1, h * w))


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_attention_bwd_with_a_partial_last_workgroup(run):
    """T = 100: the second workgroup of 64 threads holds 36 tokens"""
    qkv, y, dy, want, inside = make_inputs(1, 100, 1, 100, seed=100, N=1, C=16)
    check(launch(run, qkv, y, dy, 1, 100, 1, 100, full=True), want, inside, 1, 100)


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_attention_bwd_valid_rejects_an_extent_outside_the_grid(run):
    qkv, y, dy, _, _ = make_inputs(16, 16, 9, 9, seed=1)
    with pytest.raises(RuntimeError, match="valid extent"):
        launch(run, qkv, y, dy, 16, 16, 17, 9)
