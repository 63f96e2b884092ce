"""dmd_attention_bwd_mfma: the attention backward on the fp32 matrix cores (two tiled kernels, tokens addressed by their valid index),
on the SIMT interpreter (the kernels' own source, arrays fenced: an out-of-bounds access fails there) and on the device (-m gpu).
The workspace and dqkv start as NaN in every test.

Against float64 autograd, per (image, head) and per third dq | dk | dv (attention_cases.third_errors; every (image, head)
has its own V scale):
  * N(0, 1.5^2) inputs: <= 2e-5 of max |want|, the bound of the scalar kernels in test_attention_bwd_valid.py (the same fp32);
  * the harder families of attention_cases.BWD_CASES (a = 4, 8, the offset family), y from dmd_attention and from the
    float64 truth: error <= K_MFMA x the error of float32 CPU autograd.  K_MFMA = twice the largest ratio measured on the MI355X
    over these cases (profiles/attention_bwd_mfma_precision.txt has the table, beside the scalar kernels' ratios on the same
    inputs): 2 x 13.74 (offset family, T = 1024, dq, y from the forward; the scalar kernels: 11.94 there and 14.98 at T = 256,
    where the new ones have 11.42 -- the file says why the two scatter around each other).
The valid-extent cases are attention_cases.EXTENT_CASES, margins NaN / 3e38.  Routing: unet_train.py's switch on the interpreter
and in a device training step, which also replays as a graph bitwise."""
import functools
from types import SimpleNamespace

import pytest
import torch

from tests import abi
from tests import attention_cases as A

K_MFMA = 27.48  # 2 x 13.74


# ---- the two arms ------------------------------------------------------------------------------------------------------------------
def _arm(run, c):
    """`run` is dmd_attention_bwd_mfma on an extent, `attention` dmd_attention on (N, T, 3C), as tensors"""
    return SimpleNamespace(name=run.name, c=c, attention=lambda qkv, c: torch.from_numpy(abi.attention_default(run, qkv, c)),
                           run=lambda qkv, y, dy, h, w, vh, vw, c: torch.from_numpy(
                               abi.attention_bwd(run, qkv, y, dy, c, "dmd_attention_bwd_mfma", (h, w, vh, vw))))


SIMT = _arm(abi.Simt, 16)
GPU = _arm(abi.Gpu, 24)  # three heads: a wrong head stride shows
BOTH = abi.arms(SIMT, GPU)


# ---- against float64 autograd, full grid -----------------------------------------------------------------------------------------
# 64: one query block, one partial key tile; 80: partial query block and partial 16-key group; 256: one full tile; 320: full +
# partial tile; 512: both buffers of the staging; 768 / 1024: three / four key tiles (six / eight query tiles of the key-side kernel)
@pytest.mark.parametrize("arm,t", abi.arms_by_token_count(SIMT, GPU, (64, 80, 256, 320, 512, 768, 1024)))
def test_full_grid_vs_fp64_autograd(arm, t):
    n, c = 2, arm.c
    ref, b = A.bwd_case(n, c, t, 1, 1.5)
    got = arm.run(ref.qkv, b.y64.float(), b.dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(got).all())
    e = A.third_errors(got, b.want, c)
    print(f"ATTBWD {arm.name} T={t} N={n} C={c}: err dq|dk|dv {[f'{float(x):.2e}' for x in e.amax(dim=(0, 2))]}")
    assert float(e.max()) <= 2e-5, e


def measure(arm, t, family, a, y_from, run=None):
    """(error per (image, third, head), float32 CPU autograd's) of `run` (default: the arm's dmd_attention_bwd_mfma)"""
    n, c = 2, arm.c
    ref, b = A.bwd_case(n, c, t, family, a)
    y = arm.attention(ref.qkv, c) if y_from == "forward" else b.y64.float()
    got = run(ref.qkv, y, b.dy, c) if run is not None else arm.run(ref.qkv, y, b.dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(got).all())
    return A.third_errors(got, b.want, c), A.third_errors(b.g32, b.want, c)


@pytest.mark.parametrize("y_from", ["forward", "truth"])
@pytest.mark.parametrize("arm,t,family,a", abi.arms_by_token_count(SIMT, GPU, (64, 256, 1024), *[fa for fa in A.BWD_CASES if fa != (1, 1.5)]))
def test_harder_families_within_k_of_float32_autograd(arm, t, family, a, y_from):
    e, e32 = measure(arm, t, family, a, y_from)
    ratio = e / e32
    print(f"ATTBWD {arm.name} family={family} a={a} T={t} C={arm.c} y={y_from}: err dq|dk|dv "
          f"{[f'{float(x):.2e}' for x in e.amax(dim=(0, 2))]} float32 autograd {[f'{float(x):.2e}' for x in e32.amax(dim=(0, 2))]} "
          f"ratio dq|dk|dv {[f'{float(x):.2f}' for x in ratio.amax(dim=(0, 2))]}")
    assert float(ratio.max()) <= K_MFMA, ratio


# ---- valid extent ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extent_inputs(h, w, vh, vw):
    return A.extent_inputs(h, w, vh, vw, seed=h + vh + vw)



@pytest.mark.parametrize("arm,h,w,vh,vw", abi.arms(SIMT, GPU, A.EXTENT_CASES, tag=abi.joined_by_x))
def test_valid_extent_vs_fp64_autograd_with_garbage_margins(arm, h, w, vh, vw):
    qkv, y, dy, want, inside = extent_inputs(h, w, vh, vw)
    A.check_extent_grad(arm.run(qkv, y, dy, h, w, vh, vw, A.EXTENT_C), want, inside, vh, vw)


@pytest.mark.parametrize("arm", BOTH)
def test_whole_grid_extent_is_bitwise_the_flat_call(arm):
    n, c, t = 2, arm.c, 256
    ref, b = A.bwd_case(n, c, t, 1, 1.5)
    y = b.y64.float()
    flat = arm.run(ref.qkv, y, b.dy, 1, t, 1, t, c)
    grid = arm.run(ref.qkv.reshape(n, 16, 16, 3 * c), y.reshape(n, 16, 16, c), b.dy.reshape(n, 16, 16, c), 16, 16, 16, 16, c)
    assert bool(torch.isfinite(flat).all()) and torch.equal(grid.reshape(n, t, 3 * c), flat)


@pytest.mark.parametrize("arm", BOTH)
def test_rejects_an_extent_outside_the_grid(arm):
    qkv, y, dy, _, _ = extent_inputs(16, 16, 9, 9)
    with pytest.raises(RuntimeError, match="valid extent"):
        arm.run(qkv, y, dy, 16, 16, 17, 9, A.EXTENT_C)


# ---- run to run --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_launches_are_bitwise_equal():
    """N = 4, C = 64, T = 1024: 512 workgroups per kernel, two per CU"""
    n, c, t = 4, 64, 1024
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(n, t, 3 * c, generator=g) * 1.5
    y, dy = A.formula(qkv, c, torch.float32), torch.randn(n, t, c, generator=g)
    first = GPU.run(qkv, y, dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(first).all()) and torch.equal(first, GPU.run(qkv, y, dy, 1, t, 1, t, c))



def test_routing_switch_on_the_interpreter(monkeypatch):
    """the two-level network of tests/test_simt_host.py (attention over 64 tokens at its 8x8 level): DIAMOND_ATTN_BWD_MIN_T=64 sends
    every attention backward through dmd_attention_bwd_mfma, =0 none; the default threshold leaves 64 tokens on the scalar pair"""
    from diamond_amd import native as nv
    from diamond_amd import unet_train as UT
    from tests.simt.host_harness import engine_on_interpreter

    assert UT.ATTN_BWD_MFMA_MIN_T >= 256
    den, batch, _, _ = A.two_level_denoiser()
    den.train()
    got = {}
    with engine_on_interpreter():
        for value in ("64", "0", None):
            if value is None:
                monkeypatch.delenv("DIAMOND_ATTN_BWD_MIN_T", raising=False)
            else:
                monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", value)
            counter = A.LaunchCounter()
            monkeypatch.setattr(nv, "PROFILER", counter)
            got[value] = (A.training_step(den, batch), counter.n)
    (_, g_new), n_new = got["64"]
    (_, g_old), n_old = got["0"]
    attn = sum(v for k, v in n_new.items() if k in ("attention_kernel", "attention_f16x2_kernel", "dmd_attention"))
    assert attn >= 1 and n_new.get("dmd_attention_bwd_mfma", 0) == attn and "dmd_attention_bwd" not in n_new, n_new
    assert n_old.get("dmd_attention_bwd", 0) == attn and "dmd_attention_bwd_mfma" not in n_old, n_old
    assert got[None][1] == n_old, (got[None][1], n_old)
    A.assert_training_parity(g_new, g_old)
    assert any(not torch.equal(g_new[k], g_old[k]) for k in g_old), "the switch changed nothing"


@pytest.mark.gpu
def test_training_step_on_the_new_route_matches_the_scalar_route(monkeypatch):
    from diamond_amd import native as nv

    den = A.device_denoiser()
    den.randn_fn = lambda shape: torch.randn(*shape)
    batch = A.device_batches(1)[0]
    got = {}
    for value in ("1024", "0"):
        monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", value)
        counter = A.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        got[value] = (A.training_step(den, batch), counter.n)
    (l_new, g_new), n_new = got["1024"]
    (l_old, g_old), n_old = got["0"]
    # (the 1024-token forwards are attention_f16x2_kernel's; the mid blocks attend over 64 tokens at the 8x8 level: attention_kernel,
    #  whose backward stays on the scalar pair under either setting)
    long_t, short_t = n_new.get("attention_f16x2_kernel", 0), n_new.get("attention_kernel", 0)
    assert long_t >= 1 and n_new.get("dmd_attention_bwd_mfma", 0) == long_t and n_new.get("dmd_attention_bwd", 0) == short_t, n_new
    assert n_old.get("dmd_attention_bwd", 0) == long_t + short_t and "dmd_attention_bwd_mfma" not in n_old, n_old
    assert torch.equal(l_new, l_old) and all(bool(torch.isfinite(v).all()) for v in g_new.values())
    A.assert_training_parity(g_new, g_old)


@pytest.mark.gpu
def test_graphed_training_step_on_the_new_route_is_bitwise_the_eager_loop(monkeypatch):
    """the launches record into a hipGraph (no allocation, no synchronisation) and replay exactly the eager loop, in the manner of
    tests/test_offgrid_train.py"""
    A.check_graphed_training_step_is_bitwise_the_eager_loop(monkeypatch)
