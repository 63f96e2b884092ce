"""dmd_attention_bwd_mfma: the attention backward on the fp32 matrix cores (two tiled kernels, tokens addressed by their valid index),
on the SIMT interpreter (the kernels' own source, arrays fenced: an out-of-bounds access fails there) and on the device (-m gpu).
The workspace and dqkv start as NaN in every test.

Against float64 autograd, per (image, head) and per third dq | dk | dv (test_attention_precision.third_errors; every (image, head)
has its own V scale):
  * N(0, 1.5^2) inputs: <= 2e-5 of max |want|, the bound of the scalar kernels in test_attention_bwd_valid.py (the same fp32);
  * the harder families of test_attention_precision.BWD_CASES (a = 4, 8, the offset family), y from dmd_attention and from the
    float64 truth: error <= K_MFMA x the error of float32 CPU autograd.  K_MFMA = twice the largest ratio measured on the MI355X
    over these cases (profiles/attention_bwd_mfma_precision.txt has the table, beside the scalar kernels' ratios on the same
    inputs): 2 x 13.74 (offset family, T = 1024, dq, y from the forward; the scalar kernels: 11.94 there and 14.98 at T = 256,
    where the new ones have 11.42 -- the file says why the two scatter around each other).
The valid-extent cases are test_attention_bwd_valid's, margins NaN / 3e38.  Routing: unet_train.py's switch on the interpreter
and in a device training step, which also replays as a graph bitwise."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import test_attention_bwd_valid as V
from tests import test_attention_precision as P

K_MFMA = 27.48  # 2 x 13.74


# ---- the two runners ---------------------------------------------------------------------------------------------------------------
def run_simt(qkv, y, dy, h, w, vh, vw, c):
    from tests.simt import loader as S
    from tests.simt.fence import fenced as G

    L = S.lib()
    n = qkv.shape[0]
    a = [G(t.contiguous().numpy()) for t in (qkv, y, dy)]
    ws = G(np.full(L.dmd_attention_bwd_workspace_floats(n, h * w, c), np.nan, dtype=np.float32))
    dqkv = G(np.full(tuple(qkv.shape), np.nan, dtype=np.float32))
    S.check(L.dmd_attention_bwd_mfma(*(S.ptr(x) for x in a), S.ptr(dqkv), S.ptr(ws), n, h, w, vh, vw, c, 8, None), "dmd_attention_bwd_mfma")
    return torch.from_numpy(np.array(dqkv))


def run_gpu(qkv, y, dy, h, w, vh, vw, c):
    from diamond_amd import native as nv

    n = qkv.shape[0]
    a = [t.cuda().contiguous() for t in (qkv, y, dy)]
    ws = torch.full((int(nv.lib().dmd_attention_bwd_workspace_floats(n, h * w, c)),), float("nan"), device="cuda")
    dqkv = torch.full(tuple(qkv.shape), float("nan"), device="cuda")
    nv.check(nv.lib().dmd_attention_bwd_mfma(*(nv.fptr(x) for x in a), nv.fptr(dqkv), nv.fptr(ws), n, h, w, vh, vw, c, 8, nv.stream()),
             "dmd_attention_bwd_mfma")
    return dqkv.cpu()


SIMT = SimpleNamespace(name="simt", run=run_simt, c=16, attention=P.Simt.attention)
GPU = SimpleNamespace(name="gpu", run=run_gpu, c=24, attention=P.Gpu.attention)  # three heads: a wrong head stride shows


def arms(ts, *more, simt_max_t=512):
    """(arm, t, *extra) cases: the interpreter arm gets T <= 512 only, the device arm every T"""
    extras = [()] if not more else [e if isinstance(e, tuple) else (e,) for e in more]
    out = []
    for t in ts:
        for e in extras:
            tag = "-".join([str(t)] + [str(x) for x in e])
            if t <= simt_max_t:
                out.append(pytest.param(SIMT, t, *e, id=f"simt-{tag}"))
            out.append(pytest.param(GPU, t, *e, marks=pytest.mark.gpu, id=f"gpu-{tag}"))
    return out


BOTH = [pytest.param(SIMT, id="simt"), pytest.param(GPU, marks=pytest.mark.gpu, id="gpu")]


# ---- against float64 autograd, full grid -----------------------------------------------------------------------------------------
# 64: one query block, one partial key tile; 80: partial query block and partial 16-key group; 256: one full tile; 320: full +
# partial tile; 512: both buffers of the staging; 768 / 1024: three / four key tiles (six / eight query tiles of the key-side kernel)
@pytest.mark.parametrize("arm,t", arms((64, 80, 256, 320, 512, 768, 1024)))
def test_full_grid_vs_fp64_autograd(arm, t):
    n, c = 2, arm.c
    ref, b = P.bwd_case(n, c, t, 1, 1.5)
    got = arm.run(ref.qkv, b.y64.float(), b.dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(got).all())
    e = P.third_errors(got, b.want, c)
    print(f"ATTBWD {arm.name} T={t} N={n} C={c}: err dq|dk|dv {[f'{float(x):.2e}' for x in e.amax(dim=(0, 2))]}")
    assert float(e.max()) <= 2e-5, e


def measure(arm, t, family, a, y_from, run=None):
    """(error per (image, third, head), float32 CPU autograd's) of `run` (default: the arm's dmd_attention_bwd_mfma)"""
    n, c = 2, arm.c
    ref, b = P.bwd_case(n, c, t, family, a)
    y = arm.attention(ref.qkv, c) if y_from == "forward" else b.y64.float()
    got = run(ref.qkv, y, b.dy, c) if run is not None else arm.run(ref.qkv, y, b.dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(got).all())
    return P.third_errors(got, b.want, c), P.third_errors(b.g32, b.want, c)


@pytest.mark.parametrize("y_from", ["forward", "truth"])
@pytest.mark.parametrize("arm,t,family,a", arms((64, 256, 1024), *[fa for fa in P.BWD_CASES if fa != (1, 1.5)]))
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
    return V.make_inputs(h, w, vh, vw, seed=h + vh + vw)


def extent_arms():
    out = []
    for case in V.CASES:
        tag = "x".join(str(x) for x in case)
        out.append(pytest.param(SIMT, *case, id=f"simt-{tag}"))
        out.append(pytest.param(GPU, *case, marks=pytest.mark.gpu, id=f"gpu-{tag}"))
    return out


@pytest.mark.parametrize("arm,h,w,vh,vw", extent_arms())
def test_valid_extent_vs_fp64_autograd_with_garbage_margins(arm, h, w, vh, vw):
    qkv, y, dy, want, inside = extent_inputs(h, w, vh, vw)
    V.check(arm.run(qkv, y, dy, h, w, vh, vw, V.C), want, inside, vh, vw)


@pytest.mark.parametrize("arm", BOTH)
def test_whole_grid_extent_is_bitwise_the_flat_call(arm):
    n, c, t = 2, arm.c, 256
    ref, b = P.bwd_case(n, c, t, 1, 1.5)
    y = b.y64.float()
    flat = arm.run(ref.qkv, y, b.dy, 1, t, 1, t, c)
    grid = arm.run(ref.qkv.reshape(n, 16, 16, 3 * c), y.reshape(n, 16, 16, c), b.dy.reshape(n, 16, 16, c), 16, 16, 16, 16, c)
    assert bool(torch.isfinite(flat).all()) and torch.equal(grid.reshape(n, t, 3 * c), flat)


@pytest.mark.parametrize("arm", BOTH)
def test_rejects_an_extent_outside_the_grid(arm):
    qkv, y, dy, _, _ = extent_inputs(16, 16, 9, 9)
    with pytest.raises(RuntimeError, match="valid extent"):
        arm.run(qkv, y, dy, 16, 16, 17, 9, V.C)


# ---- run to run --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_launches_are_bitwise_equal():
    """N = 4, C = 64, T = 1024: 512 workgroups per kernel, two per CU"""
    n, c, t = 4, 64, 1024
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(n, t, 3 * c, generator=g) * 1.5
    y, dy = P.formula(qkv, c, torch.float32), torch.randn(n, t, c, generator=g)
    first = run_gpu(qkv, y, dy, 1, t, 1, t, c)
    assert bool(torch.isfinite(first).all()) and torch.equal(first, run_gpu(qkv, y, dy, 1, t, 1, t, c))


# ---- routing and the training step -------------------------------------------------------------------------------------------------
class _Counter:
    """stands in for native.PROFILER: counts launches per key (no timing)"""

    def __init__(self):
        self.n = {}
        self._pending = None

    def annotate(self, key, flops, nbytes):
        self._pending = key

    def call(self, name, fn, args):
        key, self._pending = self._pending or name, None
        self.n[key] = self.n.get(key, 0) + 1
        return fn(*args)


def _step(den, batch, seed=77):
    den.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    loss, _ = den(batch)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in den.named_parameters()}


def assert_training_parity(new, old):
    """every parameter gradient within 2e-5 of max |g| (README, "Parity")"""
    bad = {}
    for k, g in old.items():
        err = float((new[k].double() - g.double()).abs().max() / g.double().abs().max().clamp_min(1e-30))
        if not err <= 2e-5:
            bad[k] = err
    assert not bad, bad


def test_routing_switch_on_the_interpreter(monkeypatch):
    """the two-level network of tests/test_simt_host.py (attention over 64 tokens at its 8x8 level): DIAMOND_ATTN_BWD_MIN_T=64 sends
    every attention backward through dmd_attention_bwd_mfma, =0 none; the default threshold leaves 64 tokens on the scalar pair"""
    import diamond_amd as D
    from diamond_amd import native as nv
    from diamond_amd import unet_train as UT
    from diamond_amd.inner_model import InnerModelConfig
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames
    from tests import wide_configs as W
    from tests.simt.host_harness import engine_on_interpreter

    assert UT.ATTN_BWD_MFMA_MIN_T >= 256
    cfg = dict(W.DENOISER, depths=[1, 1], channels=[64, 96], attn_depths=[0, 1])
    den = D.Denoiser(D.DenoiserConfig(inner_model=InnerModelConfig(**cfg), sigma_data=0.5, sigma_offset_noise=0.3))
    fill_module_(den, W.WEIGHT_SEED)
    den.setup_training(D.SigmaDistributionConfig(**W.SIGMA_DIST))
    den.randn_fn = lambda shape: torch.randn(*shape)
    den.train()
    g = torch.Generator().manual_seed(31)
    batch = SimpleNamespace(obs=synthetic_frames(g, 1, 5, 3, 16, 16), act=synthetic_actions(g, 4, 1, 5), mask_padding=torch.ones(1, 5, dtype=torch.bool))
    got = {}
    with engine_on_interpreter():
        for value in ("64", "0", None):
            if value is None:
                monkeypatch.delenv("DIAMOND_ATTN_BWD_MIN_T", raising=False)
            else:
                monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", value)
            counter = _Counter()
            monkeypatch.setattr(nv, "PROFILER", counter)
            got[value] = (_step(den, batch), counter.n)
    (_, g_new), n_new = got["64"]
    (_, g_old), n_old = got["0"]
    attn = sum(v for k, v in n_new.items() if k in ("attention_kernel", "attention_f16x2_kernel", "dmd_attention"))
    assert attn >= 1 and n_new.get("dmd_attention_bwd_mfma", 0) == attn and "dmd_attention_bwd" not in n_new, n_new
    assert n_old.get("dmd_attention_bwd", 0) == attn and "dmd_attention_bwd_mfma" not in n_old, n_old
    assert got[None][1] == n_old, (got[None][1], n_old)
    assert_training_parity(g_new, g_old)
    assert any(not torch.equal(g_new[k], g_old[k]) for k in g_old), "the switch changed nothing"


def _device_denoiser():
    """the default denoiser at 64x64 with attention at its 32x32 level: 1024 tokens, batch 2"""
    import diamond_amd as D
    from diamond_amd.testing import fill_module_
    from tests.conftest import WEIGHT_SEED

    agent = D.Agent(D.default_agent_config(denoiser_attn_depths=(0, 1, 0, 0)))
    fill_module_(agent, WEIGHT_SEED)
    den = agent.to("cuda").eval().denoiser
    den.train()
    den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
    return den


def _device_batches(count):
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    g = torch.Generator().manual_seed(8)
    return [SimpleNamespace(obs=synthetic_frames(g, 2, 5, 3, 64, 64).cuda(), act=synthetic_actions(g, 4, 2, 5).cuda(),
                            mask_padding=torch.ones(2, 5, dtype=torch.bool).cuda()) for _ in range(count)]


@pytest.mark.gpu
def test_training_step_on_the_new_route_matches_the_scalar_route(monkeypatch):
    from diamond_amd import native as nv

    den = _device_denoiser()
    den.randn_fn = lambda shape: torch.randn(*shape)
    batch = _device_batches(1)[0]
    got = {}
    for value in ("1024", "0"):
        monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", value)
        counter = _Counter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        got[value] = (_step(den, batch), counter.n)
    (l_new, g_new), n_new = got["1024"]
    (l_old, g_old), n_old = got["0"]
    # (the 1024-token forwards are attention_f16x2_kernel's; the mid blocks attend over 64 tokens at the 8x8 level: attention_kernel,
    #  whose backward stays on the scalar pair under either setting)
    long_t, short_t = n_new.get("attention_f16x2_kernel", 0), n_new.get("attention_kernel", 0)
    assert long_t >= 1 and n_new.get("dmd_attention_bwd_mfma", 0) == long_t and n_new.get("dmd_attention_bwd", 0) == short_t, n_new
    assert n_old.get("dmd_attention_bwd", 0) == long_t + short_t and "dmd_attention_bwd_mfma" not in n_old, n_old
    assert torch.equal(l_new, l_old) and all(bool(torch.isfinite(v).all()) for v in g_new.values())
    assert_training_parity(g_new, g_old)


@pytest.mark.gpu
def test_graphed_training_step_on_the_new_route_is_bitwise_the_eager_loop(monkeypatch):
    """the launches record into a hipGraph (no allocation, no synchronisation) and replay exactly the eager loop, in the manner of
    tests/test_offgrid_train.py"""
    from diamond_amd.train_graph import GraphedTrainStep

    monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", "1024")

    def setup():
        den = _device_denoiser()
        table = {}

        def randn_fn(shape):  # device-resident noise, the same at every step for both runs
            if shape not in table:
                table[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(len(table) + 99)).cuda()
            return table[shape]

        den.randn_fn = randn_fn
        return den, torch.optim.AdamW(den.parameters(), lr=3e-4, capturable=True), _device_batches(2)

    warm, steps = 2, 2
    den, opt, batches = setup()
    init = {k: v.detach().clone() for k, v in den.state_dict().items()}
    losses_e = []
    for i in range(warm + steps):
        loss, _ = den(batches[0] if i < warm else batches[i % 2])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(den.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if i >= warm:
            losses_e.append(loss.detach().clone())
    params_e = {k: v.detach().clone() for k, v in den.named_parameters()}

    den2, opt2, batches2 = setup()
    den2.load_state_dict(init)
    gstep = GraphedTrainStep(den2, opt2, 1.0, batches2[0], warmup_steps=warm)
    losses_g = [gstep(batches2[(warm + i) % 2])[0].clone() for i in range(steps)]
    torch.cuda.synchronize()
    assert len({float(x) for x in losses_g}) == steps, "the replayed step must see the new batch / the updated weights"
    assert all(torch.equal(a, b) for a, b in zip(losses_e, losses_g)), (losses_e, losses_g)
    assert max(float((p.detach() - params_e[k]).abs().max()) for k, p in den2.named_parameters()) == 0.0
    assert max(float((p.detach() - init[k]).abs().max()) for k, p in den2.named_parameters()) > 1e-4, "parameters did not train"
