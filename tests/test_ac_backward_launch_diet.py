"""The actor-critic encoder's backward with fewer launches: the end-of-backward reduction launch (dmd_wgrad_reduce_jobs) applies the
2^-k of the scaled backward as it writes (bitwise reduce-then-multiply), sums the GroupNorm parameter gradients in the same launch
(DMD_REDUCE_COLSUM: ascending n, fp64 accumulation), everything lands in ONE flat buffer, and the encoder's parameters reach the
graph through one bundle node (ac_native._ParamBundleFn) so that autograd adds one flat gradient per step instead of one per
parameter and step.  The kernel tests run on the GPU and, as their twin, on the SIMT interpreter (the same host code on CPU tensors)."""
import contextlib
import os

import pytest
import torch

SIMT, GPU = "simt", "gpu"
BOTH = [pytest.param(SIMT, id="simt"), pytest.param(GPU, marks=pytest.mark.gpu, id="gpu")]


def _backend(kind):
    if kind == GPU:
        return contextlib.nullcontext(), "cuda"
    from tests.simt.host_harness import engine_on_interpreter
    return engine_on_interpreter(), "cpu"


# ---- the reduction that scales ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,num_wg", [(6, 8, 3), (34, 16, 68)], ids=["direct-fp64", "sliced"])
@pytest.mark.parametrize("kind", BOTH)
def test_reduce_with_scale_is_bitwise_reduce_then_multiply(kind, n, hw, num_wg):
    """one 3x3 32 -> 32 job and one 1x1 32 -> 64 job, num_wg = 3 (few partials: summed directly in fp64) and 68 (> 4 * WGRAD_SLICES:
    fp32 slices, then fp64): the SAME partials reduced twice by one launch, without a scale and with 2^-7"""
    from diamond_amd import grad_ops as G
    from diamond_amd import native as nv
    from diamond_amd.engine import Act

    ctx, dev = _backend(kind)
    g = torch.Generator().manual_seed(n)
    scale = torch.tensor([2.0 ** -7], dtype=torch.float32, device=dev)
    with ctx:
        batch = G.WgradBatch()
        outs = []
        for cout, taps in ((32, 9), (64, 1)):
            k = 3 if taps == 9 else 1
            x = torch.randn(n, hw, hw, 32, generator=g).to(dev)
            dy = torch.randn(n, hw, hw, cout, generator=g).to(dev)
            mk = lambda: (torch.full((cout, 32, k, k), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev))
            (dw0, db0), (dw1, db1) = mk(), mk()
            G.wgrad(Act(x), nv.PROLOGUE_NONE, None, dy, taps, 32, split=False, batch=batch, dw_out=dw0, db_out=db0)
            job = batch.jobs[-1]
            assert job.num_wg == num_wg and not job.scale
            twin = nv.WgradReduceJob.from_buffer_copy(bytes(job))  # the same partials, other outputs, scaled
            twin.dw, twin.dbias, twin.scale = nv.ptr(dw1), nv.ptr(db1), nv.ptr(scale)
            batch.add(twin, dw1, db1)
            outs.append((dw0, db0, dw1, db1))
        assert len(batch.jobs) == 4
        batch.flush()
        for dw0, db0, dw1, db1 in outs:
            assert bool(torch.isfinite(dw0).all()) and bool(torch.isfinite(db0).all()) and float(dw0.abs().max()) > 0
            want = torch._foreach_mul([dw0, db0], scale[0])  # what the backward did before: one multiplication pass over the gradients
            assert torch.equal(dw1, want[0]) and torch.equal(db1, want[1])


# ---- GroupNorm parameter sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("n", [1, 37, 300])
@pytest.mark.parametrize("kind", BOTH)
def test_groupnorm_parameter_sums(kind, n, c):
    """dgamma / dbeta = the sums of dmd_gn_silu_bwd's per-(sample, channel) gradients over the batch, as jobs of the reduction launch:
    against a float64 sum no worse than torch's fp32 `sum(1)` of the same data (the kernel accumulates in fp64 and rounds once:
    the nearest fp32 to the exact sum up to fp64 rounding, which no fp32 summation order beats); two runs the same bits; the
    batch's scale applied."""
    from diamond_amd import grad_ops as G

    ctx, dev = _backend(kind)
    g = torch.Generator().manual_seed(n * 100 + c)
    # gradients of mixed sign and magnitude, like a batch with a few dominant samples
    dma = (torch.randn(2, n, c, generator=g) * torch.exp(3 * torch.randn(2, n, 1, generator=g))).to(dev)
    scale = torch.tensor([2.0 ** -5], dtype=torch.float32, device=dev)
    with ctx:
        runs = []
        for sc in (None, None, scale):
            batch = G.WgradBatch(sc)
            dgamma, dbeta = torch.full((c,), float("nan"), device=dev), torch.full((c,), float("nan"), device=dev)
            batch.add_colsum(dma, dgamma, dbeta)
            batch.flush()
            runs.append(torch.stack((dgamma, dbeta)))
        assert torch.equal(runs[0], runs[1])
        assert torch.equal(runs[2], runs[0] * scale[0])
        want = dma.double().sum(1)
        err_kernel = float((runs[0].double() - want).abs().max())
        err_torch = float((dma.sum(1).double() - want).abs().max())
        print(f"n={n} c={c}: max abs error kernel {err_kernel:.3e}, torch fp32 sum {err_torch:.3e}")
        assert err_kernel <= err_torch, (err_kernel, err_torch)
        # and never further than half an fp32 unit in the last place of the result (+ the fp64 accumulation's own rounding)
        half_ulp = torch.finfo(torch.float32).eps / 2 * want.abs().clamp_min(torch.finfo(torch.float32).tiny)
        assert bool(((runs[0].double() - want).abs() <= half_ulp * (1 + 1e-6)).all())


# ---- the parameter bundle -----------------------------------------------------------------------------------------------------------
def _window_grads(bundle: str, monkeypatch):
    """{start: {parameter: .grad}} of an ActorCritic window at B = 4, horizon 3, episode lengths staggered so that envs truncate
    inside the window (resets: the burn-in node and merge_slots take part), start = 'none' (.grad is None) and 'zeroed'; plus
    how often a post-accumulate hook on one encoder parameter fired per backward"""
    import random

    import diamond_amd as D
    from diamond_amd.actor_critic import actor_critic_loss
    from tests.test_gpu_models import _Loader, make_agent

    monkeypatch.setenv("DIAMOND_AC_GRAD_BUNDLE", bundle)
    monkeypatch.setenv("DIAMOND_ENV_LOOP", "slots")
    b, horizon, t = 4, 3, 3
    ag = make_agent()
    env = D.WorldModelEnv(ag.denoiser, ag.rew_end_model, _Loader(b, 77),
                          D.WorldModelEnvConfig(horizon=horizon, num_batches_to_preload=2,
                                                diffusion_sampler=D.DiffusionSamplerConfig(num_steps_denoising=2)))
    ac = ag.actor_critic
    ag.setup_training(D.SigmaDistributionConfig(-0.4, 1.2, 2e-3, 20),
                      D.ActorCriticLossConfig(backup_every=t, gamma=0.985, lambda_=0.95, weight_value_loss=1.0, weight_entropy_loss=0.001), env)
    torch.manual_seed(4321)
    random.seed(0)
    fired = []
    hooked = ac.encoder.encoder[0].weight
    handle = hooked.register_post_accumulate_grad_hook(lambda p: fired.append(1))
    out, hooks, resets = {}, {}, 0
    ac.env_loop.send(t)  # (a first window, never differentiated: episode lengths can be set once the env has a state)
    env.set_episode_lengths(torch.arange(b) % horizon)  # the next window truncates an env at every step
    for start in ("none", "zeroed"):
        if start == "none":
            ac.zero_grad(set_to_none=True)
        else:
            ac.zero_grad(set_to_none=False)
            assert all(p.grad is not None and float(p.grad.abs().max()) == 0 for p in ac.parameters())
        _, act, rew, end, trunc, logits_act, val, vb, _ = ac.env_loop.send(t)
        env.set_episode_lengths(torch.arange(b) % horizon)
        resets += int(end.sum() + trunc.sum())
        loss, _ = actor_critic_loss(logits_act, val, act, rew, end, trunc, vb, ac.loss_cfg)
        del fired[:]
        loss.backward()
        hooks[start] = len(fired)
        out[start] = {k: p.grad.detach().clone() for k, p in ac.named_parameters()}
    handle.remove()
    return out, hooks, resets, dict(env.stats)


@pytest.mark.gpu
def test_bundled_encoder_gradients_are_bitwise_the_per_parameter_ones(monkeypatch):
    on, hooks_on, resets, stats = _window_grads("1", monkeypatch)
    off, hooks_off, resets_off, _ = _window_grads("0", monkeypatch)
    assert resets == resets_off and resets > 0 and stats["dead_rows"] > 0, (resets, stats)  # the burn-in node and merge_slots took part
    for start in ("none", "zeroed"):
        assert set(on[start]) == set(off[start])
        for k, g in on[start].items():
            assert bool(torch.isfinite(g).all()), k
            assert torch.equal(g, off[start][k]), (start, k, float((g - off[start][k]).abs().max()))
        assert any(float(g.abs().max()) > 0 for k, g in on[start].items() if k.startswith("encoder."))
    assert hooks_on == {"none": 1, "zeroed": 1} and hooks_off == hooks_on, (hooks_on, hooks_off)


def test_bundled_encoder_gradients_interpreter(monkeypatch):
    """the twin without a GPU: two chained encoder passes of one graph (one bundle node, two _EncoderFn nodes), switch on and off"""
    import diamond_amd as D
    from diamond_amd.testing import fill_module_, synthetic_frames
    from tests.conftest import WEIGHT_SEED
    from tests.simt.host_harness import engine_on_interpreter

    grads, hooks = {}, {}
    for bundle in ("1", "0"):
        monkeypatch.setenv("DIAMOND_AC_GRAD_BUNDLE", bundle)
        ag = D.Agent(D.default_agent_config())
        fill_module_(ag, WEIGHT_SEED)
        ac = ag.actor_critic.eval()
        fired = []
        ac.encoder.encoder[0].weight.register_post_accumulate_grad_hook(lambda p: fired.append(1))
        g = torch.Generator().manual_seed(3)
        with engine_on_interpreter():
            a = ac.encode(synthetic_frames(g, 2, 3, 64, 64))
            b = ac.encode(synthetic_frames(g, 1, 3, 64, 64))
            assert (ac._native_encoder._bundle is not None) == (bundle == "1")
            (a.square().sum() + 3 * b.sum()).backward()
            assert ac._native_encoder._bundle is None
        grads[bundle] = {k: p.grad.clone() for k, p in ac.encoder.named_parameters()}
        hooks[bundle] = len(fired)
    assert hooks == {"1": 1, "0": 1}
    for k, g in grads["1"].items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        assert torch.equal(g, grads["0"][k]), k
