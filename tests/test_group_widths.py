"""Normalised widths that are NOT multiples of 32 channels (tests/group_width_configs.py): the reference forms max(1, C // 32)
GroupNorm groups of C / groups channels (models/blocks.py:27,38) -- 16, 48, 40 and 36 channels at C = 16, 48, 80 and 144 -- and
its U-Net's up path normalises concatenations whose 32-channel groups straddle the two sources.  The kernels' general-group
instances (ConvGeomGN, WgradGeomGN, gn_stats_any_kernel, gn_bwd_fused_kernel) and the host's materialised concatenation
(engine.concat) are held against fp64 torch (kernel level) and against fixtures produced by EXECUTING THE REFERENCE on the same
configurations (tests/golden/make_golden_groups.py -> tests/golden/groups.pt) at the bars of the default configuration's tests.

Every test runs on the SIMT-interpreter build of the kernels (the CPU suite) and on the device (`-m gpu`)."""
import contextlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import group_width_configs as W
from tests.simt.host_harness import engine_on_interpreter

GOLD = os.path.join(os.path.dirname(__file__), "golden", "groups.pt")
BACKENDS = ["interpreter", pytest.param("cuda", marks=[pytest.mark.gpu])]


def _backend(kind):
    """(context manager under which the product's host code runs, device of the tensors)"""
    return (engine_on_interpreter(), "cpu") if kind == "interpreter" else (contextlib.nullcontext(), "cuda")


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=False)


def _gn_ref(x_nhwc, gamma, beta, silu=True):
    """fp64 GroupNorm(max(1, C // 32) groups) + affine (+ SiLU) of an NHWC tensor, NCHW out"""
    c = x_nhwc.shape[-1]
    y = F.group_norm(x_nhwc.double().permute(0, 3, 1, 2), max(1, c // 32), gamma.double(), beta.double(), eps=1e-5)
    return F.silu(y) if silu else y


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 48, 80, 144])
@pytest.mark.parametrize("backend", BACKENDS)
def test_group_statistics_vs_fp64(c, backend):
    """dmd_gn_stats / dmd_gn_stats_valid on the general groups: per-(image, group) sums and sums of squares"""
    from diamond_amd import engine as E

    g = torch.Generator().manual_seed(c)
    x = torch.randn(2, 8, 16, c, generator=g) * 2 + 0.5
    G = max(1, c // 32)
    ctx, dev = _backend(backend)
    with ctx:
        plain = E.gn_stats(x.to(dev)).stats.cpu()
        valid = E.gn_stats(x.to(dev), (5, 11)).stats.cpu()
    assert plain.shape == (2, G, 1, 2)
    for st, xs in ((plain, x), (valid, x[:, :5, :11])):
        want = xs.double().reshape(2, -1, G, c // G).permute(0, 2, 1, 3).reshape(2, G, -1)
        assert rel(st[:, :, 0, 0], want.sum(-1)) < 1e-12 and rel(st[:, :, 0, 1], want.square().sum(-1)) < 1e-12


@pytest.mark.parametrize("c", [16, 48, 80, 144])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_conv_normalised_source_and_residual_vs_fp64(c, precision, backend):
    """the generic convolution's general-group instances: GroupNorm + affine + SiLU of a c-channel source in the load path,
    GroupNorm + affine of a c-channel residual in the epilogue (the attention's x_normed + out_proj(y)), and the statistics of
    the c-channel output (dmd_gn_stats behind the launch)"""
    from diamond_amd import engine as E
    from diamond_amd import native as nv
    from diamond_amd.engine import Act, NormSpec

    g = torch.Generator().manual_seed(100 + c)
    n, h, w = 2, 8, 16
    x = torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3
    res = torch.randn(n, h, w, c, generator=g) - 0.2
    gamma, beta = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    rg, rb = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    bias = torch.randn(c, generator=g) * 0.1
    ref = F.conv2d(_gn_ref(x, gamma, beta), wt.double(), bias.double(), padding=1) + _gn_ref(res, rg, rb, silu=False)
    ctx, dev = _backend(backend)
    on = lambda t: t.contiguous().to(dev)
    with ctx:
        out = E.conv2d([(E.gn_stats(on(x)), nv.PROLOGUE_NORM_SILU, NormSpec(mul=on(gamma), add=on(beta)))], nv.pack_conv_weight(on(wt)),
                       on(bias), c, residual=E.gn_stats(on(res)), residual_norm=NormSpec(mul=on(rg), add=on(rb)),
                       fast_math=precision == "f16x2")
    got = out.t.cpu().double().permute(0, 3, 1, 2)
    assert rel(got, ref) < (2e-6 if precision == "f32" else 2e-5), rel(got, ref)
    G = max(1, c // 32)
    sums = out.stats.cpu().sum(2)
    want = ref.reshape(n, G, -1)
    assert rel(sums[..., 0], want.sum(-1)) < 1e-5 and rel(sums[..., 1], want.square().sum(-1)) < 1e-5


@pytest.mark.parametrize("backend", BACKENDS)
def test_straddling_concatenation_80_144_vs_fp64(backend):
    """cat(x 80, skip 144): the reference normalises the 224 channels in 7 groups of 32, the third of which spans both sources --
    engine.concat materialises the concatenation with its own statistics and the convolution normalises it as one source"""
    from diamond_amd import engine as E
    from diamond_amd import native as nv
    from diamond_amd.engine import Act, NormSpec

    g = torch.Generator().manual_seed(7)
    n, h, w = 2, 8, 8
    a, b = torch.randn(n, h, w, 80, generator=g) + 1.0, torch.randn(n, h, w, 144, generator=g) * 3 - 0.5
    gamma, beta = torch.randn(224, generator=g) * 0.3 + 1, torch.randn(224, generator=g) * 0.2
    wt = torch.randn(48, 224, 3, 3, generator=g) / (9 * 224) ** 0.5
    ref = F.conv2d(_gn_ref(torch.cat([a, b], -1), gamma, beta), wt.double(), padding=1)
    ctx, dev = _backend(backend)
    on = lambda t: t.contiguous().to(dev)
    with ctx:
        xs = [E.gn_stats(on(a)), E.gn_stats(on(b))]
        assert E.straddles(xs)
        cat = E.concat(xs)
        out = E.conv2d([(cat, nv.PROLOGUE_NORM_SILU, NormSpec(mul=on(gamma), add=on(beta)))], nv.pack_conv_weight(on(wt)), None, 48)
    assert rel(out.t.cpu().double().permute(0, 3, 1, 2), ref) < 2e-6


@pytest.mark.parametrize("c", [16, 48, 80, 144])
@pytest.mark.parametrize("valid", [False, True])
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("backend", BACKENDS)
def test_groupnorm_silu_backward_vs_fp64(c, valid, film, backend):
    """dmd_gn_silu_bwd on the general groups: dx (+ the skip gradient), d mul, d add of GroupNorm + affine (nn.GroupNorm) or
    GroupNorm + FiLM (AdaGroupNorm: y = xn * (1 + scale) + shift) + SiLU, with and without a valid extent, against autograd in fp64"""
    from diamond_amd import engine as E
    from diamond_amd.grad_ops import gn_bwd
    from diamond_amd.engine import NormSpec

    g = torch.Generator().manual_seed(300 + c)
    n, h, w = 2, 16, 16
    vh, vw = (11, 13) if valid else (h, w)
    x = torch.randn(n, h, w, c, generator=g) * 1.3 + 0.2
    da = torch.randn(n, h, w, c, generator=g)
    dskip = torch.randn(n, h, w, c, generator=g)
    if film:
        mul, add = torch.randn(n, c, generator=g) * 0.3, torch.randn(n, c, generator=g) * 0.2
    else:
        mul, add = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    # fp64 autograd over the valid part
    xv = x[:, :vh, :vw].double().permute(0, 3, 1, 2).requires_grad_()
    mv, av = mul.double().requires_grad_(), add.double().requires_grad_()
    xn = F.group_norm(xv, max(1, c // 32), eps=1e-5)
    y = F.silu(xn * (1 + mv[:, :, None, None]) + av[:, :, None, None] if film else xn * mv[None, :, None, None] + av[None, :, None, None])
    y.backward(da[:, :vh, :vw].double().permute(0, 3, 1, 2))
    ctx, dev = _backend(backend)
    on = lambda t: t.contiguous().to(dev)
    with ctx:
        xa = E.gn_stats(on(x), (vh, vw) if valid else None)
        spec = NormSpec(mul=on(mul), add=on(add), mul_stride=c if film else 0, add_stride=c if film else 0, plus_one=film)
        dx, (dmul, dadd) = gn_bwd(xa, spec, on(da), on(dskip))
    dx = dx.cpu().double()
    assert rel(dx[:, :vh, :vw], xv.grad.permute(0, 2, 3, 1) + dskip[:, :vh, :vw].double()) < 1e-5
    if valid:
        assert float(dx[:, vh:].abs().max()) == 0.0 and float(dx[:, :, vw:].abs().max()) == 0.0
    dm, dd = dmul.cpu().double(), dadd.cpu().double()
    assert rel(dm if film else dm.sum(0), mv.grad) < 1e-5 and rel(dd if film else dd.sum(0), av.grad) < 1e-5


@pytest.mark.parametrize("c", [16, 48, 80, 144])
@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("backend", BACKENDS)
def test_weight_gradient_normalised_source_vs_fp64(c, taps, split, backend):
    """dmd_conv2d_wgrad's general-group instances (one whole group per launch, WgradGeomGN): the GroupNorm + affine + SiLU of the
    source recomputed while staging, dW and db against fp64 torch"""
    from diamond_amd import engine as E
    from diamond_amd.grad_ops import wgrad
    from diamond_amd import native as nv
    from diamond_amd.engine import NormSpec

    g = torch.Generator().manual_seed(500 + c + taps)
    n, h, w, cout = 2, 8, 16, 48
    k = 3 if taps == 9 else 1
    x = torch.randn(n, h, w, c, generator=g) * 1.2 + 0.4
    gamma, beta = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.2
    dy = torch.randn(n, h, w, cout, generator=g)
    xin = _gn_ref(x, gamma, beta).requires_grad_()
    wt = torch.zeros(cout, c, k, k, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, wt, bt, padding=k // 2).backward(dy.double().permute(0, 3, 1, 2))
    ctx, dev = _backend(backend)
    on = lambda t: t.contiguous().to(dev)
    with ctx:
        dw, db = wgrad(E.gn_stats(on(x)), nv.PROLOGUE_NORM_SILU, NormSpec(mul=on(gamma), add=on(beta)), on(dy), taps, c, split=split)
    tol = 2e-5 if split else 2e-6
    assert rel(dw.cpu(), wt.grad) < tol and rel(db.cpu(), bt.grad) < tol, (rel(dw.cpu(), wt.grad), rel(db.cpu(), bt.grad))


# ---------------------------------------------------------------------------------------------------------------------------
# networks against the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _denoiser():
    import diamond_amd as D
    from diamond_amd.inner_model import InnerModelConfig
    from diamond_amd.testing import fill_module_

    den = D.Denoiser(D.DenoiserConfig(inner_model=InnerModelConfig(**W.DENOISER), sigma_data=0.5, sigma_offset_noise=0.3))
    fill_module_(den, W.WEIGHT_SEED)
    return den


@pytest.mark.parametrize("backend", BACKENDS)
def test_group_width_denoiser_model_output_vs_reference_golden(gold, backend):
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    ctx, dev = _backend(backend)
    den = _denoiser().eval().to(dev)
    s = W.SIZE
    g = torch.Generator().manual_seed(5)
    obs, act, x = synthetic_frames(g, 2, 12, s, s).to(dev), synthetic_actions(g, 4, 2, 4).to(dev), torch.randn(2, 3, s, s, generator=g).to(dev)
    with ctx, torch.no_grad():
        for i, sigma in enumerate((torch.tensor(0.7), torch.tensor([0.05, 3.0]))):
            f = den.compute_model_output(x, obs, act, sigma.to(dev)).cpu()
            err = rel(f, gold[f"model_output_{i}"])
            assert err < 1e-4, (i, err)


def _denoiser_batch(dev):
    from types import SimpleNamespace

    from diamond_amd.testing import synthetic_actions, synthetic_frames

    s = W.SIZE
    g = torch.Generator().manual_seed(31)
    obs, act = synthetic_frames(g, 1, 5, 3, s, s).to(dev), synthetic_actions(g, 4, 1, 5).to(dev)
    return SimpleNamespace(obs=obs, act=act, mask_padding=torch.ones(1, 5, dtype=torch.bool).to(dev))


def _grad_errors(module, ref):
    errs = {}
    for k, p in module.named_parameters():
        assert p.grad is not None, f"no gradient for {k}"
        errs["grad " + k] = rel(W.sample_grad(p.grad).cpu(), ref["grads"][k])
        nrm = float(ref["grad_norms"][k])
        errs["|grad| " + k] = abs(float(p.grad.double().norm()) - nrm) / (nrm + 1e-30)
    return errs


@pytest.mark.parametrize("backend", BACKENDS)
def test_group_width_denoiser_training_step_vs_reference_golden(gold, backend):
    """Denoiser.forward + loss.backward() (the recorded forward with its materialised concatenations + the hand-written backward):
    loss and every gradient against the reference's autograd; split-fp16, and exact fp32 on the device"""
    import diamond_amd as D
    from diamond_amd import unet_train as UT

    ctx, dev = _backend(backend)
    den = _denoiser().train().to(dev)
    den.setup_training(D.SigmaDistributionConfig(**W.SIGMA_DIST))
    batch = _denoiser_batch(dev)
    den.randn_fn = lambda shape: torch.randn(*shape)  # CPU default generator: the stream the reference consumed
    ref = gold["train"]
    try:
        both = backend != "interpreter" or os.environ.get("DIAMOND_SLOW_CPU_TESTS") == "1"
        for precision in ("f16x2", "f32") if both else ("f16x2",):
            UT.TRAIN_PRECISION = precision
            with _backend(backend)[0]:
                torch.manual_seed(77)
                den.zero_grad()
                loss, _ = den(batch)
                loss.backward()
            errs = {"loss": rel(loss.detach().cpu(), ref["loss"]), **_grad_errors(den, ref)}
            bad = {k: v for k, v in errs.items() if v >= 1e-4}
            assert not bad, (precision, bad)
    finally:
        UT.TRAIN_PRECISION = "f16x2"


@pytest.mark.parametrize("backend", BACKENDS)
def test_group_width_rew_end_model_vs_reference_golden(gold, backend):
    """RewEndModel.predict_rew_end and RewEndModel.forward + loss.backward() on 16 / 48 / 80-channel levels"""
    from types import SimpleNamespace

    from diamond_amd.rew_end_model import RewEndModel, RewEndModelConfig
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames

    s = W.SIZE
    ctx, dev = _backend(backend)
    m = RewEndModel(RewEndModelConfig(**W.REW_END))
    fill_module_(m, W.WEIGHT_SEED + 1)
    m.eval().to(dev)
    g = torch.Generator().manual_seed(9)
    obs, act = synthetic_frames(g, 2, 3, 3, s, s).to(dev), synthetic_actions(g, 4, 2, 2).to(dev)
    with ctx, torch.no_grad():
        lr, le, (h, c) = [t.cpu() if torch.is_tensor(t) else tuple(u.cpu() for u in t) for t in m.predict_rew_end(obs[:, :-1], act, obs[:, 1:])]
    r = gold["rew_end"]
    errs = {"logits_rew": rel(lr, r["logits_rew"]), "logits_end": rel(le, r["logits_end"]), "h": rel(h, r["h"]), "c": rel(c, r["c"])}
    assert max(errs.values()) < 1e-4, errs

    m.train()
    d = W.rew_end_train_batch(torch.Generator().manual_seed(41))
    batch = SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()})
    if dev != "cpu":
        batch.info[1]["final_observation"] = batch.info[1]["final_observation"].to(dev)
    r = gold["rew_end_train"]
    with _backend(backend)[0]:
        m.zero_grad()
        loss, logs = m(batch)
        loss.backward()
    errs = {"loss": rel(loss.detach().cpu(), r["loss"]), "loss_rew": rel(logs["loss_rew"].cpu(), r["loss_rew"]),
            "loss_end": rel(logs["loss_end"].cpu(), r["loss_end"]), **_grad_errors(m, r)}
    bad = {k: v for k, v in errs.items() if v >= 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("backend", BACKENDS)
def test_group_width_actor_critic_vs_reference_golden(gold, backend):
    """ActorCritic.predict_act_value + backward on a 16 / 48 / 80 / 144-channel encoder"""
    from diamond_amd.actor_critic import ActorCritic, ActorCriticConfig
    from diamond_amd.testing import fill_module_, synthetic_frames

    s = W.SIZE
    ctx, dev = _backend(backend)
    ac = ActorCritic(ActorCriticConfig(**W.ACTOR_CRITIC))
    fill_module_(ac, W.WEIGHT_SEED + 2)
    ac.to(dev)
    g = torch.Generator().manual_seed(11)
    obs = synthetic_frames(g, 2, 3, s, s).to(dev)
    with ctx:
        o = ac.predict_act_value(obs, None)
        (o.logits_act.square().sum() + o.val.sum()).backward()
    r = gold["actor_critic"]
    errs = {"logits": rel(o.logits_act.detach().cpu(), r["logits"]), "val": rel(o.val.detach().cpu(), r["val"]), **_grad_errors(ac, r)}
    bad = {k: v for k, v in errs.items() if v >= 1e-4}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# widths outside the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels,rule", [([64, 48], "do not divide 112 channels"),  # up path: cat(64, 48), 3 groups of 112
                                           ([40, 80], "C % 16 == 0"),
                                           ([64, 272], "C <= 256 unless C % 32 == 0")])
def test_widths_outside_the_rule_raise_at_construction(channels, rule):
    import diamond_amd as D
    from diamond_amd.inner_model import InnerModelConfig

    cfg = dict(W.DENOISER, channels=channels, depths=[1, 1], attn_depths=[0, 0])
    with pytest.raises(ValueError, match=re.escape(rule)):
        D.Denoiser(D.DenoiserConfig(inner_model=InnerModelConfig(**cfg), sigma_data=0.5, sigma_offset_noise=0.3))


# ---------------------------------------------------------------------------------------------------------------------------
# device only: the imagination loop and the captured training step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_width_imagined_window_slots_is_bitwise_the_sequential_one(monkeypatch):
    """WorldModelEnv + make_env_loop on the three networks of group_width_configs: two imagined windows with the deaths resolved
    on the device (the default slots loop) and in the reference's order (DIAMOND_ENV_LOOP=sequential), every output bitwise equal"""
    import random

    import diamond_amd as D
    from diamond_amd.actor_critic import ActorCriticConfig
    from diamond_amd.inner_model import InnerModelConfig
    from diamond_amd.rew_end_model import RewEndModelConfig
    from diamond_amd.testing import fill_module_
    from tests.test_gpu_models import _Loader

    b, t = 4, 4
    runs = []
    for mode in ("slots", "sequential"):
        monkeypatch.setenv("DIAMOND_ENV_LOOP", mode)
        ag = D.Agent(W.agent_config(D.AgentConfig, D.DenoiserConfig, InnerModelConfig, RewEndModelConfig, ActorCriticConfig))
        fill_module_(ag, W.WEIGHT_SEED)
        ag = ag.to("cuda").eval()
        env = D.WorldModelEnv(ag.denoiser, ag.rew_end_model, _Loader(b, 77, size=W.SIZE),
                              D.WorldModelEnvConfig(horizon=5, num_batches_to_preload=2,
                                                    diffusion_sampler=D.DiffusionSamplerConfig(num_steps_denoising=2)))
        ag.setup_training(D.SigmaDistributionConfig(**W.SIGMA_DIST),
                          D.ActorCriticLossConfig(backup_every=t, gamma=0.985, lambda_=0.95, weight_value_loss=1.0,
                                                  weight_entropy_loss=0.001), env)
        torch.manual_seed(4321)
        random.seed(0)
        outs = []
        for _ in range(2):
            res = ag.actor_critic.env_loop.send(t)
            outs.append([x.detach().cpu() for x in res[:8]])
        runs.append(outs)
    names = ("obs", "act", "rew", "end", "trunc", "logits", "val", "val_bootstrap")
    for w, (wa, wb) in enumerate(zip(*runs)):
        for name, a, b_ in zip(names, wa, wb):
            assert torch.equal(a, b_), (w, name)


@pytest.mark.gpu
def test_group_width_graphed_training_step_matches_eager():
    """the denoiser's training step (its concatenations materialised inside the capture) as one replayed hipGraph
    (train_graph.GraphedTrainStep) against the eager loop on the same batches and noise, at the bars of
    tests/test_gpu_train_graph.py"""
    from types import SimpleNamespace

    import diamond_amd as D
    from diamond_amd.testing import synthetic_actions, synthetic_frames
    from diamond_amd.train_graph import GraphedTrainStep

    def setup():
        den = _denoiser().to("cuda").train()
        den.setup_training(D.SigmaDistributionConfig(**W.SIGMA_DIST))
        g = torch.Generator().manual_seed(5)
        batches = [SimpleNamespace(obs=synthetic_frames(g, 2, 5, 3, W.SIZE, W.SIZE).cuda(), act=synthetic_actions(g, 4, 2, 5).cuda(),
                                   mask_padding=torch.ones(2, 5, dtype=torch.bool).cuda()) for _ in range(3)]
        table = {}

        def randn_fn(shape):  # device-resident noise: the same at every step for both runs
            if shape not in table:
                table[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(len(table) + 99)).cuda()
            return table[shape]

        den.randn_fn = randn_fn
        return den, torch.optim.AdamW(den.parameters(), lr=3e-4, capturable=True, fused=True), batches

    warm, steps = 2, 3
    den, opt, batches = setup()
    init = {k: v.detach().clone() for k, v in den.state_dict().items()}
    losses_e = []
    for i in range(warm + steps):
        loss, _ = den(batches[0] if i < warm else batches[(i - warm) % 3])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(den.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if i >= warm:
            losses_e.append(float(loss.detach()))
    params_e = {k: v.detach().clone() for k, v in den.named_parameters()}
    den2, opt2, batches2 = setup()
    den2.load_state_dict(init)
    gstep = GraphedTrainStep(den2, opt2, 1.0, batches2[0], warmup_steps=warm)
    losses_g = [float(gstep(batches2[i % 3])[0]) for i in range(steps)]
    torch.cuda.synchronize()
    assert len(set(losses_g)) == steps, "the replayed step must see the new batch / the updated weights"
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-6 * abs(a), (losses_e, losses_g)
    worst = max(float((p.detach() - params_e[k]).abs().max() / params_e[k].abs().max().clamp_min(1e-12)) for k, p in den2.named_parameters())
    assert worst < 1e-5, worst
