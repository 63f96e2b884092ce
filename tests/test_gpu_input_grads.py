"""Image gradients of the three networks on the device: autograd reaches `noisy_next_obs` / `obs` of the denoiser, `obs` of the
policy and the frames of the reward / end model through grad_ops.dgrad_input (dmd_conv2d_dgrad_input, one launch per backward),
and nothing changes where no input requires a gradient.

Reference: the float64 autograd of the oracle's functional restatement (oracle.diamond_oracle.model_output / ac_predict /
rew_end_predict, pinned to the reference by tests/test_oracle_golden.py) on the same weights (diamond_amd.testing.fill_module_),
inputs and a fixed random cotangent.  Measure and bar: rel_err = max |err| / max |ref| <= 1e-4, what tests/test_gpu_models.py
applies to every parameter gradient."""
from types import SimpleNamespace

import pytest
import torch

from tests.conftest import WEIGHT_SEED
from tests.test_gpu_models import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4


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


def work_launches(counter):
    """launches per key without the pack cache's housekeeping (the first use of a module packs its weights; an audit of the packed
    copies comes round every few thousand lookups): what a forward and backward themselves launch"""
    return {k: v for k, v in counter.n.items() if k not in ("dmd_pack_jobs", "dmd_checksums")}


def _agent(img_size=64):
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    agent = D.Agent(D.default_agent_config(img_size=img_size))
    fill_module_(agent, WEIGHT_SEED)
    return agent.to(DEV).eval()


def _sd64(module):
    return {k: v.detach().double().cpu() for k, v in module.state_dict().items()}


@pytest.fixture(scope="module")
def agents():
    return {64: _agent(64), 72: _agent(72)}


# ---- denoiser ----------------------------------------------------------------------------------------------------------------------
def _denoiser_case(size, b=2, channels=12, seed=41):
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    g = torch.Generator().manual_seed(seed + size)
    obs = synthetic_frames(g, b, channels, size, size)
    act = synthetic_actions(g, 4, b, 4)
    noisy = torch.randn(b, 3, size, size, generator=g)
    sigma = torch.tensor([5.0, 0.3])[:b]
    cot = torch.randn(b, 3, size, size, generator=g)
    return noisy, obs, act, sigma, cot


def _denoiser_reference(den, spec, noisy, obs, act, sigma, cot):
    from oracle import diamond_oracle as O

    n64, o64 = noisy.double().requires_grad_(True), obs.double().requires_grad_(True)
    out = O.model_output(_sd64(den), spec, n64, sigma.double(), o64, act)
    return torch.autograd.grad((out * cot.double()).sum(), [n64, o64])


def _denoiser_grads(den, noisy, obs, act, sigma, cot, precision, want=(True, True)):
    x = noisy.to(DEV).requires_grad_(want[0])
    o = obs.to(DEV).requires_grad_(want[1])
    out = den.model_output_with_grad(x, o, act.to(DEV), den._training_conditioners(sigma.to(DEV)), precision=precision)
    (out * cot.to(DEV)).sum().backward()
    return out.detach(), x.grad, o.grad


@pytest.mark.parametrize("size", [64, 72])
def test_denoiser_image_gradients_vs_float64_oracle(agents, size):
    from oracle import diamond_oracle as O

    den = agents[size].denoiser
    noisy, obs, act, sigma, cot = _denoiser_case(size)
    ref_noisy, ref_obs = _denoiser_reference(den, O.DenoiserSpec(), noisy, obs, act, sigma, cot)
    for precision in ("f16x2", "f32"):
        den.zero_grad(set_to_none=True)
        _, g_noisy, g_obs = _denoiser_grads(den, noisy, obs, act, sigma, cot, precision)
        # the assertion that cannot pass without the feature: the gradients exist
        assert g_noisy is not None and g_obs is not None, "autograd did not reach the images"
        assert g_noisy.shape == noisy.shape and g_obs.shape == obs.shape
        e = (rel_err(g_noisy, ref_noisy), rel_err(g_obs, ref_obs))
        print(f"denoiser {size}x{size} [{precision}]: grad(noisy) {e[0]:.2e} grad(obs) {e[1]:.2e}")
        assert max(e) <= BAR, e


def test_denoiser_one_image_alone(agents):
    """only `obs` (only `noisy`) requires a gradient: the other one gets none, the wanted one the same bits"""
    den = agents[64].denoiser
    case = _denoiser_case(64)
    _, g_noisy, g_obs = _denoiser_grads(den, *case, "f16x2")
    _, a, b = _denoiser_grads(den, *case, "f16x2", want=(True, False))
    assert b is None and torch.equal(a, g_noisy)
    _, a, b = _denoiser_grads(den, *case, "f16x2", want=(False, True))
    assert a is None and torch.equal(b, g_obs)


def test_wide_first_layer_denoiser_image_gradients():
    """a first convolution of 96 output channels (tests/wide_configs.py's denoiser with its first level widened) at 32x32: the
    same kernel contracts over two chunks of output channels"""
    import diamond_amd as D
    from diamond_amd.inner_model import InnerModelConfig
    from diamond_amd.testing import fill_module_
    from oracle import diamond_oracle as O
    from tests import wide_configs as W

    cfg = dict(W.DENOISER, channels=[96, 160, 320])
    den = D.Denoiser(D.DenoiserConfig(inner_model=InnerModelConfig(**cfg), sigma_data=0.5, sigma_offset_noise=0.3))
    fill_module_(den, W.WEIGHT_SEED)
    den = den.to(DEV).eval()
    assert den.inner_model.conv_in.out_channels == 96
    spec = O.DenoiserSpec(depths=tuple(cfg["depths"]), channels=tuple(cfg["channels"]), attn_depths=tuple(cfg["attn_depths"]))
    noisy, obs, act, sigma, cot = _denoiser_case(W.SIZE)
    ref_noisy, ref_obs = _denoiser_reference(den, spec, noisy, obs, act, sigma, cot)
    _, g_noisy, g_obs = _denoiser_grads(den, noisy, obs, act, sigma, cot, "f32")
    assert g_noisy is not None and g_obs is not None
    e = (rel_err(g_noisy, ref_noisy), rel_err(g_obs, ref_obs))
    print(f"wide denoiser 32x32 [f32]: grad(noisy) {e[0]:.2e} grad(obs) {e[1]:.2e}")
    assert max(e) <= BAR, e


# ---- actor-critic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bundle", ["1", "0"])
@pytest.mark.parametrize("precision", ["f16x2", "f32"])
@pytest.mark.parametrize("size", [64, 72])
def test_policy_image_gradient_vs_float64_oracle(agents, monkeypatch, size, precision, bundle):
    from diamond_amd import ac_native
    from diamond_amd.testing import synthetic_frames
    from oracle import diamond_oracle as O

    monkeypatch.setattr(ac_native, "AC_PRECISION", precision)
    monkeypatch.setenv("DIAMOND_AC_GRAD_BUNDLE", bundle)
    ac = agents[size].actor_critic
    g = torch.Generator().manual_seed(7 + size)
    b = 2
    obs = synthetic_frames(g, b, 3, size, size)
    hx, cx = torch.randn(b, 512, generator=g) * 0.3, torch.randn(b, 512, generator=g) * 0.3
    cot_l, cot_v = torch.randn(b, 4, generator=g), torch.randn(b, generator=g)

    o64 = obs.double().requires_grad_(True)
    logits, val, _ = O.ac_predict(_sd64(ac), O.ActorCriticSpec(img_size=size), o64, hx.double(), cx.double())
    ((logits * cot_l.double()).sum() + (val * cot_v.double()).sum()).backward()

    ac.zero_grad(set_to_none=True)
    o = obs.to(DEV).requires_grad_(True)
    out = ac.predict_act_value(o, (hx.to(DEV), cx.to(DEV)))
    ((out.logits_act * cot_l.to(DEV)).sum() + (out.val.reshape(b) * cot_v.to(DEV)).sum()).backward()
    assert o.grad is not None and o.grad.shape == obs.shape, "autograd did not reach the policy's observation"
    assert all(p.grad is not None for p in ac.encoder.parameters())
    e = rel_err(o.grad, o64.grad)
    print(f"actor-critic {size}x{size} [{precision}, bundle {bundle}]: obs.grad {e:.2e}")
    assert e <= BAR, e


# ---- reward / end model ------------------------------------------------------------------------------------------------------------
def test_rew_end_frame_gradients_vs_float64_oracle(agents):
    from diamond_amd.testing import synthetic_actions, synthetic_frames
    from oracle import diamond_oracle as O

    m = agents[64].rew_end_model
    g = torch.Generator().manual_seed(19)
    b, t = 2, 3
    frames = synthetic_frames(g, b, t + 1, 3, 64, 64)
    act = synthetic_actions(g, 4, b, t)
    cot = torch.randn(b, t, 5, generator=g)

    o64, n64 = frames[:, :-1].double().requires_grad_(True), frames[:, 1:].double().requires_grad_(True)
    lr, le, _ = O.rew_end_predict(_sd64(m), O.RewEndSpec(), o64, act, n64)
    (torch.cat((lr, le), dim=-1) * cot.double()).sum().backward()

    got = {}
    for segment in (False, True):
        m.zero_grad(set_to_none=True)
        o = frames[:, :-1].to(DEV).contiguous().requires_grad_(True)
        n = frames[:, 1:].to(DEV).contiguous().requires_grad_(True)
        logits = m.logits_with_grad(o, act.to(DEV), n, segment=segment)
        (logits * cot.to(DEV)).sum().backward()
        assert o.grad is not None and n.grad is not None, "autograd did not reach the frames"
        assert o.grad.shape == o.shape and n.grad.shape == n.shape
        got[segment] = (o.grad, n.grad)
        e = (rel_err(o.grad, o64.grad), rel_err(n.grad, n64.grad))
        print(f"rew/end B=2 T=3 [segment={segment}]: grad(obs) {e[0]:.2e} grad(next_obs) {e[1]:.2e}")
        assert max(e) <= BAR, e
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])


# ---- nothing changes where no image requires a gradient ----------------------------------------------------------------------------
def test_denoiser_unused_path_is_unchanged_and_the_used_one_adds_one_launch(agents, monkeypatch):
    from diamond_amd import native as nv

    den = agents[64].denoiser
    case = _denoiser_case(64)
    runs = {}
    _denoiser_grads(den, *case, "f16x2", want=(False, False))  # (the packed weights exist from here on)
    for want in (False, True):
        den.zero_grad(set_to_none=True)
        counter = _Counter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        out, g_noisy, g_obs = _denoiser_grads(den, *case, "f16x2", want=(want, want))
        monkeypatch.setattr(nv, "PROFILER", None)
        runs[want] = (out, {k: p.grad.clone() for k, p in den.named_parameters() if p.grad is not None}, work_launches(counter))
        assert (g_noisy is not None) == want and (g_obs is not None) == want
    (out0, grads0, n0), (out1, grads1, n1) = runs[False], runs[True]
    assert torch.equal(out0, out1)
    assert grads0.keys() == grads1.keys() and len(grads0) > 100 and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
    assert "dgrad_input_kernel" not in n0 and n1.get("dgrad_input_kernel") == 1, (n0, n1)
    assert sum(n1.values()) == sum(n0.values()) + 1 and {k: v for k, v in n1.items() if k != "dgrad_input_kernel"} == n0


def test_policy_unused_path_is_unchanged_and_the_used_one_adds_one_launch(agents, monkeypatch):
    from diamond_amd import native as nv
    from diamond_amd.testing import synthetic_frames

    ac = agents[64].actor_critic
    g = torch.Generator().manual_seed(3)
    obs = synthetic_frames(g, 2, 3, 64, 64).to(DEV)
    cot = torch.randn(2, 4, generator=g).to(DEV)
    runs = {}
    for want in (None, False, True):  # (None: a first pass, after which the packed weights exist)
        ac.zero_grad(set_to_none=True)
        counter = _Counter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        o = obs.clone().requires_grad_(bool(want))
        out = ac.predict_act_value(o, None)
        ((out.logits_act * cot).sum() + out.val.sum()).backward()
        monkeypatch.setattr(nv, "PROFILER", None)
        if want is None:
            continue
        runs[want] = (out.logits_act.detach(), {k: p.grad.clone() for k, p in ac.named_parameters()}, work_launches(counter))
        assert (o.grad is not None) == want
    (out0, grads0, n0), (out1, grads1, n1) = runs[False], runs[True]
    assert torch.equal(out0, out1) and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
    assert sum(n1.values()) == sum(n0.values()) + 1 and n1.get("dgrad_input_kernel") == 1 and "dgrad_input_kernel" not in n0, (n0, n1)


def test_graphed_training_step_without_image_gradients_replays_the_eager_loop_bitwise():
    """a training batch's frames require no gradient: the captured step holds no image-gradient launch and replays exactly the
    eager loop (the manner of tests/test_offgrid_train.py), B = 2 at 64x64"""
    import diamond_amd as D
    from diamond_amd import native as nv
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames
    from diamond_amd.train_graph import GraphedTrainStep

    def setup():
        agent = D.Agent(D.default_agent_config())
        fill_module_(agent, WEIGHT_SEED)
        den = agent.to(DEV).eval().denoiser
        den.train()
        den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
        table = {}

        def randn_fn(shape):  # device-resident noise, the same at every step for both runs
            if shape not in table:
                table[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(len(table) + 99)).cuda()
            return table[shape]

        den.randn_fn = randn_fn
        g = torch.Generator().manual_seed(8)
        batches = [SimpleNamespace(obs=synthetic_frames(g, 2, 5, 3, 64, 64).cuda(), act=synthetic_actions(g, 4, 2, 5).cuda(),
                                   mask_padding=torch.ones(2, 5, dtype=torch.bool).cuda()) for _ in range(2)]
        return den, torch.optim.AdamW(den.parameters(), lr=3e-4, capturable=True), batches

    warm, steps = 2, 2
    den, opt, batches = setup()
    init = {k: v.detach().clone() for k, v in den.state_dict().items()}
    losses_e = []
    counter = _Counter()
    for i in range(warm + steps):
        nv.PROFILER = counter if i == 0 else None
        try:
            loss, _ = den(batches[0] if i < warm else batches[i % 2])
            loss.backward()
        finally:
            nv.PROFILER = None
        torch.nn.utils.clip_grad_norm_(den.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if i >= warm:
            losses_e.append(loss.detach().clone())
    assert "dgrad_input_kernel" not in counter.n and "dmd_conv2d_dgrad_input" not in counter.n and sum(counter.n.values()) > 100
    params_e = {k: v.detach().clone() for k, v in den.named_parameters()}

    den2, opt2, batches2 = setup()
    den2.load_state_dict(init)
    gstep = GraphedTrainStep(den2, opt2, 1.0, batches2[0], warmup_steps=warm)
    losses_g = [gstep(batches2[(warm + i) % 2])[0].clone() for i in range(steps)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(losses_e, losses_g)), (losses_e, losses_g)
    assert max(float((p.detach() - params_e[k]).abs().max()) for k, p in den2.named_parameters()) == 0.0
    assert max(float((p.detach() - init[k]).abs().max()) for k, p in den2.named_parameters()) > 1e-4, "parameters did not train"
