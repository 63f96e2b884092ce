"""The host plumbing of the image gradients on the SIMT interpreter (tests/simt/host_harness.py), so that `-m "not gpu"` covers
it: the policy's `obs.grad` through ActorCritic.predict_act_value -- _EncoderFn.backward -> grad_ops.dgrad_input ->
dmd_conv2d_dgrad_input -- against the float64 autograd of the oracle's restatement, bar 1e-4 of max |ref| as on the device
(tests/test_gpu_input_grads.py); 72x72 runs as the valid extent of a 128x128 buffer.  No launch is added where the observation
requires no gradient."""
import pytest
import torch

from tests.conftest import WEIGHT_SEED
from tests.test_gpu_input_grads import _Counter, _sd64, work_launches
from tests.test_gpu_models import rel_err


@pytest.fixture(scope="module")
def policy():
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    agent = D.Agent(D.default_agent_config())
    fill_module_(agent, WEIGHT_SEED)
    return agent.actor_critic.eval()


def _run(ac, obs, cot_l, cot_v, want):
    from diamond_amd import native as nv
    from tests.simt.host_harness import engine_on_interpreter

    ac.zero_grad(set_to_none=True)
    o = obs.clone().requires_grad_(want)
    counter = _Counter()
    saved, nv.PROFILER = nv.PROFILER, counter
    try:
        with engine_on_interpreter():
            out = ac.predict_act_value(o, None)
            ((out.logits_act * cot_l).sum() + (out.val.reshape(-1) * cot_v).sum()).backward()
    finally:
        nv.PROFILER = saved
    return o.grad, {k: p.grad.clone() for k, p in ac.named_parameters()}, work_launches(counter)


@pytest.mark.parametrize("size", [64, 72])
def test_policy_image_gradient_on_the_interpreter(policy, size):
    from diamond_amd.testing import synthetic_frames
    from oracle import diamond_oracle as O

    g = torch.Generator().manual_seed(11 + size)
    obs = synthetic_frames(g, 1, 3, size, size)
    cot_l, cot_v = torch.randn(1, 4, generator=g), torch.randn(1, generator=g)
    o64 = obs.double().requires_grad_(True)
    z = torch.zeros(1, 512, dtype=torch.float64)
    logits, val, _ = O.ac_predict(_sd64(policy), O.ActorCriticSpec(img_size=size), o64, z, z)
    ((logits * cot_l.double()).sum() + (val * cot_v.double()).sum()).backward()

    grad, params1, n1 = _run(policy, obs, cot_l, cot_v, True)
    assert grad is not None and grad.shape == obs.shape, "autograd did not reach the policy's observation"
    e = rel_err(grad, o64.grad)
    print(f"actor-critic {size}x{size} on the interpreter: obs.grad {e:.2e}")
    assert e <= 1e-4, e
    none, params0, n0 = _run(policy, obs, cot_l, cot_v, False)
    assert none is None and all(torch.equal(params0[k], params1[k]) for k in params0)
    assert n1.get("dgrad_input_kernel") == 1 and "dgrad_input_kernel" not in n0 and sum(n1.values()) == sum(n0.values()) + 1, (n0, n1)
