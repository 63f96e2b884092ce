"""The ORDERED sequence of C-ABI launches of one forward + backward through each of the hand-written backward passes, on the CPU
(the real host layer -- engine.py, grad_ops.py, ac_native.py, unet_train.py -- driving the SIMT-interpreter build of the kernels).
The captured training graph and the step time depend on the order and number of launches; a change to the host layer that is meant
to leave them alone is held to tests/golden/launch_sequences.json (every launch's profiler key, from freshly built models, so the
packing launches of the first use are part of it).  Whoever changes the sequence on purpose records the file again, and says so."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests.conftest import GOLDEN, WEIGHT_SEED
from tests.simt.host_harness import engine_on_interpreter


class _LaunchRecorder:
    """stands in for native.PROFILER: the key of every launch, in order (no timing)"""

    def __init__(self):
        self.keys = []
        self._pending = None

    def annotate(self, key, flops, nbytes):
        self._pending = key

    def call(self, name, fn, args):
        key, self._pending = self._pending or name, None
        self.keys.append(key)
        return fn(*args)


def _agent(img_size=64):
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    agent = D.Agent(D.default_agent_config(img_size=img_size))
    fill_module_(agent, WEIGHT_SEED)
    return agent.eval()


def _encoder_step(size):
    from diamond_amd.testing import synthetic_frames

    ac = _agent(size).actor_critic
    ac.encode(synthetic_frames(torch.Generator().manual_seed(3), 2, 3, size, size)).square().sum().backward()
    return ac


def _denoiser_step():
    import diamond_amd as D
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    den = _agent().denoiser
    den.train()
    den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
    g = torch.Generator().manual_seed(5)
    batch = SimpleNamespace(obs=synthetic_frames(g, 1, 5, 3, 64, 64), act=synthetic_actions(g, 4, 1, 5), mask_padding=torch.ones(1, 5, dtype=torch.bool))
    den.randn_fn = lambda shape: torch.randn(*shape)
    torch.manual_seed(77)
    den(batch)[0].backward()
    return den


def _rew_end_step():
    from diamond_amd.testing import rew_end_train_batch

    m = _agent().rew_end_model
    m.train()
    m(SimpleNamespace(**rew_end_train_batch(torch.Generator().manual_seed(11), b=3, t=5)))[0].backward()
    return m


STEPS = {"encoder_64": (lambda: _encoder_step(64), 75), "encoder_72": (lambda: _encoder_step(72), 79), "denoiser": (_denoiser_step, 932),
         "rew_end": (_rew_end_step, 355)}


@pytest.mark.parametrize("step", list(STEPS))
def test_the_launches_of_a_training_step_are_the_recorded_ones_in_order(step, monkeypatch):
    from diamond_amd import native as nv

    with open(os.path.join(GOLDEN, "launch_sequences.json")) as f:
        want = json.load(f)[step]
    run, count = STEPS[step]
    assert len(want) == count
    rec = _LaunchRecorder()
    monkeypatch.setattr(nv, "PROFILER", rec)
    monkeypatch.delenv("DIAMOND_WGRAD_DEFER", raising=False)
    with engine_on_interpreter():
        module = run()
    grads = [p.grad for p in module.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    first = next((i for i, (a, b) in enumerate(zip(rec.keys, want)) if a != b), min(len(rec.keys), len(want)))
    assert rec.keys == want, (f"{len(rec.keys)} launches, {len(want)} recorded; the first difference is launch {first}: "
                              f"{rec.keys[first - 2:first + 3]} against the recorded {want[first - 2:first + 3]}")
