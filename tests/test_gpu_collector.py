"""diamond_amd.collector on the GPU (`-m gpu`): the golden script of tests/test_collector_simt.py on the device, and one imagined
window of a WorldModelEnv recorded through the collector."""
from types import SimpleNamespace

import pytest
import torch

from tests import collector_cases as CC
from tests.conftest import WEIGHT_SEED, load_golden
from tests.test_collector_simt import run_golden_script

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("window", [64, 2])
@pytest.mark.parametrize("num_envs", CC.NUM_ENVS)
def test_collector_reproduces_the_reference_collector_on_the_device(num_envs, window):
    """The reference collector's logs, ids, lengths, counts and episodes (tests/golden/collector_episodes.pt), from a store on
    the device filled by dmd_record_window."""
    store = run_golden_script(load_golden("collector_episodes.pt")[num_envs], num_envs, DEV, window)
    assert store.frames.is_cuda and store._open == {}


class _Loader:
    def __init__(self, b, batches):
        self.batch_sampler = SimpleNamespace(batch_size=b)
        self._batches = batches

    def __iter__(self):
        i = 0
        while True:
            obs, act = self._batches[i % len(self._batches)]
            i += 1
            yield SimpleNamespace(obs=obs, act=act)


def test_imagined_rollout_is_recorded_through_the_collector():
    """WorldModelEnv (64x64 frames, horizon 3, one denoising step) driven by the policy for 5 env steps of 3 envs, in windows of 2:
    every env is truncated at the horizon inside the collect.  The store's episodes are the frames the env loop yielded,
    quantised (an imagined frame is the sampler's last Euler step, ulps off the level the denoiser quantised it to: the store
    is built with strict_grid=False and holds its nearest level), cut where end | trunc, with the infos' final observations;
    ids and lengths are what the reference collector's bookkeeping gives on the yielded flags."""
    import diamond_amd as D
    from diamond_amd.collector import NumToCollect, make_collector
    from diamond_amd.replay import DeviceReplay
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames

    agent = D.Agent(D.default_agent_config())
    fill_module_(agent, WEIGHT_SEED)
    agent = agent.to(DEV).eval()
    b, steps = 3, 5
    g = torch.Generator().manual_seed(5)
    batches = [(synthetic_frames(g, b, 4, 3, 64, 64), synthetic_actions(g, 4, b, 4)) for _ in range(4)]
    env = D.WorldModelEnv(agent.denoiser, agent.rew_end_model, _Loader(b, batches),
                          D.WorldModelEnvConfig(horizon=3, num_batches_to_preload=2, diffusion_sampler=D.DiffusionSamplerConfig(num_steps_denoising=1)))
    store = DeviceReplay(DEV, name="imagination", strict_grid=False)
    yielded = []
    record = store.record_window

    def spy(obs, act, rew, end, trunc, final_observation=None, **kw):
        yielded.append([x.clone() for x in (obs, act, rew, end, trunc)] + [[f.clone() for f in final_observation or []]])
        return record(obs, act, rew, end, trunc, final_observation, **kw)

    store.record_window = spy
    torch.manual_seed(3)
    logs = make_collector(env, agent.actor_critic, store, window=2).send(NumToCollect(steps=b * steps))
    assert [w[0].shape[1] for w in yielded] == [2, 2, 1]
    obs, act, rew, end, trunc = (torch.cat([w[k] for w in yielded], dim=1).cpu() for k in range(5))
    finals = [f.cpu() for w in yielded for tensor in w[5] for f in tensor]  # in order of death
    dead = (end != 0) | (trunc != 0)
    assert bool(trunc.any()) and len(finals) == int(dead.sum())

    # the reference collector's bookkeeping (coroutines/collector.py:60-90) on the yielded flags
    want, open_since, ids = [], [0] * b, {}
    for t in range(steps):
        for i in range(b):
            if dead[i, t] or t == steps - 1:
                ids[(i, open_since[i])] = len(ids)
                final = finals.pop(0) if dead[i, t] else None
                want.append((i, open_since[i], t + 1, final))
                if dead[i, t]:
                    open_since[i] = t + 1
    assert store.num_episodes == len(want) and store.num_steps == b * steps and not finals
    for eid, (i, t0, t1, final) in enumerate(want):
        ep = store.load_episode(eid).to("cpu")
        assert torch.equal(ep.obs, CC.dequant(CC.levels(obs[i, t0:t1].clamp(-1, 1)))) and float((ep.obs - obs[i, t0:t1].clamp(-1, 1)).abs().max()) <= 1.001 / 255, eid  # (half a grid step)
        assert torch.equal(ep.act, act[i, t0:t1]) and torch.equal(ep.rew, rew[i, t0:t1]), eid
        assert torch.equal(ep.end, (end[i, t0:t1] != 0).to(torch.uint8)) and torch.equal(ep.trunc, (trunc[i, t0:t1] != 0).to(torch.uint8)), eid
        assert torch.equal(store.frames[int(store._first[eid]):][:t1 - t0].cpu().reshape(-1, 3, 64, 64), CC.levels(obs[i, t0:t1].clamp(-1, 1))), eid
        assert ("final_observation" in ep.info) == (final is not None), eid
        if final is not None:
            assert torch.equal(ep.info["final_observation"], CC.dequant(CC.levels(final.clamp(-1, 1)))), eid
    ended = [e for e, (i, t0, t1, final) in enumerate(want) if final is not None]
    assert [d["imagination/episode_id"] for d in logs[:-1]] == ended
    assert [d["length"] for d in logs[:-1]] == [want[e][2] - want[e][1] for e in ended]
    assert logs[-1]["imagination/num_steps"] == b * steps
    assert logs[-1]["imagination/counts/end_0"] + logs[-1]["imagination/counts/end_1"] == b * steps
