"""bench.py --dump-outputs (CPU): the tap keeps what ActorCritic.forward() hands its caller in one step and leaves the module as it
found it; dump_outputs writes float32 / float64 arrays within the size limit, with seeded samples that are the same every run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _FakeActorCritic(torch.nn.Module):
    """ActorCritic's calling convention: forward() pulls one window from env_loop.send(steps) and returns (loss, metrics)."""

    def __init__(self, b=5, t=3, size=8):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)
        g = torch.Generator().manual_seed(0)

        def loop():
            n = yield
            while True:
                out = (torch.randn(b, n, 3, size, size, generator=g), torch.randint(0, 3, (b, n), generator=g),
                       torch.randn(b, n, generator=g), torch.rand(b, n, generator=g) > 0.5, torch.rand(b, n, generator=g) > 0.5,
                       self.lin(torch.randn(b, n, 4, generator=g)), torch.randn(b, n, generator=g), torch.randn(b, n, generator=g), [])
                n = yield out

        self.env_loop = loop()
        next(self.env_loop)
        self.t = t

    def forward(self):
        _, act, rew, end, trunc, logits, val, vb, _ = self.env_loop.send(self.t)
        loss = logits.square().mean() + rew.mean()
        return loss, {"loss_total": loss.detach(), "policy_entropy": logits.detach().std()}


def _step(ac):
    loss, _ = ac()
    loss.backward()
    with torch.no_grad():
        for p in ac.parameters():
            p -= 0.1 * p.grad
    return loss


def test_tap_records_one_step_and_restores_the_module(tmp_path):
    ac = _FakeActorCritic()
    loop = ac.env_loop
    tap = bench.OutputTap(ac)
    loss = _step(ac)
    tap.remove()
    assert ac.env_loop is loop and "forward" not in vars(ac)
    assert tap.loss.requires_grad is False and float(tap.loss) == float(loss.detach())
    assert set(tap.rollout) == set(bench.OutputTap.ROLLOUT) and tap.rollout["obs"].shape == (5, 3, 3, 8, 8)

    shapes = bench.dump_outputs(str(tmp_path), tap, ac)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(f"{k}.npy" for k in shapes)
    for f in files:
        assert np.load(tmp_path / f).dtype in (np.float32, np.float64), f
    assert np.load(tmp_path / "loss.npy").shape == () and np.load(tmp_path / "loss.npy") == np.float32(float(loss.detach()))
    params = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "actor_critic_params.npy"), params)  # (the parameters AFTER the step)
    assert np.array_equal(np.load(tmp_path / "rollout_obs_sample.npy"), tap.rollout["obs"].numpy())  # small: every row
    assert np.array_equal(np.load(tmp_path / "rollout_end.npy"), tap.rollout["end"].numpy().astype(np.float32))


def test_samples_are_seeded_and_within_budget(tmp_path):
    ac = _FakeActorCritic(b=7, size=16)
    tap = bench.OutputTap(ac)
    _step(ac)
    tap.remove()
    row = 3 * 3 * 16 * 16 * 4
    kw = dict(frame_budget=2 * row, param_budget=12 * 4)  # (15 parameters do not fit: 4 sampled at 12 bytes, value + position)
    bench.dump_outputs(str(tmp_path / "a"), tap, ac, **kw)
    bench.dump_outputs(str(tmp_path / "b"), tap, ac, **kw)
    rows = np.load(tmp_path / "a" / "rollout_obs_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 2 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rollout_obs_sample.npy"), tap.rollout["obs"][torch.from_numpy(rows).long()].numpy())
    idx = np.load(tmp_path / "a" / "actor_critic_params_sample_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 4 and np.all(np.diff(idx) > 0)
    flat = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "actor_critic_params.npy"), flat[idx.astype(np.int64)])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < bench.DUMP_LIMIT_BYTES


def test_configs4_sizes_fit_the_limit_with_the_default_budgets(tmp_path):
    """configs[4] (256x256, 8 envs, horizon 15): the real ActorCritic (~35M parameters: the sampled branch) and a rollout of that
    shape, through dump_outputs with its default budgets -- within the 64 MB limit, sampled values at their stored positions."""
    from types import SimpleNamespace

    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    ac = D.ActorCritic(D.default_agent_config(num_actions=4, img_size=256).actor_critic)
    fill_module_(ac, 3)
    b, t = 8, 15
    g = torch.Generator().manual_seed(0)
    rollout = {k: torch.randn(b, t, generator=g) for k in bench.OutputTap.ROLLOUT}
    rollout["obs"] = torch.randn(b, t, 3, 256, 256, generator=g)
    rollout["logits_act"] = torch.randn(b, t, 4, generator=g)
    loss = torch.tensor(0.5)
    tap = SimpleNamespace(loss=loss, metrics={"loss_total": loss}, rollout=rollout)
    shapes = bench.dump_outputs(str(tmp_path), tap, ac)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= bench.DUMP_LIMIT_BYTES, shapes
    flat = torch.cat([p.detach().reshape(-1) for p in ac.parameters()])
    assert flat.numel() > 30_000_000 and "actor_critic_params_sample_index" in shapes
    idx = np.load(tmp_path / "actor_critic_params_sample_index.npy")
    vals = np.load(tmp_path / "actor_critic_params.npy")
    assert len(idx) == len(vals) > 1_000_000 and np.all(np.diff(idx) > 0) and idx[-1] < flat.numel()
    assert np.array_equal(vals, flat.numpy()[idx.astype(np.int64)])
    rows = np.load(tmp_path / "rollout_obs_rows.npy").astype(np.int64)
    assert len(rows) >= 1 and np.array_equal(np.load(tmp_path / "rollout_obs_sample.npy"), rollout["obs"].numpy()[rows])


def test_configs1_parameters_are_dumped_whole(tmp_path):
    """configs[1] (64x64, 256 envs): the actor-critic's 3.2M parameters fit the parameter budget as float32 values, so all of them
    are written, in named_parameters() order, with no position array."""
    from types import SimpleNamespace

    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    ac = D.ActorCritic(D.default_agent_config(num_actions=4).actor_critic)
    fill_module_(ac, 3)
    rollout = {k: torch.zeros(256, 15) for k in bench.OutputTap.ROLLOUT}
    rollout["obs"] = torch.zeros(256, 15, 3, 64, 64)
    loss = torch.tensor(0.5)
    shapes = bench.dump_outputs(str(tmp_path), SimpleNamespace(loss=loss, metrics={}, rollout=rollout), ac)
    assert "actor_critic_params_sample_index" not in shapes
    flat = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "actor_critic_params.npy"), flat)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_LIMIT_BYTES
