"""Shared by tests/golden/make_collector_golden.py (which drives the REFERENCE's collector) and the collector tests (which drive
diamond_amd.collector): a scripted env with the interface of the reference's TorchEnv, a scripted policy, and the script of
collects.  Torch only; nothing here imports the reference or the product.

The env: frames of 3x8x8 on the uint8 grid, a function of (env, episode, step); the reward an integer in {-2 ... 2} that depends on
the ACTION taken; episode lengths from a table, deaths alternately by `end` and by `trunc`; a dead env restarts at once and the
step's info carries `final_observation` (n_dead, 3, 8, 8) in ascending env order.  The policy puts one action -- the level of
the frame's first value modulo the number of actions -- 1e4 above the others, so the sampled action does not depend on the draw.
"""
from __future__ import annotations

from typing import Any, Dict, Iterator, List, Tuple

import torch

FRAME = (3, 8, 8)
NUM_ACTIONS = 4
LENGTHS = (3, 2, 4, 1, 5, 2, 3, 6)
NUM_ENVS = (1, 3)
TRAIN_STEPS = {1: (4, 3, 5), 3: (9, 6, 12)}   # three NumToCollect(steps=...) on the train collector
TEST_EPISODES = (2, 3)                         # two NumToCollect(episodes=...) with reset_every_collect
NAME = "train"


def dequant(u8: torch.Tensor) -> torch.Tensor:
    return u8.div(255).mul(2).sub(1)  # the reference's Episode.load


def levels(x: torch.Tensor) -> torch.Tensor:
    return x.add(1).div(2).mul(255).round().to(torch.uint8)


def frame_levels(env: int, episode: int, step: int) -> torch.Tensor:
    n = FRAME[0] * FRAME[1] * FRAME[2]
    return ((torch.arange(n) * 7 + env * 31 + episode * 13 + step * 5) % 256).to(torch.uint8).reshape(FRAME)


def episode_length(env: int, episode: int) -> int:
    return LENGTHS[(env * 3 + episode) % len(LENGTHS)]


class ScriptedEnv:
    def __init__(self, num_envs: int, device="cpu") -> None:
        self.num_envs, self.num_actions, self.device = num_envs, NUM_ACTIONS, torch.device(device)
        self.resets = 0
        self.episode = [0] * num_envs
        self.step_in_episode = [0] * num_envs

    def _obs(self) -> torch.Tensor:
        return dequant(torch.stack([frame_levels(i, self.episode[i], self.step_in_episode[i]) for i in range(self.num_envs)])).to(self.device)

    def reset(self, **kwargs: Any) -> Tuple[torch.Tensor, Dict[str, Any]]:
        self.episode = [10 * self.resets] * self.num_envs
        self.step_in_episode = [0] * self.num_envs
        self.resets += 1
        return self._obs(), {}

    def step(self, act: torch.Tensor):
        acts = act.tolist()
        rew, end, trunc, finals = [], [], [], []
        for i in range(self.num_envs):
            e, s = self.episode[i], self.step_in_episode[i]
            rew.append(float((s + acts[i] + e) % 5 - 2))
            dead = s + 1 == episode_length(i, e)
            by_end = (i + e) % 2 == 0
            end.append(int(dead and by_end))
            trunc.append(int(dead and not by_end))
            if dead:
                finals.append(frame_levels(i, e, s + 1))
                self.episode[i], self.step_in_episode[i] = e + 1, 0
            else:
                self.step_in_episode[i] = s + 1
        info = {"final_observation": dequant(torch.stack(finals)).to(self.device)} if finals else {}
        d = self.device
        return (self._obs(), torch.tensor(rew, dtype=torch.float32, device=d), torch.tensor(end, dtype=torch.uint8, device=d),
                torch.tensor(trunc, dtype=torch.uint8, device=d), info)


class ScriptedPolicy:
    lstm_dim = 4

    def __init__(self, device="cpu") -> None:
        self.device = torch.device(device)

    def predict_act_value(self, obs: torch.Tensor, hx_cx):
        a = levels(obs[:, 0, 0, 0]).long() % NUM_ACTIONS
        logits = torch.zeros(obs.shape[0], NUM_ACTIONS, device=obs.device)
        logits[torch.arange(obs.shape[0], device=obs.device), a] = 1e4
        return logits, torch.zeros(obs.shape[0], device=obs.device), hx_cx


def run_script(num_envs: int, make_collector, num_to_collect, dataset, device="cpu", **collector_kwargs) -> Iterator[List[Dict[str, Any]]]:
    """The script on any collector with the reference's protocol (`dataset`: the reference's Dataset or a DeviceReplay): three
    collects by steps on a train collector, `dataset.clear()`, two collects by episodes on a collector that resets at every
    collect.  A generator: yields the logs of each of the five collects, so that the caller can look at the dataset in between."""
    env, model = ScriptedEnv(num_envs, device), ScriptedPolicy(device)
    collector = make_collector(env, model, dataset, epsilon=0.0, reset_every_collect=False, verbose=False, **collector_kwargs)
    for steps in TRAIN_STEPS[num_envs]:
        yield collector.send(num_to_collect(steps=steps))
    dataset.clear()
    collector = make_collector(env, model, dataset, epsilon=0.0, reset_every_collect=True, verbose=False, **collector_kwargs)
    for episodes in TEST_EPISODES:
        yield collector.send(num_to_collect(episodes=episodes))
