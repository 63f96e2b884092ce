"""Collector: env steps from the env loop straight into the device replay store (reference coroutines/collector.py:16-126).

The reference's collector reads `(end + trunc).item()` once per env and step, concatenates every step into a CPU Episode and, for an
episode that is still growing, reloads the whole episode, appends to it and hands it over again.  Here a WINDOW of env steps -- the
stacked device tensors `make_env_loop` yields -- goes into the store's arena in one launch (`DeviceReplay.record_window`): per
window the host reads back B x T rewards and flags, never a frame.

    store = DeviceReplay(device, name="train")
    collector = make_collector(env, agent.actor_critic, store, epsilon=0.01)
    logs = collector.send(NumToCollect(steps=1000))       # the reference's protocol and the reference's log dicts, in its order

The same entry records the IMAGINED rollouts of WorldModelEnv (play.py's recording mode, datasets collected from imagination).
The collector asks `make_env_loop` for the sequential order of calls: the slots loop's infos carry no `final_observation`;
recording at the slots loop's speed is out of scope here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Generator, List, Optional

import torch

from .env_loop import coroutine, make_env_loop
from .replay import DeviceReplay

Logs = List[Dict[str, Any]]


@dataclass
class NumToCollect:
    steps: Optional[int] = None
    episodes: Optional[int] = None

    def __post_init__(self) -> None:
        assert (self.steps is None) != (self.episodes is None)

    def can_stop(self, num_steps: int, num_episodes: int) -> bool:
        return num_steps >= self.steps if self.steps is not None else num_episodes >= self.episodes

    @property
    def unit(self) -> str:
        return "steps" if self.steps is not None else "eps"

    @property
    def total(self) -> int:
        return self.steps if self.steps is not None else self.episodes


@coroutine
def make_collector(env, model, store: DeviceReplay, epsilon: float = 0.0, reset_every_collect: bool = False, verbose: bool = False,
                   window: int = 64) -> Generator[Logs, NumToCollect, None]:
    """The reference's collector protocol: send a NumToCollect, get the logs -- per episode that ended {"<name>/episode_id",
    "length", "return"} in order of death, then one dict with "<name>/num_steps" and the five "<name>/counts/..." -- with the ids,
    lengths and counts the reference's collector and Dataset give on the same env and policy.
    NumToCollect(steps=): `num_envs` steps are collected per env step, so the stop step is known in advance: windows of up to
    `window` env steps that never cross it.  NumToCollect(episodes=): one env step per window (an env cannot be un-stepped).
    reset_every_collect: a new env loop per collect, unfinished episodes are dropped (the test collector); otherwise they stay
    in the store and grow in the next collect (the train collector).  Frames off the uint8 grid raise ValueError
    (`store.assert_on_grid()`) before the logs of the collect are yielded."""
    num_envs = env.num_envs
    assert window >= 1
    env_loop = None

    def reset() -> None:
        nonlocal env_loop
        env_loop = make_env_loop(env, model, epsilon, kind="sequential")

    num_to_collect = yield
    reset()
    keep_open = not reset_every_collect
    while True:
        num_steps = num_episodes = 0
        to_log: Logs = []
        while True:
            if num_to_collect.steps is not None:
                left = max(1, -(-(num_to_collect.steps - num_steps) // num_envs))  # env steps up to the stop step
                t = min(window, left)
                stop_if = 0 if t == left else None
            else:
                t, stop_if = 1, max(1, num_to_collect.episodes - num_episodes)
            with torch.no_grad():
                all_obs, act, rew, end, trunc, *_, infos = env_loop.send(t)
            finals = [info["final_observation"] for info in infos if "final_observation" in info]
            done = store.record_window(all_obs, act, rew, end, trunc, finals or None, store_open_if_episodes=stop_if if keep_open else None)
            num_steps += num_envs * t
            num_episodes += len(done)
            to_log += [{f"{store.name}/episode_id": d["episode_id"], "length": d["length"], "return": d["return"]} for d in done]
            if num_to_collect.can_stop(num_steps, num_episodes):
                break
        store.end_collect(keep_open=keep_open)
        store.assert_on_grid()
        counts_rew, counts_end = store.counts_rew, store.counts_end
        metrics = {"num_steps": store.num_steps, "counts/rew_-1": counts_rew[0], "counts/rew__0": counts_rew[1], "counts/rew_+1": counts_rew[2],
                   "counts/end_0": counts_end[0], "counts/end_1": counts_end[1]}
        to_log.append({f"{store.name}/{k}": v for k, v in metrics.items()})
        if verbose:
            print(f"Collect {store.name}: {num_steps} steps, {num_episodes} episodes; {store.num_episodes} episodes, {store.num_steps} steps stored")
        num_to_collect = yield to_log
        if reset_every_collect:
            reset()
