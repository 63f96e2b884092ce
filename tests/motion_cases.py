"""Shared by tests/test_openloop_motion.py and tests/openloop_motion_launch.py: an arena that looks like recorded frames (a static
background per episode, a handful of levels changing per step, some steps identical to their predecessor), descriptor rows of
every kind dmd_openloop_motion distinguishes, a ring whose newest slot alone holds numbers, and an int64 numpy RESTATEMENT of the
entry point written from its contract in include/diamond_hip.h:

    level(v) = clip(rint((v + 1) / 2 * 255), 0, 255) in fp32.  s = start + T + step.  y: arena row first + s when 0 <= s < len, the
    final observation when s == len, final_row >= 0 (and finals is not NULL) and the episode's last step has end != 0; otherwise the
    frame is invalid: eight zeros, three zero flags.  r = arena row first + s - 1, valid with the frame when s >= 1.  a = arena row
    first + start + T - 1, valid with the frame when 0 <= start + T - 1 < len.  q = level(pred), m = level(ring slot (head + T - 1) % T).
    out = sum (y - r)^2, sum (y - a)^2, #{y != r}, #{q != m}, #{y != r and q != m}, sum over {y != r} of (q - y)^2,
    #{y != r and q == y}, 0; entries 0, 2, 4, 5, 6 are 0 without r, entry 1 without a.  out_valid = frame, r, a.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from tests import openloop_cases as OC
from tests.replay_cases import dequant

STEP = OC.STEP
PER_FRAMES = OC.PER_FRAMES  # 16 levels per lane; 4 levels per lane; one level per lane
EPISODES = OC.EPISODES      # (length, last step has end != 0, has a final observation)
# (episode, s - 5, kind): the frame compared is episode step s whatever T is (start = s - T - STEP), the anchor is step s - 2.
# The nine kinds of tests/openloop_cases.py first (their starts at T = 4), then the ones only this entry tells apart.
SAMPLES = OC.SAMPLES + (
    (1, 1, "final observation after the last step"),  # s = 6 = len: y is the final observation, r the episode's last step
    (0, -5, "s = 0"),                                 # frame valid, nothing before it: r (and a) invalid
    (0, -4, "context of padding only"),               # s = 1, the anchor would be step -1: r valid, a invalid
    (0, 3, "prediction equal to the recording"),      # s = 8
    (0, 1, "prediction equal to m"),                  # s = 6: q == m everywhere
    (0, 5, "an unchanged step"),                      # s = 10 repeats step 9: nothing moved in the recording
)
KINDS = tuple(k for _, _, k in SAMPLES)
#                 (frame, r, a)
EXPECTED_VALID = {"inside": (1, 1, 1), "left padding": (1, 1, 1), "final observation": (1, 1, 1), "end without a final frame": (0, 0, 0),
                  "beyond the end": (0, 0, 0), "final frame without an end": (0, 0, 0), "first step": (1, 0, 0), "before the episode": (0, 0, 0),
                  "equal to its target": (1, 1, 1), "final observation after the last step": (1, 1, 1), "s = 0": (1, 0, 0),
                  "context of padding only": (1, 1, 0), "prediction equal to the recording": (1, 1, 1), "prediction equal to m": (1, 1, 1),
                  "an unchanged step": (1, 1, 1)}
UNCHANGED = (3, 10)  # episode steps that repeat their predecessor (where the episode is that long)


def make_arena(per_frame: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Per episode one random background; every step changes up to three values to another level, the steps of UNCHANGED none; a
    final observation changes up to three values of the last step."""
    rng = np.random.RandomState(seed)
    total = sum(n for n, _, _ in EPISODES)
    frames, end = np.empty((total, per_frame), np.uint8), np.zeros(total, np.uint8)
    first, final_row, finals, at = [], [], [], 0

    def moved(frame):
        out = frame.copy()
        at_ = rng.choice(per_frame, min(3, per_frame), replace=False)
        out[at_] = (out[at_].astype(np.int64) + rng.randint(1, 256, len(at_))) % 256  # never the level it had
        return out

    for n, ends, final in EPISODES:
        first.append(at)
        frames[at] = rng.randint(0, 256, per_frame)
        for k in range(1, n):
            frames[at + k] = frames[at + k - 1] if k in UNCHANGED else moved(frames[at + k - 1])
        end[at + n - 1] = int(ends)
        final_row.append(len(finals) if final else -1)
        if final:
            finals.append(moved(frames[at + n - 1]))
        at += n
    return {"frames": frames, "end": end, "finals": np.array(finals, np.uint8).reshape(len(finals), per_frame), "first": np.array(first, np.int64),
            "len": np.array([n for n, _, _ in EPISODES], np.int64), "final_row": np.array(final_row, np.int64)}


def descriptor(arena: Dict[str, np.ndarray], t: int) -> np.ndarray:
    return np.array([(arena["first"][e], start + OC.T - t, arena["len"][e], arena["final_row"][e]) for e, start, _ in SAMPLES], np.int64)


def levels_of(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.float32)
    lv = np.rint((v + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0))
    return np.clip(lv, np.float32(0.0), np.float32(255.0)).astype(np.int64)


def target_of(arena: Dict[str, np.ndarray], row: np.ndarray, t: int, step: int) -> Optional[np.ndarray]:
    first, start, n, final_row = (int(v) for v in row)
    s = start + t + step
    if 0 <= s < n:
        return arena["frames"][first + s]
    if s == n and n >= 1 and final_row >= 0 and len(arena["finals"]) and arena["end"][first + n - 1] != 0:
        return arena["finals"][final_row]
    return None


def _values(rng, base: np.ndarray, changes: int) -> np.ndarray:
    """fp32 values whose levels are `base` with `changes` of them moved: on the grid, +- 0.499 of a level beside it, and (on top
    of the changes) two values far outside [-1, 1]"""
    pf = len(base)
    level = base.astype(np.float64)
    at = rng.choice(pf, min(changes, pf), replace=False)
    level[at] = (level[at] + rng.randint(1, 256, len(at))) % 256
    kind = rng.randint(0, 3, pf)
    v = ((level + np.where(kind == 1, 0.499, 0.0) - np.where(kind == 2, 0.499, 0.0)) / 255.0) * 2.0 - 1.0
    far = rng.choice(pf, min(2, pf), replace=False)
    v[far] = np.where(rng.rand(len(far)) < 0.5, -1.0 - rng.rand(len(far)) * 3, 1.0 + rng.rand(len(far)) * 3)
    return v.astype(np.float32)


def make_case(per_frame: int, head: int, t: int = OC.T, step: int = STEP, seed: int = 0) -> Dict[str, np.ndarray]:
    """The ring's newest slot: the previous recorded frame with a few values moved (what a rollout's last frame looks like); every
    other slot NaN -- the entry must not read them.  The prediction: the target with a few values moved."""
    arena = make_arena(per_frame, seed)
    seg = descriptor(arena, t)
    rng = np.random.RandomState(seed + 100)
    b, newest = len(seg), (head + t - 1) % t
    ring = np.full((b, t, per_frame), np.nan, np.float32)
    pred = np.empty((b, per_frame), np.float32)
    for i, row in enumerate(seg):
        first, start, n, _ = (int(v) for v in row)
        s = start + t + step
        y = target_of(arena, row, t, step)
        r = arena["frames"][first + s - 1] if y is not None and s >= 1 else rng.randint(0, 256, per_frame)
        ring[i, newest] = _values(rng, r, 2)
        pred[i] = _values(rng, rng.randint(0, 256, per_frame) if y is None else y, 4)
        if KINDS[i] in ("equal to its target", "prediction equal to the recording") and y is not None:
            pred[i] = dequant(y)
        if KINDS[i] == "prediction equal to m":
            pred[i] = ring[i, newest]
    return {"arena": arena, "seg": seg, "T": t, "head": head, "step": step, "pred": pred, "ctx_obs": ring}


def rows_of(case: Dict[str, np.ndarray], rows) -> Dict[str, np.ndarray]:
    """The same case restricted to some samples."""
    out = dict(case)
    for k in ("seg", "pred", "ctx_obs"):
        out[k] = np.ascontiguousarray(case[k][rows])
    return out


def without_finals(case: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The same case on an arena that kept no final observation (finals = NULL)."""
    return dict(case, arena=dict(case["arena"], finals=case["arena"]["finals"][:0]))


def restate(case: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    arena, seg, t, head, step, pred = (case[k] for k in ("arena", "seg", "T", "head", "step", "pred"))
    b = len(seg)
    out, valid = np.zeros((b, 8), np.int64), np.zeros((b, 3), np.uint8)
    for i, row in enumerate(seg):
        first, start, n, _ = (int(v) for v in row)
        s, c = start + t + step, start + t - 1
        y = target_of(arena, row, t, step)
        if y is None:
            continue
        y = y.astype(np.int64)
        q, m = levels_of(pred[i]), levels_of(case["ctx_obs"][i, (head + t - 1) % t])
        valid[i, 0] = 1
        out[i, 3] = (q != m).sum()
        if s >= 1:
            r = arena["frames"][first + s - 1].astype(np.int64)
            ch = y != r
            out[i, [0, 2, 4, 5, 6]] = (((y - r) ** 2).sum(), ch.sum(), (ch & (q != m)).sum(), ((q - y) ** 2)[ch].sum(), (ch & (q == y)).sum())
            valid[i, 1] = 1
        if 0 <= c < n:
            out[i, 1] = ((y - arena["frames"][first + c].astype(np.int64)) ** 2).sum()
            valid[i, 2] = 1
    return {"out": out, "valid": valid}
