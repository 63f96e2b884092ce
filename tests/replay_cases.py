"""Shared by tests/test_replay_simt.py and tests/test_gpu_replay.py: synthetic arenas, the descriptor sets of the issue's kernel
cases and a numpy RESTATEMENT of dmd_segment_gather (include/diamond_hip.h), written from the entry's contract:

    step s = start + t is valid iff 0 <= s < len; a valid position copies arena row first + s (frames dequantised as
    (q / 255) * 2 - 1 in fp32), an invalid one is exact zeros with mask 0; final_obs[b] is the dequantised final frame or zeros;
    with put_back_final, the position s == len (t >= 1) of an episode whose last step has end != 0 and that has a final frame
    holds that frame.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Tuple

import numpy as np

# (length, how the last step is marked): lengths 1, 2, 7, 30 with `end`, `trunc` only, and neither
EPISODES = ((1, "end"), (2, "trunc"), (7, "end"), (30, "none"), (7, "trunc"), (30, "end"), (2, "none"), (1, "none"), (2, "end"))
PER_FRAMES = (192, 108, 25)  # 3x8x8: 16-byte path; 3x6x6: 4-byte path; 1x5x5: scalar path
SEQ_LENGTHS = (5, 20)


def dequant(q: np.ndarray) -> np.ndarray:
    return (q.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


def make_arena(per_frame: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """Episodes back to back; an episode marked `end` or `trunc` has a final frame (the collector's rule), the others have none."""
    rng = np.random.RandomState(seed)
    total = sum(n for n, _ in EPISODES)
    a = {"frames": rng.randint(0, 256, (total, per_frame)).astype(np.uint8), "act": rng.randint(0, 18, total).astype(np.int64),
         "rew": rng.randint(-3, 4, total).astype(np.float32) * np.float32(0.5), "end": np.zeros(total, np.uint8),
         "trunc": np.zeros(total, np.uint8)}
    first, lens, final_row = [], [], []
    at = 0
    for n, last in EPISODES:
        first.append(at)
        lens.append(n)
        if last != "none":
            a[last][at + n - 1] = 1
            final_row.append(sum(r >= 0 for r in final_row))
        else:
            final_row.append(-1)
        at += n
    a["finals"] = rng.randint(0, 256, (sum(r >= 0 for r in final_row), per_frame)).astype(np.uint8)
    a["first"], a["len"], a["final_row"] = (np.array(v, np.int64) for v in (first, lens, final_row))
    return a


def levels_arena() -> Dict[str, np.ndarray]:
    """per_frame = 256 and EVERY frame a permutation of the 256 levels: the dequantisation of each level, at every lane position."""
    a = make_arena(256, seed=4)
    for name in ("frames", "finals"):
        for r in range(len(a[name])):
            a[name][r] = (np.arange(256) * (2 * r + 1) + 3 * r) % 256  # an odd multiplier permutes 0 ... 255
    return a


def all_segments(arena: Dict[str, np.ndarray], t: int) -> np.ndarray:
    """(n, 4) descriptor rows of EVERY segment of T steps that overlaps an episode: starts -(T - 1) ... len - 1, i.e. all but one
    position left-padded, right-padded, padded on both sides (short episodes) and unpadded."""
    rows = [(f, s, n, r) for f, n, r in zip(arena["first"], arena["len"], arena["final_row"]) for s in range(-(t - 1), n)]
    return np.array(rows, np.int64)


def batches(seg: np.ndarray, size: int = 37) -> Iterator[np.ndarray]:
    """B = 1 (the first and the last row alone), then batches of 37 in a fixed shuffled order (the last one may be shorter)."""
    yield seg[:1]
    yield seg[-1:]
    order = np.random.RandomState(5).permutation(len(seg))
    for i in range(0, len(seg), size):
        yield seg[order[i:i + size]]


def restate(arena: Dict[str, np.ndarray], seg: np.ndarray, t: int, flag_dtype, put_back_final: bool) -> Dict[str, np.ndarray]:
    b, pf = len(seg), arena["frames"].shape[1]
    out = {"obs": np.zeros((b, t, pf), np.float32), "act": np.zeros((b, t), np.int64), "rew": np.zeros((b, t), np.float32),
           "end": np.zeros((b, t), flag_dtype), "trunc": np.zeros((b, t), flag_dtype), "mask_padding": np.zeros((b, t), np.uint8),
           "final_obs": np.zeros((b, pf), np.float32)}
    for i, (first, start, n, row) in enumerate(seg):
        for k in range(t):
            s = start + k
            if 0 <= s < n:
                j = first + s
                out["obs"][i, k] = dequant(arena["frames"][j])
                out["act"][i, k], out["rew"][i, k] = arena["act"][j], arena["rew"][j]
                out["end"][i, k], out["trunc"][i, k] = arena["end"][j], arena["trunc"][j]
                out["mask_padding"][i, k] = 1
            elif put_back_final and s == n and k >= 1 and row >= 0 and arena["end"][first + n - 1] != 0:
                out["obs"][i, k] = dequant(arena["finals"][row])
        if row >= 0:
            out["final_obs"][i] = dequant(arena["finals"][row])
    return out


def bits(x: np.ndarray) -> np.ndarray:
    """Raw bytes, so that -0.0 / NaN payloads / dtypes all count in a comparison."""
    return np.ascontiguousarray(x).view(np.uint8)


def assert_same(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray], keys: Tuple[str, ...], what: str) -> None:
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if not np.array_equal(bits(got[k]), bits(want[k])):
            same = (bits(got[k]).reshape(got[k].shape + (-1,)) == bits(want[k]).reshape(want[k].shape + (-1,))).all(-1)
            bad = np.argwhere(~same)
            raise AssertionError(f"{what}: {k} differs from the restatement at {len(bad)} elements, first {bad[:3].tolist()}: "
                                 f"{got[k][tuple(bad[0])]!r} for {want[k][tuple(bad[0])]!r}")


OUTPUTS = ("obs", "act", "rew", "end", "trunc", "mask_padding", "final_obs")
