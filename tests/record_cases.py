"""Shared by tests/test_record_window.py and the collector tests: windows, arenas, run tables and a numpy RESTATEMENT of
dmd_record_window (include/diamond_hip.h), written from the entry's contract:

    a run (kind, src, n, dst) writes n rows.  kind 0: window steps src ... src + n - 1 -> arena rows dst ..., frames as levels
    clamp(rint((v + 1) / 2 * 255), 0, 255) in fp32, act / rew copied, end / trunc as (value != 0).  kind 1: final_obs[src] ->
    finals[dst] as levels.  kind 2: arena rows src ... -> arena rows dst ..., all five fields byte for byte.  off_grid is 1 iff
    some quantised value v is not (level / 255) * 2 - 1 in fp32.  Every other byte of the destinations stays what it was.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests.replay_cases import bits, dequant

PER_FRAMES = (192, 108, 25)  # 3x8x8: four 16-byte loads per lane; 3x6x6: one; 1x5x5: one level per lane
B, T = 6, 8                  # the window of the mixed cases: 48 steps
RUN_COUNTS = (1, 2, 3, 5, 37)
POISON = 0x5A
ARENA = ("frames", "act", "rew", "end", "trunc", "finals")
F32 = np.float32


def level(v: np.ndarray) -> np.ndarray:
    """dmd_level: fminf(fmaxf(rintf((v + 1) / 2 * 255), 0), 255) -- fmax / fmin drop a NaN operand, as the C functions do"""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lv = np.rint((v + F32(1)) / F32(2) * F32(255))
    return np.fmin(np.fmax(lv, F32(0)), F32(255)).astype(F32)


def on_grid(v: np.ndarray) -> bool:
    lv = level(v)
    return bool(((lv / F32(255)) * F32(2) - F32(1) == np.asarray(v, F32)).all())


def poisoned(shape, dtype) -> np.ndarray:
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = POISON
    return a


def make_window(per_frame: int, flag_dtype, seed: int, b: int = B, t: int = T, k: int = 8) -> Dict[str, np.ndarray]:
    """The env loop's stacked tensors, flattened to (b * t, ...): frames on the grid, flags with values other than 0 / 1 too."""
    rng = np.random.RandomState(seed)
    n = b * t
    flags = rng.randint(0, 4, (2, n)) * (rng.rand(2, n) < 0.4)
    if np.dtype(flag_dtype).itemsize == 8:
        flags = flags * (1 << 40)  # (a value whose low byte is 0: the whole element counts)
    return {"obs": dequant(rng.randint(0, 256, (n, per_frame)).astype(np.uint8)), "act": rng.randint(0, 18, n).astype(np.int64),
            "rew": (rng.randint(-4, 5, n) * 0.5).astype(F32), "end": flags[0].astype(flag_dtype), "trunc": flags[1].astype(flag_dtype),
            "final_obs": dequant(rng.randint(0, 256, (k, per_frame)).astype(np.uint8)), "steps": n, "K": k}


def candidate_runs(b: int = B, t: int = T, k: int = 8) -> List[Tuple[int, int, int]]:
    """(kind, src, n) in the order the cases take them: a whole env (n = T); an episode of 5 rows MOVED (arena rows 1 ... 5) and
    2 steps of env 1 appended behind it; a final observation; then the other envs cut into runs of 1 and 2 steps with the
    final observations between them.  39 candidates."""
    runs = [(0, 0, t), (2, 1, 5), (0, 1 * t, 2), (1, 0, 1)]
    finals = list(range(1, k))
    for env in range(2, b):
        at = 0
        for n in (1, 2, 1, 2, 1, 1):
            runs.append((0, env * t + at, n))
            at += n
            if finals and n == 2:
                runs.append((1, finals.pop(0), 1))
    at = 2
    for n in (1, 2, 1, 2):
        runs.append((0, 1 * t + at, n))
        at += n
    return runs


def make_case(per_frame: int, flag_dtype, r: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """A window, a poisoned arena whose rows 1 ... 5 hold an episode, and the first `r` candidate runs with destinations handed out
    front to back with gaps of 0, 1, 2 rows (the gaps, the rows in front and behind stay poisoned); a kind-0 run that follows the
    move lands directly behind the moved rows, as an episode that moves and grows in one window."""
    w = make_window(per_frame, flag_dtype, seed + 7 * r)
    c = {"window": w, "steps": w["steps"], "K": w["K"]}
    rng = np.random.RandomState(seed + 1)
    table, at, fat = [], 8, 1
    for i, (kind, src, n) in enumerate(candidate_runs()[:r]):
        if kind == 1:
            table.append((1, src, 1, fat))
            fat += 1 + i % 2
        else:
            table.append((kind, src, n, at))
            at += n + (0 if kind == 2 else i % 3)
    f, e = at + 2, fat + 1
    arena = {"frames": poisoned((f, per_frame), np.uint8), "act": poisoned(f, np.int64), "rew": poisoned(f, F32), "end": poisoned(f, np.uint8),
             "trunc": poisoned(f, np.uint8), "finals": poisoned((e, per_frame), np.uint8)}
    arena["frames"][1:6] = rng.randint(0, 256, (5, per_frame))
    arena["act"][1:6], arena["rew"][1:6] = rng.randint(0, 18, 5), rng.randn(5).astype(F32)
    arena["end"][1:6], arena["trunc"][1:6] = 0, (0, 0, 1, 0, 0)
    c.update(arena)
    c.update(runs=np.array(table, np.int64).reshape(-1, 4), per_frame=per_frame, F=f, E=e)
    return c


def levels_case(per_frame: int) -> Dict[str, np.ndarray]:
    """256 steps (4 envs x 64) whose frame s holds level (i + s) % 256 at position i: every level at every position of a frame,
    i.e. at every lane, word slot and byte of a word; one run per env (n = T = 64)."""
    w = make_window(per_frame, np.uint8, 3, b=4, t=64, k=0)
    c = {"window": w, "steps": w["steps"], "K": w["K"]}
    q = ((np.arange(per_frame)[None, :] + np.arange(256)[:, None]) % 256).astype(np.uint8)
    w["obs"] = dequant(q)
    c.update(frames=poisoned((258, per_frame), np.uint8), act=poisoned(258, np.int64), rew=poisoned(258, F32), end=poisoned(258, np.uint8),
             trunc=poisoned(258, np.uint8), finals=poisoned((1, per_frame), np.uint8), per_frame=per_frame, F=258, E=1,
             runs=np.array([(0, 64 * b, 64, 1 + 64 * b) for b in range(4)], np.int64))
    c["levels"] = q
    return c


def restate(c: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    out = {k: c[k].copy() for k in ARENA}
    w = c["window"]
    flag = 0
    moved = {k: c[k].copy() for k in ARENA}  # a kind-2 run reads what the arena held before the launch
    for kind, src, n, dst in c["runs"]:
        if kind == 0:
            v = w["obs"][src:src + n]
            out["frames"][dst:dst + n] = level(v).astype(np.uint8)
            flag |= not on_grid(v)
            out["act"][dst:dst + n], out["rew"][dst:dst + n] = w["act"][src:src + n], w["rew"][src:src + n]
            out["end"][dst:dst + n], out["trunc"][dst:dst + n] = w["end"][src:src + n] != 0, w["trunc"][src:src + n] != 0
        elif kind == 1:
            assert n == 1
            out["finals"][dst] = level(w["final_obs"][src]).astype(np.uint8)
            flag |= not on_grid(w["final_obs"][src])
        else:
            for k in ("frames", "act", "rew", "end", "trunc"):
                out[k][dst:dst + n] = moved[k][src:src + n]
    out["off_grid"] = np.array([int(flag)], np.int32)
    return out


def assert_same(got: Dict[str, np.ndarray], want: Dict[str, np.ndarray], what: str) -> None:
    for k in ARENA + ("off_grid",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if not np.array_equal(bits(got[k]), bits(want[k])):
            same = (bits(got[k]).reshape(got[k].shape + (-1,)) == bits(want[k]).reshape(want[k].shape + (-1,))).all(-1)
            bad = np.argwhere(~same)
            raise AssertionError(f"{what}: {k} differs from the restatement at {len(bad)} elements, first {bad[:3].tolist()}: "
                                 f"{got[k][tuple(bad[0])]!r} for {want[k][tuple(bad[0])]!r}")
