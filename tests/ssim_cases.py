"""Shared by tests/test_ssim_simt.py and tests/test_gpu_ssim.py: shapes, operand pairs, an arena descriptor with every kind of
row dmd_frame_ssim distinguishes, and an fp64 numpy RESTATEMENT of the entry point written from its contract in
include/diamond_hip.h -- as the DIRECT sum over the 121 taps of every position (weights win[i] * win[j], tap after tap in
row-major order), on purpose another summation order than the kernel's separable one:

    mx = sum w x, my = sum w y, sxx = sum w x^2 - mx^2, syy = sum w y^2 - my^2, sxy = sum w x y - mx my
    cs = (2 sxy + C2) / (sxx + syy + C2),  ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs,  out[n] = (mean ssim, mean cs)

TOL: the two orders differ by rounding only.  Per position the second moments cancel to an absolute error of at most about
65025 * 121 * 1.1e-16 = 9e-10 against denominators of at least C2 = 58.5, i.e. about 1.5e-11 per ratio; 1e-10 absolute holds for
every comparison against the restatement.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from tests import openloop_cases as OC

TAPS = 11
S = 16  # the kernel's tile edge (SSIM_S in diamond_amd/csrc/dmd_pointwise.hip): positions per workgroup and axis
TOL = 1e-10
T, STEP = OC.T, OC.STEP

SMALL_SHAPES = ((1, 1, 11, 11), (2, 1, 12, 13), (3, 3, 24, 20))  # one position; per_frame 156 with unaligned rows; several channels
EDGE_SHAPES = tuple((1, 1, h, w) for h in (S + 9, S + 10, S + 11) for w in (S + 9, S + 10, S + 11))  # S - 1, S, S + 1 positions per axis
PAIRS = ("random", "plus minus 2", "identical", "constants", "0 against 255", "255 against 254")
CONST_A, CONST_B = 200, 37


def window(sigma: float = 1.5) -> np.ndarray:
    g = np.exp(-((np.arange(TAPS, dtype=np.float64) - TAPS // 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def restate(a: np.ndarray, b: np.ndarray, win: np.ndarray = None, c1: float = C1, c2: float = C2) -> np.ndarray:
    """(N, 2) fp64 from two (N, C, H, W) arrays of levels: the 121-tap sum per position."""
    win = window() if win is None else win
    w2 = np.outer(win, win)
    x, y = a.astype(np.float64), b.astype(np.float64)
    view = lambda v: np.lib.stride_tricks.sliding_window_view(v, (TAPS, TAPS), axis=(2, 3))  # (N, C, H - 10, W - 10, 11, 11)
    mom = lambda v: np.einsum("nchwij,ij->nchw", view(v), w2)  # (no (..., 11, 11) temporary: a 256 x 256 frame stays cheap)
    mx, my = mom(x), mom(y)
    sxx, syy, sxy = mom(x * x) - mx * mx, mom(y * y) - my * my, mom(x * y) - mx * my
    cs = (2.0 * sxy + c2) / (sxx + syy + c2)
    ssim = (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    n = a.shape[0]
    return np.stack([ssim.reshape(n, -1).mean(1), cs.reshape(n, -1).mean(1)], axis=1)


def pair(kind: str, shape, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "random":
        return a, rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "plus minus 2":
        return a, np.clip(a.astype(np.int64) + rng.randint(-2, 3, shape), 0, 255).astype(np.uint8)
    if kind == "identical":
        return a, a.copy()
    full = lambda v: np.full(shape, v, np.uint8)
    return {"constants": (full(CONST_A), full(CONST_B)), "0 against 255": (full(0), full(255)), "255 against 254": (full(255), full(254))}[kind]


def check_pair(kind: str, got: np.ndarray, a: np.ndarray, b: np.ndarray) -> float:
    """What every operand pair must satisfy; returns the largest difference from the restatement."""
    want = restate(a, b)
    err = float(np.abs(got - want).max())
    assert err <= TOL, (kind, a.shape, err)
    if kind == "identical":  # x and y go through identical operations
        assert (got == 1.0).all(), (kind, got)
    if kind == "constants":
        ca, cb = float(CONST_A), float(CONST_B)
        assert np.abs(got[:, 0] - (2 * ca * cb + C1) / (ca * ca + cb * cb + C1)).max() <= TOL and np.abs(got[:, 1] - 1.0).max() <= TOL, got
    return err


def off_grid(shape, seed: int = 0) -> np.ndarray:
    """fp32 values on the level grid, +- 0.499 of a level beside it, and outside [-1, 1] (tests/openloop_cases.py `predictions`)."""
    rng = np.random.RandomState(seed)
    level = rng.randint(0, 256, shape).astype(np.float64)
    kind = rng.randint(0, 4, shape)
    level = level + np.where(kind == 1, 0.499, 0.0) - np.where(kind == 2, 0.499, 0.0)
    v = (level / 255.0) * 2.0 - 1.0
    v = np.where(kind == 3, np.where(rng.rand(*shape) < 0.5, -1.0 - rng.rand(*shape) * 3, 1.0 + rng.rand(*shape) * 3), v)
    return v.astype(np.float32)


def dequant(levels: np.ndarray) -> np.ndarray:
    return (levels.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)


# ---- arena mode: the episodes of tests/openloop_cases.py (lengths 12, 6, 6, 5; 1 and 2 end; 1 and 3 have a final frame) -----------
# (episode, start, kind, has a target) at T = 4, step = 1: s = start + 5
ARENA_SAMPLES = (
    (0, -6, "left padding", False),                 # s = -1
    (0, 2, "inside", True),                         # s = 7
    (3, -1, "the arena's last row", True),          # s = 4, episode 3 is the arena's last and 5 long
    (1, 1, "final observation", True),              # s = 6 = len behind an end, with a final frame
    (2, 1, "end without a final frame", False),     # s = 6 = len, final_row = -1
    (3, 0, "final frame without an end", False),    # s = 5 = len, the last step has end = 0
    (0, 7, "len without end or final", False),      # s = 12 = len
    (1, 3, "past the episode", False),              # s = 8
)


def arena_case(frame, seed: int = 0) -> Dict[str, np.ndarray]:
    """An arena of frames of shape `frame` = (C, H, W), the descriptor of ARENA_SAMPLES and a prediction per sample."""
    pf = int(np.prod(frame))
    arena = OC.make_arena(pf, seed)
    seg = np.array([(arena["first"][e], start, arena["len"][e], arena["final_row"][e]) for e, start, _, _ in ARENA_SAMPLES], np.int64)
    a = np.random.RandomState(seed + 7).randint(0, 256, (len(seg),) + tuple(frame)).astype(np.uint8)
    return {"arena": arena, "seg": seg, "a": a, "frame": tuple(frame)}


def arena_targets(case, step: int = STEP, finals: bool = True):
    """(valid mask, the valid samples' targets (n_valid, C, H, W))."""
    arena = case["arena"] if finals else dict(case["arena"], finals=case["arena"]["finals"][:0])
    tg = [OC.target_of(arena, row, T, step) for row in case["seg"]]
    valid = np.array([t is not None for t in tg])
    return valid, np.stack([t.reshape(case["frame"]) for t in tg if t is not None]) if valid.any() else np.zeros((0,) + case["frame"], np.uint8)
