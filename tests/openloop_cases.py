"""Shared by tests/test_openloop_simt.py and tests/test_gpu_openloop.py: a small arena, the descriptor rows of every kind of
sample dmd_openloop_step distinguishes, predictions that sit on / beside / outside the level grid, and an fp32 / int64 numpy
RESTATEMENT of the entry point written from its contract in include/diamond_hip.h:

    s = start + T + step is the predicted frame's episode step, j = s - 1 its transition.  The frame's target is arena row
    first + s when 0 <= s < len, the final observation when s == len, final_row >= 0 and the episode's last step has end != 0,
    and otherwise there is none (invalid: zero metrics).  q = clip(rint((v + 1) / 2 * 255), 0, 255) in fp32, d = q - target;
    metrics = sum d^2, sum |d|, max |d|, count d != 0.  rew / end of transition j when 0 <= j < len, else zeros.  Ring slot `head`
    takes the prediction, or with teacher_forced and a valid frame (target / 255) * 2 - 1; the action slot act[first + s] or 0.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from tests.replay_cases import dequant

T = 4
PER_FRAMES = (48, 20, 7)  # 16 levels per lane; 4 levels per lane; one level per lane
# (length, last step has end != 0, has a final observation)
EPISODES = ((12, False, False), (6, True, True), (6, True, False), (5, False, True))
STEP = 1
# (episode, start, kind) at step 1: s = start + 5
SAMPLES = (
    (0, 2, "inside"),                      # s = 7
    (0, -3, "left padding"),               # s = 2: part of the context was padding
    (1, 1, "final observation"),           # s = 6 = len, the episode ended and kept its final frame: frame valid, no next action
    (2, 1, "end without a final frame"),   # s = 6 = len, final_row = -1: frame invalid, transition valid
    (1, 3, "beyond the end"),              # s = 8: both invalid
    (3, 0, "final frame without an end"),  # s = 5 = len, a final frame exists but the last step has end = 0: frame invalid
    (0, -5, "first step"),                 # s = 0: frame valid, no transition leads into it
    (0, -6, "before the episode"),         # s = -1: both invalid
    (0, 4, "equal to its target"),         # s = 9, the prediction IS the recording: four zeros
)
KINDS = tuple(k for _, _, k in SAMPLES)


def make_arena(per_frame: int, seed: int = 0) -> Dict[str, np.ndarray]:
    rng = np.random.RandomState(seed)
    total = sum(n for n, _, _ in EPISODES)
    a = {"frames": rng.randint(0, 256, (total, per_frame)).astype(np.uint8), "act": rng.randint(1, 18, total).astype(np.int64),
         "rew": (rng.randint(-2, 3, total).astype(np.float32) * np.float32(0.5)), "end": np.zeros(total, np.uint8)}
    a["rew"][a["rew"] == 0] = np.float32(0.25)  # (no recorded value equals the zeros of an invalid transition)
    first, final_row, at, rows = [], [], 0, 0
    for n, ends, final in EPISODES:
        first.append(at)
        if ends:
            a["end"][at + n - 1] = 1
        final_row.append(rows if final else -1)
        rows += int(final)
        at += n
    a["finals"] = rng.randint(0, 256, (rows, per_frame)).astype(np.uint8)
    a["first"], a["len"], a["final_row"] = np.array(first, np.int64), np.array([n for n, _, _ in EPISODES], np.int64), np.array(final_row, np.int64)
    return a


def descriptor(arena: Dict[str, np.ndarray]) -> np.ndarray:
    return np.array([(arena["first"][e], start, arena["len"][e], arena["final_row"][e]) for e, start, _ in SAMPLES], np.int64)


def target_of(arena: Dict[str, np.ndarray], row: np.ndarray, t: int, step: int):
    first, start, n, final_row = (int(v) for v in row)
    s = start + t + step
    if 0 <= s < n:
        return arena["frames"][first + s]
    if s == n and final_row >= 0 and len(arena["finals"]) and arena["end"][first + n - 1] != 0:
        return arena["finals"][final_row]
    return None


def predictions(arena: Dict[str, np.ndarray], seg: np.ndarray, t: int, step: int, seed: int = 1, equal_rows=()) -> np.ndarray:
    """Per value one of: an exact grid value, a grid value +- 0.499 of a level, a value outside [-1, 1] -- at levels near the
    target's (small differences, zeros among them) or anywhere; the samples `equal_rows` are their dequantised targets."""
    rng = np.random.RandomState(seed)
    pf = arena["frames"].shape[1]
    pred = np.empty((len(seg), pf), np.float32)
    for b, row in enumerate(seg):
        tgt = target_of(arena, row, t, step)
        base = rng.randint(0, 256, pf) if tgt is None else tgt.astype(np.int64)
        near = np.clip(base + rng.randint(-2, 3, pf), 0, 255)
        level = np.where(rng.rand(pf) < 0.5, near, rng.randint(0, 256, pf)).astype(np.float64)
        kind = rng.randint(0, 4, pf)
        level = level + np.where(kind == 1, 0.499, 0.0) - np.where(kind == 2, 0.499, 0.0)
        v = (level / 255.0) * 2.0 - 1.0
        v = np.where(kind == 3, np.where(rng.rand(pf) < 0.5, -1.0 - rng.rand(pf) * 3, 1.0 + rng.rand(pf) * 3), v)
        pred[b] = v.astype(np.float32)
        if b in equal_rows and tgt is not None:
            pred[b] = dequant(tgt)
    return pred


def levels_of(v: np.ndarray) -> np.ndarray:
    v = v.astype(np.float32)
    lv = np.rint((v + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0))
    return np.clip(lv, np.float32(0.0), np.float32(255.0)).astype(np.int64)


def make_case(per_frame: int, head: int, step: int = STEP, seed: int = 0) -> Dict[str, np.ndarray]:
    arena = make_arena(per_frame, seed)
    seg = descriptor(arena)
    rng = np.random.RandomState(seed + 100)
    return {"arena": arena, "seg": seg, "T": T, "head": head, "step": step,
            "pred": predictions(arena, seg, T, step, seed + 1, equal_rows=(KINDS.index("equal to its target"),)),
            "ctx_obs": rng.randn(len(seg), T, per_frame).astype(np.float32), "ctx_act": rng.randint(20, 40, (len(seg), T)).astype(np.int64)}


def rows_of(case: Dict[str, np.ndarray], rows) -> Dict[str, np.ndarray]:
    """The same case restricted to some samples."""
    out = dict(case)
    for k in ("seg", "pred", "ctx_obs", "ctx_act"):
        out[k] = np.ascontiguousarray(case[k][rows])
    return out


def restate(case: Dict[str, np.ndarray], teacher_forced: bool) -> Dict[str, np.ndarray]:
    arena, seg, t, head, step, pred = (case[k] for k in ("arena", "seg", "T", "head", "step", "pred"))
    b, pf = pred.shape
    out = {"metrics": np.zeros((b, 4), np.int64), "rew": np.zeros(b, np.float32), "end": np.zeros(b, np.uint8), "valid": np.zeros((b, 2), np.uint8),
           "levels": np.zeros((b, pf), np.uint8), "ctx_obs": case["ctx_obs"].copy(), "ctx_act": case["ctx_act"].copy()}
    for i, row in enumerate(seg):
        first, start, n, _ = (int(v) for v in row)
        s = start + t + step
        j = s - 1
        q = levels_of(pred[i])
        out["levels"][i] = q.astype(np.uint8)
        tgt = target_of(arena, row, t, step)
        out["ctx_obs"][i, head] = pred[i]
        if tgt is not None:
            d = np.abs(q - tgt.astype(np.int64))
            out["metrics"][i] = (int((d * d).sum()), int(d.sum()), int(d.max()), int((d != 0).sum()))
            out["valid"][i, 0] = 1
            if teacher_forced:
                out["ctx_obs"][i, head] = dequant(tgt)
        if 0 <= j < n:
            out["rew"][i], out["end"][i], out["valid"][i, 1] = arena["rew"][first + j], arena["end"][first + j], 1
        out["ctx_act"][i, head] = arena["act"][first + s] if 0 <= s < n else 0
    return out


OUTPUTS = ("metrics", "rew", "end", "valid", "levels", "ctx_obs", "ctx_act")
# what the kinds must come out as: (frame valid, transition valid)
EXPECTED_VALID = {"inside": (1, 1), "left padding": (1, 1), "final observation": (1, 1), "end without a final frame": (0, 1),
                  "beyond the end": (0, 0), "final frame without an end": (0, 1), "first step": (1, 0), "before the episode": (0, 0),
                  "equal to its target": (1, 1)}


# ---- the composition: what open_loop_eval replaces (tests/test_gpu_openloop.py, tools/openloop_bench.py) ----------------------------
def device_levels(x):
    """The uint8 levels of a device tensor through dmd_quantize_u8 (an entry point that existed before dmd_openloop_step)."""
    import torch

    from diamond_amd import native as nv

    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    nv.check(nv.lib().dmd_quantize_u8(nv.fptr(x), nv.ptr(q), nv.ptr(flag), x.numel(), nv.stream()), "dmd_quantize_u8")
    return q


def reference_loop(sampler, rew_end_model, store, ids, t, horizon, teacher_forced):
    """open_loop_eval written with the entry points that existed before it: `gather` of the whole segment as fp32, sample_ring,
    predict_rew_end, dmd_quantize_u8, torch integer ops and boolean masks, explicit ring writes.  Returns (fields stacked to
    (B, horizon, ...), ctx_obs, ctx_act, head)."""
    import torch

    batch = store.gather(ids, put_back_final=True, info=False)  # the WHOLE segment as fp32, the final observations put back
    has_final = torch.tensor([store._final_row[e] >= 0 for e, _, _ in ids], device=store.device)
    mask, b = batch.mask_padding, len(ids)
    ctx_obs, ctx_act = batch.obs[:, :t].clone(), batch.act[:, :t].clone()
    *_, hx_cx = rew_end_model.predict_rew_end(ctx_obs[:, :-1], ctx_act[:, :-1], ctx_obs[:, 1:])
    out = {k: [] for k in ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true",
                           "end_true", "levels")}
    head = 0
    for i in range(horizon):
        pred, _ = sampler.sample_ring(ctx_obs, ctx_act, head, head)
        newest = (head - 1) % t
        l_rew, l_end, hx_cx = rew_end_model.predict_rew_end(ctx_obs[:, newest:newest + 1], ctx_act[:, newest:newest + 1], pred, hx_cx)
        k = t + i
        tv = mask[:, k - 1]
        fv = mask[:, k] | (~mask[:, k] & tv & batch.end[:, k - 1].bool() & has_final)
        q = device_levels(pred)
        d = (q.long() - device_levels(batch.obs[:, k]).long()).abs().reshape(b, -1) * fv[:, None]
        for name, val in (("sq_err", (d * d).sum(1)), ("abs_err", d.sum(1)), ("max_err", d.max(1).values), ("pixels_off", (d != 0).sum(1)),
                          ("frame_valid", fv), ("transition_valid", tv), ("logits_rew", l_rew[:, 0]), ("logits_end", l_end[:, 0]),
                          ("rew_true", batch.rew[:, k - 1]), ("end_true", batch.end[:, k - 1]), ("levels", q)):
            out[name].append(val)
        new = torch.where(fv[:, None, None, None], batch.obs[:, k], pred) if teacher_forced else pred
        ctx_obs[:, head] = new
        ctx_act[:, head] = batch.act[:, k]
        head = (head + 1) % t
    return {k: torch.stack(v, dim=1) for k, v in out.items()}, ctx_obs, ctx_act, head
