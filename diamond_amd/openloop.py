"""Open-loop evaluation of the world model against recorded episodes in a DeviceReplay: how far does a rollout drift?

The two training losses (Denoiser.forward, RewEndModel.forward) are single-step quantities averaged over noise levels.  This is the
report world-model code bases ship beside them: start from a REAL context of T = num_steps_conditioning frames, feed the RECORDED
actions, and compare what the model imagines with what happened, step by step -- free running (the model's own frames go back into
its context, as in imagination) or teacher forced (the recorded frame does: one-step errors at every horizon).

    from diamond_amd.openloop import open_loop_eval
    report = open_loop_eval(sampler, agent.rew_end_model, store, ids, horizon=15)      # nothing is read back yet
    print(report.summary())                                                            # the one wait

Per evaluated step: `DiffusionSampler.sample_ring` over the context rings, `RewEndModel.predict_rew_end` on (newest frame, its action,
prediction) with the carried LSTM state (what WorldModelEnv does per imagined step), then ONE `dmd_openloop_step` launch that
compares the prediction with the arena's uint8 levels (exact integer metrics), looks up the recorded reward / end, and advances the
rings from the prediction or from the recording.  No fp32 copy of the target frames, no boolean masks, no host synchronisation.
With `ssim=True` one dmd_frame_ssim call per step more: the prediction's SSIM against the same arena frame (diamond_amd/metrics.py).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence

import torch
from torch import Tensor

from . import native as nv
from .metrics import set_operand, ssim_params, ssim_workspace
from .replay import DeviceReplay, _id_fields
from .rew_end_model import confusion_matrix


@dataclass
class OpenLoopReport:
    """Device tensors, (B, horizon, ...): column i is evaluated step i, the frame T + i of each segment."""
    sq_err: Tensor            # int64, in uint8 levels: sum d^2 over the frame, d = level(prediction) - recorded level
    abs_err: Tensor           # int64: sum |d|
    max_err: Tensor           # int64: max |d|
    pixels_off: Tensor        # int64: values with d != 0
    frame_valid: Tensor       # bool: the episode recorded this frame (a step, or the final observation after an end)
    transition_valid: Tensor  # bool: the episode recorded the transition into it (reward, end)
    logits_rew: Tensor        # (B, horizon, 3)
    logits_end: Tensor        # (B, horizon, 2)
    rew_true: Tensor          # fp32, 0 where the transition is not valid
    end_true: Tensor          # the store's flag dtype, 0 where the transition is not valid
    levels: Optional[Tensor]  # (B, horizon, C, H, W) uint8: the predictions as levels (return_levels), else None
    ctx_obs: Tensor           # (B, T, C, H, W): the context ring after the last step
    ctx_act: Tensor           # (B, T)
    head: int                 # the rings' oldest slot after the last step
    per_frame: int
    ssim: Optional[Tensor] = None     # (B, horizon) fp64: mean SSIM of the frame (open_loop_eval(ssim=True)), nan where not frame_valid
    ssim_cs: Optional[Tensor] = None  # (B, horizon) fp64: its contrast-structure term alone

    def summary(self) -> Dict[str, Any]:
        """Plain Python numbers (this is where the host waits for the device), one entry per evaluated step over the samples
        whose frame / transition is valid there: `mse` in [-1, 1] units (formed in fp64 from the integer sums), `psnr` in dB
        (peak-to-peak 2; inf for an exact match), `pixels_off` as a share of the values, the worst `max_err` in levels, and the
        reward (3 x 3) / end (2 x 2) confusion matrices of the argmax predictions (rows: recorded class, sign(rew) + 1 / end).
        A step without valid samples has nan.  With the ssim fields: `ssim` and `ssim_cs`, the fp64 means over the valid frames."""
        cpu = {k: getattr(self, k).cpu() for k in ("sq_err", "pixels_off", "max_err", "frame_valid", "transition_valid", "logits_rew",
                                                   "logits_end", "rew_true", "end_true")}
        fv, tv = cpu["frame_valid"], cpu["transition_valid"]
        n = fv.sum(0).double() * self.per_frame  # values compared per step
        mse = (cpu["sq_err"] * fv).sum(0).double() / n * (2.0 / 255.0) ** 2
        off = (cpu["pixels_off"] * fv).sum(0).double() / n
        psnr = [float("nan") if math.isnan(m) else (float("inf") if m == 0 else 10.0 * math.log10(4.0 / m)) for m in mse.tolist()]
        rew_class = torch.sign(cpu["rew_true"]).long() + 1
        horizon = fv.shape[1]
        cm_rew = [confusion_matrix(cpu["logits_rew"][tv[:, i], i], rew_class[tv[:, i], i], 3).tolist() for i in range(horizon)]
        cm_end = [confusion_matrix(cpu["logits_end"][tv[:, i], i], cpu["end_true"][tv[:, i], i], 2).tolist() for i in range(horizon)]
        out = {"horizon": horizon, "valid_frames": fv.sum(0).tolist(), "valid_transitions": tv.sum(0).tolist(), "mse": mse.tolist(),
               "psnr": psnr, "pixels_off": off.tolist(), "max_err": (cpu["max_err"] * fv).max(0).values.tolist(),
               "confusion_matrix_rew": cm_rew, "confusion_matrix_end": cm_end}
        for k in ("ssim", "ssim_cs"):
            if getattr(self, k) is not None:
                v = getattr(self, k).cpu().double()
                out[k] = (torch.where(fv, v, torch.zeros_like(v)).sum(0) / fv.sum(0).double()).tolist()  # 0 / 0: nan
        return out


def _launch_step(store: DeviceReplay, seg: Tensor, pred: Tensor, ctx_obs: Tensor, ctx_act: Tensor, step: int, head: int,
                 teacher_forced: bool, metrics: Tensor, rew: Tensor, end: Tensor, valid: Tensor, levels: Optional[Tensor]) -> None:
    p = nv.OpenLoopParams()
    p.B, p.T, p.per_frame = ctx_act.shape[0], ctx_act.shape[1], store.per_frame
    p.step, p.head, p.teacher_forced = step, head, int(bool(teacher_forced))
    p.frames, p.act, p.rew, p.end, p.finals = (nv.ptr(x) for x in (store.frames, store.act, store.rew, store.end, store.finals))
    p.seg, p.pred, p.ctx_obs, p.ctx_act = nv.ptr(seg), nv.fptr(pred), nv.fptr(ctx_obs), nv.ptr(ctx_act)
    p.metrics, p.out_rew, p.out_end, p.out_valid, p.out_levels = (nv.ptr(x) for x in (metrics, rew, end, valid, levels))
    nv.check(nv.lib().dmd_openloop_step(C.byref(p), nv.stream()), "dmd_openloop_step")


def _launch_ssim(p: nv.SsimParams, store: DeviceReplay, seg: Tensor, pred: Tensor, t: int, step: int, work: Tensor, out: Tensor) -> None:
    """SSIM of `pred` against the arena frame dmd_openloop_step compares it with (the same seg, T and step) -> out (B, 2)."""
    set_operand(p, "a", pred)
    p.frames, p.finals, p.end, p.seg = (nv.ptr(x) for x in (store.frames, store.finals, store.end, seg))
    p.T, p.step = t, step
    p.workspace, p.out = nv.ptr(work), nv.ptr(out)
    nv.check(nv.lib().dmd_frame_ssim(C.byref(p), nv.stream()), "dmd_frame_ssim")


@torch.no_grad()
def open_loop_eval(sampler, rew_end_model, store: DeviceReplay, ids: Sequence[Any], horizon: int, *, teacher_forced: bool = False,
                   return_levels: bool = False, ssim: bool = False) -> OpenLoopReport:
    """Roll the world model `horizon` steps along the recorded segments `ids` and report, per step, how the imagined frames and
    the reward / end predictions compare with the recording.
    sampler: a DiffusionSampler (its `noise_fn` hook injects the draws); rew_end_model: a RewEndModel; store: a DeviceReplay.
    ids: (episode_id, start, stop), SegmentId-like or tuples, stop - start == T + horizon with T = the denoiser's
    num_steps_conditioning: the first T steps are the context, the rest is evaluated.  Validated on the host by the store's
    descriptor code before anything is launched (ValueError); left padding (start < 0) and segments that run past the episode's
    end are allowed as in `gather` -- what the episode did not record is flagged invalid, never compared.
    teacher_forced: the context advances with the RECORDED frame where there is one (free running: with the prediction).
    return_levels: keep the predictions as uint8 levels (for videos).
    ssim: also the per-frame SSIM of every prediction against its recorded frame (one dmd_frame_ssim call per step, fp64, against
    the arena's levels): the report's `ssim` / `ssim_cs`.
    Nothing is read back: the host waits when the report's numbers are (`OpenLoopReport.summary`)."""
    nv.check_current_device(store.device)
    t = int(sampler.denoiser.cfg.inner_model.num_steps_conditioning)
    horizon, ids = int(horizon), list(ids)
    if horizon < 1:
        raise ValueError(f"open_loop_eval: horizon {horizon}")
    for i, sid in enumerate(ids):
        _, start, stop = _id_fields(sid)
        if stop - start != t + horizon:
            raise ValueError(f"open_loop_eval: segment {i} has {stop - start} steps; {t} of context + {horizon} evaluated = {t + horizon}")
    if ssim and len(store.frame_shape or ()) != 3:
        raise ValueError(f"open_loop_eval: ssim needs (C, H, W) frames, the store holds {store.frame_shape}")
    ssim_p = ssim_params(len(ids), *store.frame_shape) if ssim else None  # (sizes the entry refuses: ValueError before any launch)
    seg_host, _, _ = store._descriptor(ids)
    dev, b = store.device, len(seg_host)
    seg = torch.from_numpy(seg_host).to(dev, non_blocking=True)

    # 1. the context: the first T steps of every segment, straight into the rings (slot t = step t: head 0)
    ctx_obs = torch.empty((b, t) + store.frame_shape, dtype=torch.float32, device=dev)
    ctx_act = torch.empty((b, t), dtype=torch.int64, device=dev)
    store.gather_static(seg, {"obs": ctx_obs, "act": ctx_act})
    # 2. the reward / end LSTM burnt in on the context's transitions (InitialConditionPool._load_round)
    hx_cx = None
    if t > 1:
        *_, hx_cx = rew_end_model.predict_rew_end(ctx_obs[:, :-1], ctx_act[:, :-1], ctx_obs[:, 1:])

    metrics = torch.empty((horizon, b, 4), dtype=torch.int64, device=dev)
    rew = torch.empty((horizon, b), dtype=torch.float32, device=dev)
    end = torch.empty((horizon, b), dtype=torch.uint8, device=dev)
    valid = torch.empty((horizon, b, 2), dtype=torch.uint8, device=dev)
    levels = torch.empty((horizon, b) + store.frame_shape, dtype=torch.uint8, device=dev) if return_levels else None
    if ssim:
        ssim_work = ssim_workspace(ssim_p, dev)
        ssim_out = torch.empty((horizon, b, 2), dtype=torch.float64, device=dev)  # row i: step i's (ssim, cs) pairs
    logits_rew, logits_end = [], []
    head = 0  # the rings' oldest slot: where the next frame goes
    for i in range(horizon):
        pred, _ = sampler.sample_ring(ctx_obs, ctx_act, head, head)
        newest = (head - 1) % t
        l_rew, l_end, hx_cx = rew_end_model.predict_rew_end(ctx_obs[:, newest:newest + 1], ctx_act[:, newest:newest + 1], pred, hx_cx)
        logits_rew.append(l_rew[:, 0])
        logits_end.append(l_end[:, 0])
        pred = pred.contiguous()
        _launch_step(store, seg, pred, ctx_obs, ctx_act, i, head, teacher_forced, metrics[i], rew[i], end[i], valid[i],
                     None if levels is None else levels[i])
        if ssim:
            _launch_ssim(ssim_p, store, seg, pred, t, i, ssim_work, ssim_out[i])
        head = (head + 1) % t

    m = metrics.permute(2, 1, 0)  # (4, B, horizon) views of the per-step rows
    v = valid.permute(2, 1, 0).bool()
    return OpenLoopReport(sq_err=m[0], abs_err=m[1], max_err=m[2], pixels_off=m[3], frame_valid=v[0], transition_valid=v[1],
                          logits_rew=torch.stack(logits_rew, dim=1), logits_end=torch.stack(logits_end, dim=1), rew_true=rew.t(),
                          end_true=end.t().to(store.flag_dtype), levels=None if levels is None else levels.transpose(0, 1),
                          ctx_obs=ctx_obs, ctx_act=ctx_act, head=head, per_frame=store.per_frame,
                          ssim=ssim_out[:, :, 0].t() if ssim else None, ssim_cs=ssim_out[:, :, 1].t() if ssim else None)
