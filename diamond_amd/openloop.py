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
With `motion=True` one dmd_openloop_motion launch per step more, before the ring advances: at 64 x 64 almost every value of a frame
equals the previous frame's, so a model that hands its newest context frame back scores well on all of the above.  The launch
counts what changed in the recording and in the prediction and what copying a frame would have scored: `summary()` then has the
skill over the two copies, recall / precision of the changed values, and the error split into changed and static values.

    totals = evaluate_store(sampler, agent.rew_end_model, store, horizon=15)           # every window of the store, batch by batch
    print(totals.summary())                                                            # the one wait
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Dict, Iterator, Optional, Sequence

import torch
from torch import Tensor

from . import native as nv
from .metrics import set_operand, ssim_params, ssim_workspace
from .replay import DeviceReplay, SegmentId, _id_fields


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
    # open_loop_eval(motion=True), else None -- (B, horizon) int64 in uint8 levels, with y the recorded frame, r the recorded frame
    # before it, a the context's last recorded frame, q the prediction's level and m the level of the frame the model saw last
    sq_copy_prev: Optional[Tensor] = None    # sum (y - r)^2: the error of copying the previous recorded frame; 0 where not prev_valid
    sq_copy_anchor: Optional[Tensor] = None  # sum (y - a)^2: the error of freezing the context; 0 where not anchor_valid
    changed_true: Optional[Tensor] = None    # values with y != r; 0 where not prev_valid
    changed_pred: Optional[Tensor] = None    # values with q != m, for every valid frame
    changed_both: Optional[Tensor] = None    # values with y != r and q != m; 0 where not prev_valid
    sq_err_changed: Optional[Tensor] = None  # sum of (q - y)^2 over the values with y != r; 0 where not prev_valid
    exact_changed: Optional[Tensor] = None   # values with y != r and q == y; 0 where not prev_valid
    prev_valid: Optional[Tensor] = None      # bool: the frame is valid and the episode recorded the step before it
    anchor_valid: Optional[Tensor] = None    # bool: the frame is valid and the context's last step is a recorded one

    def summary(self) -> Dict[str, Any]:
        """Plain Python numbers (this is where the host waits for the device), one entry per evaluated step over the samples
        whose frame / transition is valid there: `mse` in [-1, 1] units (formed in fp64 from the integer sums), `psnr` in dB
        (peak-to-peak 2; inf for an exact match), `pixels_off` as a share of the values, the worst `max_err` in levels, and the
        reward (3 x 3) / end (2 x 2) confusion matrices of the argmax predictions (rows: recorded class, sign(rew) + 1 / end).
        A step without valid samples has nan.  With the ssim fields: `ssim` and `ssim_cs`, the fp64 means over the valid frames.
        With the motion fields, each over the samples that are valid for it, 0 / 0 = nan:
          skill_prev / skill_anchor   1 - sum sq_err / sum sq_copy_prev (sq_copy_anchor): 0 for a model that copies that frame, 1 for
                                      the recording, negative for a model worse than the copy
          change_recall / _precision  sum changed_both / sum changed_true (sum changed_pred): of the values that changed, the share
                                      the prediction changed too / of the values the prediction changed, the share that did change
          share_changed               sum changed_true / values compared
          mse_changed / mse_static    `mse` over the values that changed / over the rest
          exact_changed               sum exact_changed / sum changed_true: changed values predicted to the level"""
        names = _SUM_INPUTS + tuple(k for k in ("ssim", "ssim_cs") + MOTION_FIELDS if getattr(self, k) is not None)
        sums = step_sums(SimpleNamespace(**{k: getattr(self, k).cpu() for k in names}))  # (summed on the host: one order on every device)
        return summarise(sums, self.per_frame)


MOTION_FIELDS = ("sq_copy_prev", "sq_copy_anchor", "changed_true", "changed_pred", "changed_both", "sq_err_changed", "exact_changed",
                 "prev_valid", "anchor_valid")
_SUM_INPUTS = ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true", "end_true")


def _confusion(logits: Tensor, target: Tensor, valid: Tensor, n: int) -> Tensor:
    """(horizon, n, n) int64: per step, entry [i, j] counts the valid samples of true class i predicted (argmax) as class j --
    rew_end_model.confusion_matrix per step, as comparisons and a sum (no data-dependent shape: no synchronisation)."""
    cell = target.long() * n + logits.argmax(dim=-1)  # (B, horizon)
    hit = (cell.unsqueeze(-1) == torch.arange(n * n, device=cell.device)) & valid.unsqueeze(-1)
    return hit.long().sum(0).reshape(-1, n, n)


def step_sums(rep) -> Dict[str, Tensor]:
    """The per-step sums over the samples of a report's (B, horizon) tensors that `summarise` forms its numbers from, on the
    tensors' device and without a synchronisation: int64 counts and sums masked by the validity flag of each entry, the worst
    max_err, the confusion matrices, and fp64 sums of the SSIM fields where present.  `rep`: an OpenLoopReport or a namespace
    with its fields."""
    fv, tv = rep.frame_valid, rep.transition_valid
    s = {"valid_frames": fv.long().sum(0), "valid_transitions": tv.long().sum(0)}
    for k in ("sq_err", "abs_err", "pixels_off"):
        s[k] = (getattr(rep, k) * fv).sum(0)
    s["max_err"] = (rep.max_err * fv).max(0).values
    s["confusion_matrix_rew"] = _confusion(rep.logits_rew, torch.sign(rep.rew_true).long() + 1, tv, 3)
    s["confusion_matrix_end"] = _confusion(rep.logits_end, rep.end_true, tv, 2)
    for k in ("ssim", "ssim_cs"):
        v = getattr(rep, k, None)
        if v is not None:
            v = v.double()
            s[k] = torch.where(fv, v, torch.zeros_like(v)).sum(0)
    if getattr(rep, "prev_valid", None) is not None:
        pv, av = rep.prev_valid, rep.anchor_valid
        s["prev_valid"], s["anchor_valid"] = pv.long().sum(0), av.long().sum(0)
        for k in ("sq_copy_prev", "changed_true", "changed_both", "sq_err_changed", "exact_changed"):
            s[k] = (getattr(rep, k) * pv).sum(0)
        s["sq_copy_anchor"] = (rep.sq_copy_anchor * av).sum(0)
        s["changed_pred"] = (rep.changed_pred * fv).sum(0)
        # the other side of each ratio over the same samples
        s["sq_err_prev"], s["sq_err_anchor"], s["changed_pred_prev"] = (rep.sq_err * pv).sum(0), (rep.sq_err * av).sum(0), (rep.changed_pred * pv).sum(0)
    return s


def summarise(sums: Dict[str, Tensor], per_frame: int) -> Dict[str, Any]:
    """`step_sums` (host tensors) -> the numbers of `OpenLoopReport.summary`.  The one place they are formed: equal sums give
    equal floats, whether they come from one report or from OpenLoopTotals."""
    unit = (2.0 / 255.0) ** 2  # one level squared, in [-1, 1] units
    vf = sums["valid_frames"]
    n = vf.double() * per_frame  # values compared per step
    mse = sums["sq_err"].double() / n * unit
    psnr = [float("nan") if math.isnan(m) else (float("inf") if m == 0 else 10.0 * math.log10(4.0 / m)) for m in mse.tolist()]
    out = {"horizon": int(vf.shape[0]), "valid_frames": vf.tolist(), "valid_transitions": sums["valid_transitions"].tolist(), "mse": mse.tolist(),
           "psnr": psnr, "pixels_off": (sums["pixels_off"].double() / n).tolist(), "max_err": sums["max_err"].tolist(),
           "confusion_matrix_rew": sums["confusion_matrix_rew"].tolist(), "confusion_matrix_end": sums["confusion_matrix_end"].tolist()}
    for k in ("ssim", "ssim_cs"):
        if k in sums:
            out[k] = (sums[k] / vf.double()).tolist()  # 0 / 0: nan
    if "prev_valid" in sums:
        d = {k: v.double() for k, v in sums.items() if k not in out}
        n_prev = d["prev_valid"] * per_frame
        out["valid_prev"], out["valid_anchor"] = sums["prev_valid"].tolist(), sums["anchor_valid"].tolist()
        out["skill_prev"] = (1.0 - d["sq_err_prev"] / d["sq_copy_prev"]).tolist()
        out["skill_anchor"] = (1.0 - d["sq_err_anchor"] / d["sq_copy_anchor"]).tolist()
        out["change_recall"] = (d["changed_both"] / d["changed_true"]).tolist()
        out["change_precision"] = (d["changed_both"] / d["changed_pred_prev"]).tolist()
        out["share_changed"] = (d["changed_true"] / n_prev).tolist()
        out["mse_changed"] = (d["sq_err_changed"] / d["changed_true"] * unit).tolist()
        out["mse_static"] = ((d["sq_err_prev"] - d["sq_err_changed"]) / (n_prev - d["changed_true"]) * unit).tolist()
        out["exact_changed"] = (d["exact_changed"] / d["changed_true"]).tolist()
    return out


class OpenLoopTotals:
    """The per-step sums of any number of reports (`step_sums`), kept on the device: `add` is torch integer ops on (B, horizon)
    tensors -- no synchronisation, no kernel of its own -- and `summary` is the one wait.  Reports must agree in horizon, frame
    size and in which optional fields (ssim, motion) they carry."""

    def __init__(self) -> None:
        self.sums: Optional[Dict[str, Tensor]] = None
        self.windows = 0
        self.per_frame: Optional[int] = None

    def add(self, report: OpenLoopReport) -> "OpenLoopTotals":
        s = step_sums(report)
        if self.sums is None:
            self.sums, self.per_frame = s, report.per_frame
        else:
            if set(s) != set(self.sums) or report.per_frame != self.per_frame or s["valid_frames"].shape != self.sums["valid_frames"].shape:
                raise ValueError("OpenLoopTotals.add: the report's horizon, frame size or optional fields differ from the totals'")
            self.sums = {k: torch.maximum(v, s[k]) if k == "max_err" else v + s[k] for k, v in self.sums.items()}
        self.windows += int(report.frame_valid.shape[0])
        return self

    def summary(self) -> Dict[str, Any]:
        """The keys of `OpenLoopReport.summary` over everything added, plus `windows` (this is where the host waits)."""
        if self.sums is None:
            raise ValueError("OpenLoopTotals.summary: nothing was added")
        out = summarise({k: v.cpu() for k, v in self.sums.items()}, self.per_frame)
        out["windows"] = self.windows
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


def _launch_motion(store: DeviceReplay, seg: Tensor, pred: Tensor, ctx_obs: Tensor, step: int, head: int, out: Tensor, valid: Tensor) -> None:
    """dmd_openloop_motion on the ring as it stands BEFORE step `step`'s advance -> out (B, 8), valid (B, 3)."""
    p = nv.MotionParams()
    p.B, p.T, p.per_frame, p.step, p.head = ctx_obs.shape[0], ctx_obs.shape[1], store.per_frame, step, head
    p.frames, p.end, p.finals, p.seg = (nv.ptr(x) for x in (store.frames, store.end, store.finals, seg))
    p.pred, p.ctx_obs, p.out, p.out_valid = nv.fptr(pred), nv.fptr(ctx_obs), nv.ptr(out), nv.ptr(valid)
    nv.check(nv.lib().dmd_openloop_motion(C.byref(p), nv.stream()), "dmd_openloop_motion")


@torch.no_grad()
def open_loop_eval(sampler, rew_end_model, store: DeviceReplay, ids: Sequence[Any], horizon: int, *, teacher_forced: bool = False,
                   return_levels: bool = False, ssim: bool = False, motion: bool = False) -> OpenLoopReport:
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
    motion: also what changed from frame to frame, in the recording and in the prediction, and what copying the previous recorded
    frame or the context's last frame would have scored (one dmd_openloop_motion launch per step, before the rings advance): the
    report's MOTION_FIELDS and the skill / change keys of `summary()`.
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
    if motion:
        moved = torch.empty((horizon, b, 8), dtype=torch.int64, device=dev)
        moved_valid = torch.empty((horizon, b, 3), dtype=torch.uint8, device=dev)
    logits_rew, logits_end = [], []
    head = 0  # the rings' oldest slot: where the next frame goes
    for i in range(horizon):
        pred, _ = sampler.sample_ring(ctx_obs, ctx_act, head, head)
        newest = (head - 1) % t
        l_rew, l_end, hx_cx = rew_end_model.predict_rew_end(ctx_obs[:, newest:newest + 1], ctx_act[:, newest:newest + 1], pred, hx_cx)
        logits_rew.append(l_rew[:, 0])
        logits_end.append(l_end[:, 0])
        pred = pred.contiguous()
        if motion:  # (on the ring before the advance: its newest slot is the frame the model saw last)
            _launch_motion(store, seg, pred, ctx_obs, i, head, moved[i], moved_valid[i])
        _launch_step(store, seg, pred, ctx_obs, ctx_act, i, head, teacher_forced, metrics[i], rew[i], end[i], valid[i],
                     None if levels is None else levels[i])
        if ssim:
            _launch_ssim(ssim_p, store, seg, pred, t, i, ssim_work, ssim_out[i])
        head = (head + 1) % t

    m = metrics.permute(2, 1, 0)  # (4, B, horizon) views of the per-step rows
    v = valid.permute(2, 1, 0).bool()
    extra = {}
    if motion:
        mm, mv = moved.permute(2, 1, 0), moved_valid.permute(2, 1, 0).bool()  # (8 | 3, B, horizon)
        extra = dict(sq_copy_prev=mm[0], sq_copy_anchor=mm[1], changed_true=mm[2], changed_pred=mm[3], changed_both=mm[4], sq_err_changed=mm[5],
                     exact_changed=mm[6], prev_valid=mv[1], anchor_valid=mv[2])
    return OpenLoopReport(sq_err=m[0], abs_err=m[1], max_err=m[2], pixels_off=m[3], frame_valid=v[0], transition_valid=v[1],
                          logits_rew=torch.stack(logits_rew, dim=1), logits_end=torch.stack(logits_end, dim=1), rew_true=rew.t(),
                          end_true=end.t().to(store.flag_dtype), levels=None if levels is None else levels.transpose(0, 1),
                          ctx_obs=ctx_obs, ctx_act=ctx_act, head=head, per_frame=store.per_frame,
                          ssim=ssim_out[:, :, 0].t() if ssim else None, ssim_cs=ssim_out[:, :, 1].t() if ssim else None, **extra)


def store_windows(store: DeviceReplay, horizon: int, stride: Optional[int] = None, *, t: int) -> Iterator[SegmentId]:
    """The windows of a whole-store pass, for `open_loop_eval` with a context of `t` steps: for every episode in id order and
    a = 0, stride, 2 * stride, ... while a + t < length (the context and at least one evaluated step are recorded),
    SegmentId(e, a, a + t + horizon).  stride defaults to `horizon`: every recorded step after an episode's first context is
    evaluated once.  A window may run past the episode's end; what was not recorded is flagged invalid there."""
    horizon, t = int(horizon), int(t)
    stride = horizon if stride is None else int(stride)
    if horizon < 1 or stride < 1 or t < 1:
        raise ValueError(f"store_windows: horizon {horizon}, stride {stride}, context {t}")
    for e in range(store.num_episodes):
        for a in range(0, max(int(store.lengths[e]) - t, 0), stride):
            yield SegmentId(e, a, a + t + horizon)


def evaluate_store(sampler, rew_end_model, store: DeviceReplay, horizon: int, *, batch_size: int = 32, stride: Optional[int] = None,
                   teacher_forced: bool = False, ssim: bool = False, motion: bool = True, max_windows: Optional[int] = None) -> OpenLoopTotals:
    """"How good is this world model on this store?": `open_loop_eval` over `store_windows(store, horizon, stride)` (the first
    `max_windows` of them), `batch_size` windows at a time -- the last batch may be short --, every report added to one
    OpenLoopTotals.  The host waits for the device only in the totals' `summary()`."""
    if int(batch_size) < 1:
        raise ValueError(f"evaluate_store: batch_size {batch_size}")
    t = int(sampler.denoiser.cfg.inner_model.num_steps_conditioning)
    ids = list(store_windows(store, horizon, stride, t=t))
    if max_windows is not None:
        ids = ids[:int(max_windows)]
    if not ids:
        raise ValueError(f"evaluate_store: no episode of the store has more than the {t} steps of a context")
    totals = OpenLoopTotals()
    for at in range(0, len(ids), int(batch_size)):
        totals.add(open_loop_eval(sampler, rew_end_model, store, ids[at:at + int(batch_size)], horizon, teacher_forced=teacher_forced, ssim=ssim,
                                  motion=motion))
    return totals
