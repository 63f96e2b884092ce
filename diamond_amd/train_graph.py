"""The world-model training step as ONE hipGraph (reference trainer.py:349-388: `loss, metrics = model(batch);
loss.backward(); clip_grad_norm_; opt.step(); opt.zero_grad()`).

At the reference's batch of 32 the step is launch-bound: ~600 kernel launches of 5-30 us each, issued by a Python
interpreter that needs longer per launch than the GPU needs per kernel.  Every dmd_* entry point is asynchronous on
torch's current stream, allocates nothing and synchronises nothing (include/diamond_hip.h), and the step itself is free
of host synchronisations (Denoiser.forward masks the loss arithmetically instead of gathering), so forward, backward,
clipping and the optimizer update record into one graph that is replayed per step on static input buffers:

    step = GraphedTrainStep(agent.denoiser, opt, max_grad_norm, example_batch)     # opt: capturable=True (+ fused=True)
    for batch in loader:
        loss, metrics = step(batch)          # == model(batch) ... opt.step(); opt.zero_grad() of the eager loop

Nothing of an earlier eager step's autograd graph may still be referenced when the step is constructed (e.g. a kept `loss`
tensor): its AccumulateGrad nodes belong to the stream they were created on, and autograd would synchronise the capturing
stream with it (torch warns "AccumulateGrad node's stream does not match"; the capture then aborts).

The optimizer: `torch.optim.AdamW(..., capturable=True, fused=True)`.  The capturable FOREACH form divides every tensor by its
0-dim bias corrections with one broadcast kernel each -- 2 x 236 launches of ~4 us, 1.5 ms of an 11.9 ms step
(profiles/r04_train_kernel_stats_foreach_adamw.csv); torch's fused form is one multi-tensor kernel: 10.35 ms.  It does not
bump `Tensor._version`; engine's optimizer post-step hook marks the weight caches stale instead.

What is captured is exactly the eager step's launch sequence.  Weight packing (engine.PackCache, blocks.FilmTable) is keyed
on parameter versions / that hook: the warm-up steps' optimizer updates make every copy stale, so every pack / transpose kernel is recorded
too: the step ends with an explicit refresh of every cache behind the optimizer update (one dmd_pack_jobs launch per cache,
in place), so after a replay the packed copies equal the parameters -- also for readers that never look a copy up again (the
sampler's captured imagination graphs read the packed buffers directly).

The reward / end model (the trainer's second world-model component) records the same way through `graphed_rew_end_step`: its
`forward` asks the host which episodes ended and gathers by a boolean mask, so the captured step is `forward_static`, and the
one thing that needs the host -- which samples carry a `final_observation` -- runs on every incoming batch before it is copied
into the static buffers (`stage`).

The rest of the trainer's loop body (trainer.py:365-382), keyword-only and off by default -- host orchestration around the same
launches, no kernel and no ABI change:

    step = GraphedTrainStep(model, opt, cfg.max_grad_norm, first_batch, lr_scheduler=lr_sched, grad_acc_steps=cfg.grad_acc_steps,
                            adopt_optimizer=True, preserve_state=True)              # the trainer's own `opt` and `lr_sched`
    for i in range(cfg.grad_acc_steps * steps):
        loss, metrics = step(batch)          # == trainer.py:365-382: "grad_norm_before_clip" and "lr" on every k-th call

  lr_scheduler    A captured `optimizer.step()` reads a host-float `lr` ONCE, at capture: it becomes a launch constant, and the
                  reference's `LambdaLR` warm-up (utils.py:177-181; `lr` is 0.0 right after its construction) would replay that
                  value for ever.  WITHOUT `lr_scheduler=` a captured step keeps the LR of capture time.  With it every group's
                  `lr` is made a 0-dim fp32 device tensor before warm-up and capture (torch's AdamW then reads it from memory,
                  torch's schedulers `fill_` it in place), and every update call sets `metrics["lr"]` to the LR that update
                  used -- for a `LambdaLR` the host float `base_lr * lambda(last_epoch)`, the very expression `get_last_lr()`
                  stores, computed without reading the device -- and then calls `lr_scheduler.step()` (trainer.py:380-382);
                  `step_scheduler=False` leaves that call to the caller.  The `fill_` goes to the stream of the replay.
  grad_acc_steps  k > 1: two graphs from one memory pool.  Calls that are not a multiple of k replay forward + backward, which
                  accumulates into the static gradient buffers, and return (loss, metrics) of that micro-step; every k-th call
                  replays forward + backward + clip + update + refresh of the packed weights + an in-place zeroing of the
                  gradients.  The loss is not divided by k (the reference does not).
  grad_norm_before_clip   what `clip_grad_norm_` returns (a graph buffer like the loss), on update calls with a `max_grad_norm`.
  preserve_state  Construction runs `warmup_steps` REAL updates on the example batch (kernel attributes, optimizer state, job
                  tables).  With preserve_state=True it leaves no trace: parameters, buffers, optimizer state (zero moments and
                  step 0 where there was none), the LR, the scheduler's state and both default generators are put back IN
                  PLACE -- the graph holds these pointers -- and the packed weights are rebuilt from the restored parameters.
  adopt_optimizer A plain `torch.optim.AdamW` / `Adam` as `utils.configure_opt` builds it (foreach, float step counters on the
                  host, several groups) is converted in place by `adopt_optimizer(optimizer, device)` below instead of being
                  rejected; call it AFTER `optimizer.load_state_dict` on a resume (loading replaces the groups' options).
"""
from __future__ import annotations

import copy
from typing import Any, Callable, Dict, Optional, Tuple

import torch
from torch import Tensor, nn


def _weight_caches(model: nn.Module):
    from . import engine as E

    for m in model.modules():
        if isinstance(getattr(m, "_cache", None), E.PackCache):
            yield m._cache
        film = getattr(m, "_film", None)
        if film is not None and hasattr(film, "refresh"):
            yield film


def _mark_weight_caches_stale(model: nn.Module) -> None:
    """Every packed copy of the model's parameters is stale (buffers and job tables are kept: engine.PackCache.invalidate)."""
    for c in _weight_caches(model):
        c.invalidate()


def _refresh_weight_caches(model: nn.Module) -> None:
    """Rebuild, in place and on the current stream, every packed copy that is stale (capturable: no allocation of a table,
    no upload -- the job tables exist after the warm-up)."""
    for c in _weight_caches(model):
        c.refresh()


def adopt_optimizer(optimizer: torch.optim.Optimizer, device) -> torch.optim.Optimizer:
    """Make a plain `torch.optim.AdamW` / `Adam` replayable, in place: every group capturable=True, fused=True, foreach=False (one
    multi-tensor kernel that reads step counters and a tensor `lr` from device memory), existing `step` entries fp32 tensors on
    the parameters' device; `exp_avg` / `exp_avg_sq`, the groups and their `weight_decay` are kept.  Works on an empty state and
    behind `load_state_dict`.  Host code only (on the CPU torch's fused Adam runs the same way)."""
    if not isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)):
        raise TypeError(f"adopt_optimizer: torch.optim.AdamW or Adam expected, got {type(optimizer).__module__}.{type(optimizer).__qualname__}")
    kind = torch.device(device).type
    for group in optimizer.param_groups:
        if group.get("differentiable", False):
            raise ValueError("adopt_optimizer: a differentiable optimizer has no fused form")
        for p in group["params"]:
            if p.device.type != kind or not p.is_floating_point():
                raise ValueError(f"adopt_optimizer: a {p.dtype} parameter on {p.device}, floating-point parameters on {kind} expected")
            state = optimizer.state.get(p)
            if state and "step" in state:
                step = state["step"]
                if not (torch.is_tensor(step) and step.dtype == torch.float32 and step.device == p.device):
                    state["step"] = torch.tensor(float(step), dtype=torch.float32, device=p.device)
        group.update(capturable=True, fused=True, foreach=False)
    return optimizer


_adopt_optimizer = adopt_optimizer  # (GraphedTrainStep's keyword of the same name shadows the function)


def _lr_to_device_tensors(optimizer: torch.optim.Optimizer, device) -> None:
    """Every group's `lr` a 0-dim fp32 tensor on `device` (kept if it is one): what a captured optimizer kernel reads at replay and
    torch's schedulers update with `fill_`."""
    for group in optimizer.param_groups:
        lr = group["lr"]
        if not (torch.is_tensor(lr) and lr.dtype == torch.float32 and lr.device == torch.device(device) and lr.dim() == 0):
            group["lr"] = torch.tensor(float(lr), dtype=torch.float32, device=device)


def _scheduled_lr(scheduler) -> Any:
    """The LR of the update that just ran, as trainer.py:381 logs it (`lr_sched.get_last_lr()[0]`), without a device read: for a
    LambdaLR the closed form `get_lr` evaluates -- the same host expression, so the same float; for any other scheduler what
    `get_last_lr()` holds (a device tensor once the LR is one; it is not read here)."""
    if isinstance(scheduler, torch.optim.lr_scheduler.LambdaLR):
        return scheduler.base_lrs[0] * scheduler.lr_lambdas[0](scheduler.last_epoch)
    return scheduler.get_last_lr()[0]


class _Snapshot:
    """preserve_state: what construction may change, and how to put it back in place."""

    def __init__(self, model: nn.Module, optimizer: torch.optim.Optimizer, scheduler, device) -> None:
        self.cpu_rng, self.dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state(device)
        self.tensors = [(t, t.detach().clone()) for t in list(model.parameters()) + list(model.buffers())]
        self.state = {p: {k: (v.detach().clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in st.items()}
                      for p, st in optimizer.state.items()}
        self.lrs = [float(g["lr"]) for g in optimizer.param_groups]
        self.scheduler = None if scheduler is None else copy.deepcopy(scheduler.state_dict())

    @torch.no_grad()
    def restore(self, model: nn.Module, optimizer: torch.optim.Optimizer, scheduler, device) -> None:
        for t, saved in self.tensors:
            t.copy_(saved)
        for p, st in optimizer.state.items():
            before = self.state.get(p)
            for k, v in st.items():
                if not torch.is_tensor(v):
                    if before is not None and k in before:
                        st[k] = copy.deepcopy(before[k])
                elif before is not None and k in before:
                    v.copy_(before[k])
                else:
                    v.zero_()  # no state before: zero moments, step 0 (the entries stay: the graph holds their pointers)
        for group, lr in zip(optimizer.param_groups, self.lrs):
            if torch.is_tensor(group["lr"]):
                group["lr"].fill_(lr)
            else:
                group["lr"] = lr
        if scheduler is not None:
            scheduler.load_state_dict(copy.deepcopy(self.scheduler))
        # the packed copies hold the warm-up's weights; the first replay reads them before its own refresh
        _mark_weight_caches_stale(model)
        _refresh_weight_caches(model)
        torch.set_rng_state(self.cpu_rng)
        torch.cuda.set_rng_state(self.dev_rng, device)


class GraphedTrainStep:
    def __init__(self, model: nn.Module, optimizer: torch.optim.Optimizer, max_grad_norm: Optional[float], example_batch: Any,
                 warmup_steps: int = 3, fields: Tuple[str, ...] = ("obs", "act", "mask_padding"),
                 step_fn: Optional[Callable[[Any], Tuple[Tensor, Dict[str, Any]]]] = None,
                 stage: Optional[Callable[[Any], None]] = None, *, lr_scheduler: Any = None, step_scheduler: bool = True,
                 grad_acc_steps: int = 1, preserve_state: bool = False, adopt_optimizer: bool = False) -> None:
        """step_fn: (static_batch) -> (loss, metrics), what the captured step calls instead of `model` (it must be free of host
        synchronisations and data-dependent shapes).  stage: (batch) -> None, run on the example batch and on every incoming
        batch BEFORE it is copied into the static buffers -- eager, outside the graph: the place for what needs the host.
        lr_scheduler / step_scheduler / grad_acc_steps / preserve_state / adopt_optimizer: the module docstring."""
        assert torch.cuda.is_available(), "GraphedTrainStep needs the GPU"
        assert int(grad_acc_steps) >= 1, f"grad_acc_steps = {grad_acc_steps}"
        device = next(model.parameters()).device
        if adopt_optimizer:
            _adopt_optimizer(optimizer, device)
        for group in optimizer.param_groups:
            assert group.get("capturable", False), \
                "construct the optimizer with capturable=True (its step counter must live on the device to be replayed)"
        if lr_scheduler is not None:
            assert lr_scheduler.optimizer is optimizer, "lr_scheduler drives another optimizer"
            _lr_to_device_tensors(optimizer, device)  # before warm-up and capture: the captured update reads the LR from memory
        self.model, self.optimizer, self.max_grad_norm, self.fields = model, optimizer, max_grad_norm, fields
        self.step_fn, self.stage = (model if step_fn is None else step_fn), stage
        self.lr_scheduler, self.step_scheduler, self.grad_acc_steps = lr_scheduler, bool(step_scheduler), int(grad_acc_steps)
        self._calls = 0  # the trainer's `i`
        snapshot = _Snapshot(model, optimizer, lr_scheduler, device) if preserve_state else None
        if stage is not None:
            stage(example_batch)
        self.static = {k: getattr(example_batch, k).detach().clone() for k in fields}
        self._batch = type("StaticBatch", (), {})()
        for k, v in self.static.items():
            setattr(self._batch, k, v)
        accumulate = self.grad_acc_steps > 1
        if accumulate:
            optimizer.zero_grad(set_to_none=True)  # the warm-up's first backward allocates the buffers every later one adds to
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # eager warm-up: kernel attributes, optimizer state, parameter versions bumped
            for _ in range(max(1, warmup_steps)):
                if accumulate:
                    for _ in range(self.grad_acc_steps - 1):
                        self._micro()
                self._eager(zero_in_place=accumulate)
                if lr_scheduler is not None and self.step_scheduler:
                    lr_scheduler.step()  # a warm-up step is a real step of the trainer's loop
        cur.wait_stream(side)
        torch.cuda.synchronize()
        # The packed copies are rebuilt at the END of the captured step, behind the optimizer update (not at its start): a
        # replay then leaves them equal to the parameters it leaves, and anything that reads them without a lookup -- the
        # sampler's captured imagination graphs -- is never a step behind.  So they have to be fresh going in:
        _mark_weight_caches_stale(model)
        _refresh_weight_caches(model)
        self.graph = torch.cuda.CUDAGraph()
        if not accumulate:
            optimizer.zero_grad(set_to_none=True)  # the gradients of the captured step come from the graph's own pool
            # thread_local: other threads' HIP calls (the RCCL watchdog polls its events) must not invalidate this capture
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.loss, self.metrics = self._eager(zero=False)
            # (gradients stay allocated: the captured backward writes, not accumulates, into them at every replay)
        else:
            # The gradients are the warm-up's buffers, zero now and never re-allocated: both graphs ADD to them (0 + g is g, bit
            # for bit), the update graph zeroes them in place at its end.  One pool: the graphs never run concurrently, and they
            # are replayed in the order of capture (micro-steps, then the update).
            self._grads = [p.grad for p in model.parameters() if p.grad is not None]
            self.graph_acc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_acc, capture_error_mode="thread_local"):
                self._acc_loss, self._acc_metrics = self._micro()
            with torch.cuda.graph(self.graph, pool=self.graph_acc.pool(), capture_error_mode="thread_local"):
                self.loss, self.metrics = self._eager(zero_in_place=True)
        if snapshot is not None:
            snapshot.restore(model, optimizer, lr_scheduler, device)

    def _micro(self):
        """forward + backward: trainer.py:365-366"""
        loss, metrics = self.step_fn(self._batch)
        loss.backward()
        return loss.detach(), {k: (v.detach() if isinstance(v, Tensor) else v) for k, v in metrics.items()}

    def _eager(self, zero: bool = True, zero_in_place: bool = False):
        """forward + backward + trainer.py:372-378"""
        loss, metrics = self._micro()
        if self.max_grad_norm is not None:
            metrics["grad_norm_before_clip"] = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm).detach()
        self.optimizer.step()
        _refresh_weight_caches(self.model)  # one dmd_pack_jobs launch per cache, on the updated weights
        if zero_in_place:
            self.optimizer.zero_grad(set_to_none=False)  # (multi-tensor zeroing; the buffers and their pointers stay)
        elif zero:
            self.optimizer.zero_grad(set_to_none=True)
        return loss, metrics

    def __call__(self, batch: Any) -> Tuple[Tensor, Dict[str, Any]]:
        if self.stage is not None:
            self.stage(batch)
        for k, buf in self.static.items():
            src = getattr(batch, k)
            assert src.shape == buf.shape and src.dtype == buf.dtype, \
                f"batch.{k}: {tuple(src.shape)} {src.dtype}, captured with {tuple(buf.shape)} {buf.dtype} (static shapes)"
            buf.copy_(src, non_blocking=True)
        self._calls += 1
        if self._calls % self.grad_acc_steps != 0:  # trainer.py:372: a micro-step, the gradients accumulate
            self.graph_acc.replay()
            return self._acc_loss, dict(self._acc_metrics)
        self.graph.replay()
        self._replays = getattr(self, "_replays", 0) + 1
        if self._replays % 64 == 0:  # the always-on audit of the packed copies (engine.WeightAudit): no lookup runs inside a replay
            for c in _weight_caches(self.model):
                for a in c.audits():
                    a.run()
        # The replayed optimizer update changed every parameter without bumping its `_version`; the packed copies were
        # rebuilt from the new values by the replay itself, in place: the stamps of capture time still describe them, and
        # graphs captured elsewhere from the same weights (DiffusionSampler.sample_ring_graphed) read the new values through
        # the same pointers.
        if self.lr_scheduler is None and self.grad_acc_steps == 1:
            return self.loss, self.metrics
        metrics = dict(self.metrics)  # the caller's own dict (the trainer adds keys to it and keeps it)
        if self.lr_scheduler is not None:
            metrics["lr"] = _scheduled_lr(self.lr_scheduler)  # trainer.py:381, a host value: nothing is read from the device
            if self.step_scheduler:
                self.lr_scheduler.step()  # trainer.py:382: `fill_` of the device LR on this stream, behind the replay
        return self.loss, metrics


def graphed_rew_end_step(model: nn.Module, optimizer: torch.optim.Optimizer, max_grad_norm: Optional[float], example_batch: Any,
                         warmup_steps: int = 3, **trainer_kwargs: Any) -> GraphedTrainStep:
    """The reward / end model's training step (reference trainer.py:349-388 on `agent.rew_end_model`) as one replayed hipGraph:

        step = graphed_rew_end_step(agent.rew_end_model, opt, max_grad_norm, example_batch)    # opt: capturable=True
        for batch in loader:
            loss, metrics = step(batch)

    Per batch, eagerly: RewEndModel.put_back_final_observations (writes through to `batch.obs`, like `forward`), then the copy of
    obs / act / rew / end / mask_padding into the static buffers; replayed: RewEndModel.forward_static, backward, clipping, the
    optimizer update and the refresh of the packed weights.  The returned loss and metrics -- the nested confusion matrices
    included, returned as they are -- are the graph's own buffers: the next replay overwrites them, so clone what has to outlive
    the step (as for the denoiser).  trainer_kwargs: GraphedTrainStep's keyword-only arguments (lr_scheduler, step_scheduler,
    grad_acc_steps, preserve_state, adopt_optimizer), forwarded unchanged."""
    return GraphedTrainStep(model, optimizer, max_grad_norm, example_batch, warmup_steps=warmup_steps,
                            fields=("obs", "act", "rew", "end", "mask_padding"), stage=model.put_back_final_observations,
                            step_fn=model.forward_static, **trainer_kwargs)
