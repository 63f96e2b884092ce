"""The host side of the graphed trainer step (diamond_amd/train_graph.py): `adopt_optimizer` turns the plain two-group AdamW that
the reference's `configure_opt` builds (utils.py:129-166: foreach, float LR, step counters on the host) into the form a captured step
can replay -- fused, capturable, step counters and LR in tensors -- without changing what it computes, and checkpoints travel both
ways.  Everything here runs on the CPU, where torch's fused Adam takes the same arguments.

The loop is the trainer's (trainer.py:363-382): backward per batch; every k-th batch clip, step, zero_grad, log
`get_last_lr()[0]`, `lr_sched.step()`."""
import copy

import pytest
import torch
from torch import nn
from torch.optim.lr_scheduler import LambdaLR

WARMUP, CLIP, ACC, UPDATES = 5, 0.5, 2, 8


def _model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(6, 16), nn.Tanh(), nn.Linear(16, 3))


LR = 1e-4  # the reference's (config/trainer.yaml), like the weight decay and eps below


def _plain_opt(m, lr=LR):
    """configure_opt's shape: weights decayed, biases not"""
    decay = [p for n, p in m.named_parameters() if n.endswith("weight")]
    rest = [p for n, p in m.named_parameters() if not n.endswith("weight")]
    return torch.optim.AdamW([{"params": decay, "weight_decay": 1e-2}, {"params": rest, "weight_decay": 0.0}], lr=lr, eps=1e-8)


def _sched(opt, warmup=WARMUP):
    return LambdaLR(opt, lambda s: 1 if s >= warmup else s / max(1, warmup))


def _batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(4, 6, generator=g), torch.randn(4, 3, generator=g)) for _ in range(n)]


def _train(m, opt, sched, batches, k=ACC):
    """the trainer's loop body; returns (losses, logged LRs)"""
    losses, lrs = [], []
    opt.zero_grad()
    for i, (x, y) in enumerate(batches):
        loss = (m(x) - y).square().mean()
        loss.backward()
        losses.append(float(loss.detach()))
        if (i + 1) % k == 0:
            torch.nn.utils.clip_grad_norm_(m.parameters(), CLIP)
            opt.step()
            opt.zero_grad()
            lrs.append(sched.get_last_lr()[0])
            sched.step()
    return losses, lrs


def _steps(opt):
    return [float(opt.state[p]["step"]) for g in opt.param_groups for p in g["params"]]


def test_adopted_optimizer_trains_like_the_plain_one():
    """two groups, LambdaLR warm-up over 5 steps, clip 0.5, accumulation 2, 8 updates: the same logged LRs (==), the same losses,
    parameters within 1e-6 relative (the fused CPU kernel rounds differently: ~1.5e-8 absolute on O(0.3) weights)"""
    from diamond_amd.train_graph import _lr_to_device_tensors, _scheduled_lr, adopt_optimizer

    batches = _batches(ACC * UPDATES)
    m0 = _model()
    o0 = _plain_opt(m0)
    losses0, lrs0 = _train(m0, o0, _sched(o0), batches)

    m1 = _model()
    o1 = _plain_opt(m1)
    s1 = _sched(o1)  # the trainer builds the scheduler on the plain optimizer: lr is the float 0.0 now
    assert o1.param_groups[0]["lr"] == 0.0
    assert adopt_optimizer(o1, "cpu") is o1
    _lr_to_device_tensors(o1, "cpu")
    for g in o1.param_groups:
        assert g["capturable"] is True and g["fused"] is True and g["foreach"] is False
        assert torch.is_tensor(g["lr"]) and g["lr"].dtype == torch.float32 and g["lr"].dim() == 0
    assert [g["weight_decay"] for g in o1.param_groups] == [1e-2, 0.0]
    closed = []
    real_step = s1.step

    def spy():  # the closed form GraphedTrainStep logs, evaluated where it evaluates it: right before the scheduler steps
        closed.append(_scheduled_lr(s1))
        real_step()

    s1.step = spy
    losses1, lrs1 = _train(m1, o1, s1, batches)
    assert len(lrs0) == UPDATES and lrs0[0] == 0.0 and lrs0[-1] == LR
    assert [float(x) for x in lrs1] == [float(torch.tensor(x, dtype=torch.float32)) for x in lrs0], "the tensor LR follows the schedule"
    assert closed == lrs0 and all(isinstance(x, float) for x in closed), (closed, lrs0)
    assert losses1 == losses0, (losses0, losses1)
    for (n, a), b in zip(m0.named_parameters(), m1.parameters()):
        assert float((a - b).detach().abs().max()) <= 1e-6 * float(a.detach().abs().max()), n
    assert _steps(o1) == [float(UPDATES)] * 4
    assert all(o1.state[p]["step"].dtype == torch.float32 and o1.state[p]["step"].dim() == 0 for p in m1.parameters())


def test_adopt_rejects_other_optimizers_by_name():
    from diamond_amd.train_graph import adopt_optimizer

    m = _model()
    with pytest.raises(TypeError, match="SGD"):
        adopt_optimizer(torch.optim.SGD(m.parameters(), lr=0.1), "cpu")


def test_adopt_keeps_loaded_moments_and_makes_the_step_counters_tensors():
    from diamond_amd.train_graph import adopt_optimizer

    batches = _batches(ACC * 3)
    m = _model()
    o = _plain_opt(m)
    _train(m, o, _sched(o), batches)
    before = {p: (o.state[p]["exp_avg"].clone(), o.state[p]["exp_avg_sq"].clone(), o.state[p]["exp_avg"].data_ptr()) for p in m.parameters()}
    adopt_optimizer(o, "cpu")
    for p in m.parameters():
        st = o.state[p]
        assert torch.equal(st["exp_avg"], before[p][0]) and torch.equal(st["exp_avg_sq"], before[p][1])
        assert st["exp_avg"].data_ptr() == before[p][2], "the moments are kept, not copied"
        assert torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32 and float(st["step"]) == 3.0


def test_checkpoints_travel_both_ways():
    """adopted -> plain: the adopted optimizer's state_dict loads into a freshly built plain optimizer, which then steps;
    plain -> adopted: a plain checkpoint loads into a fresh optimizer that is adopted afterwards.  Either way the step counters
    equal the number of updates, and the continued run is the uninterrupted one (same bar as above)."""
    from diamond_amd.train_graph import _lr_to_device_tensors, adopt_optimizer

    first, second = 3, 2
    batches = _batches(ACC * (first + second))
    ref_m = _model()
    ref_o = _plain_opt(ref_m)
    _train(ref_m, ref_o, _sched(ref_o), batches)

    for direction in ("adopted -> plain", "plain -> adopted"):
        m = _model()
        o = _plain_opt(m)
        s = _sched(o)
        if direction == "adopted -> plain":
            adopt_optimizer(o, "cpu")
            _lr_to_device_tensors(o, "cpu")
        _train(m, o, s, batches[:ACC * first])
        assert _steps(o) == [float(first)] * 4, direction
        ckpt = copy.deepcopy({"model": m.state_dict(), "opt": o.state_dict(), "sched": s.state_dict()})

        m2 = _model(seed=9)
        o2 = _plain_opt(m2)
        s2 = _sched(o2)
        m2.load_state_dict(ckpt["model"])
        o2.load_state_dict(ckpt["opt"])
        s2.load_state_dict(ckpt["sched"])
        if direction == "plain -> adopted":
            adopt_optimizer(o2, "cpu")
            _lr_to_device_tensors(o2, "cpu")
            assert all(g["fused"] is True and g["capturable"] is True for g in o2.param_groups)
        assert _steps(o2) == [float(first)] * 4, direction
        assert [g["weight_decay"] for g in o2.param_groups] == [1e-2, 0.0]
        _, lrs = _train(m2, o2, s2, batches[ACC * first:])
        assert _steps(o2) == [float(first + second)] * 4, direction
        assert [round(float(x) / LR, 6) for x in lrs] == [0.6, 0.8], (direction, lrs)
        for (n, a), b in zip(ref_m.named_parameters(), m2.parameters()):
            assert float((a - b).detach().abs().max()) <= 1e-6 * float(a.detach().abs().max()), (direction, n)


def test_new_arguments_are_keyword_only_and_default_to_todays_behaviour():
    import inspect

    from diamond_amd.train_graph import GraphedTrainStep, graphed_rew_end_step

    sig = inspect.signature(GraphedTrainStep.__init__).parameters
    want = {"lr_scheduler": None, "step_scheduler": True, "grad_acc_steps": 1, "preserve_state": False, "adopt_optimizer": False}
    for name, default in want.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert list(sig)[:9] == ["self", "model", "optimizer", "max_grad_norm", "example_batch", "warmup_steps", "fields", "step_fn", "stage"]
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(graphed_rew_end_step).parameters.values())
