"""The graphed world-model step as the whole body of the trainer's loop (diamond_amd/train_graph.py; reference trainer.py:363-382):
the LR warm-up schedule survives replay (`lr_scheduler=`), gradients accumulate over k calls (`grad_acc_steps=`), the trainer's
`grad_norm_before_clip` and `lr` metrics come back, construction can leave no trace (`preserve_state=`), and the plain optimizer that
`configure_opt` builds is taken over and resumed from a checkpoint (`adopt_optimizer=`).

The eager arm is the literal trainer body: zero_grad; per batch forward, backward; every k-th batch clip_grad_norm_, step, zero_grad,
log `get_last_lr()[0]`, `lr_sched.step()`.  Fixtures: the default denoiser at 64 x 64, batch 2, a segment of 6 frames, the device-
resident noise table of tests/test_gpu_train_graph.py; the reward / end model on the batch-2 fixture of tests/test_rew_end_graph.py.
Bars: losses 1e-6 and parameters 1e-5 relative (test_graphed_training_step_matches_the_eager_loop's), gradient norms 1e-5."""
import copy
import io
from types import SimpleNamespace

import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

from tests.test_gpu_models import make_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
BASE_LR, WARMUP, CLIP = 3e-4, 3, 1.0


def _denoiser(seed=5, b=2, t=6):
    """(denoiser in training mode with the fixed noise table, three batches): tests/test_gpu_train_graph.py::_setup at batch 2"""
    import diamond_amd as D
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    den = make_agent().denoiser
    den.train()
    den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
    g = torch.Generator().manual_seed(seed)
    batches = []
    for k in range(3):
        mask = torch.ones(b, t, dtype=torch.bool)
        mask[k % b, 5] = False
        batches.append(SimpleNamespace(obs=synthetic_frames(g, b, t, 3, 64, 64).to(DEV), act=synthetic_actions(g, 4, b, t).to(DEV),
                                       mask_padding=mask.to(DEV)))
    table = {}

    def randn_fn(shape):
        if shape not in table:
            table[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(len(table) + 99)).to(DEV)
        return table[shape]

    den.randn_fn = randn_fn
    return den, batches


def _fused(model, lr=BASE_LR):
    return torch.optim.AdamW(model.parameters(), lr=lr, capturable=True, fused=True)


def _plain_two_groups(model, lr=BASE_LR):
    """what configure_opt returns (utils.py:129-166): a plain foreach AdamW, matrices and kernels decayed, the rest not"""
    decay = [p for p in model.parameters() if p.dim() >= 2]
    rest = [p for p in model.parameters() if p.dim() < 2]
    return torch.optim.AdamW([{"params": decay, "weight_decay": 1e-2}, {"params": rest, "weight_decay": 0.0}], lr=lr, eps=1e-8)


def _warmup(opt, n=WARMUP):
    return LambdaLR(opt, lambda s: 1 if s >= n else s / max(1, n))  # utils.get_lr_sched


def _params(model):
    return {k: v.detach().clone() for k, v in model.named_parameters()}


def _trainer_loop(model, fwd, opt, sched, batches, calls, k, clip=CLIP, after_update=None):
    """trainer.py:357-382; returns (losses per call, [(grad_norm_before_clip, lr)] per update)"""
    losses, updates = [], []
    opt.zero_grad()
    for i in range(calls):
        loss, _ = fwd(batches[i % len(batches)])
        loss.backward()
        losses.append(float(loss.detach()))
        del loss  # (no reference to the autograd graph survives into a later capture: train_graph.py)
        if (i + 1) % k == 0:
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            opt.step()
            opt.zero_grad()
            updates.append((float(norm), sched.get_last_lr()[0]))
            sched.step()
            if after_update is not None:
                after_update(len(updates))
    return losses, updates


def _graph_loop(step, batches, calls, k, after_update=None, first=0):
    losses, updates = [], []
    for i in range(first, first + calls):
        loss, metrics = step(batches[i % len(batches)])
        losses.append(float(loss))
        if (i + 1) % k == 0:
            assert torch.is_tensor(metrics["grad_norm_before_clip"]) and metrics["grad_norm_before_clip"].dim() == 0
            assert metrics["grad_norm_before_clip"].is_cuda
            updates.append((float(metrics["grad_norm_before_clip"]), metrics["lr"]))
            if after_update is not None:
                after_update(len(updates))
        else:
            assert "lr" not in metrics and "grad_norm_before_clip" not in metrics, sorted(metrics)
    return losses, updates


def _compare(eager, graph, params_e, model, init):
    (losses_e, upd_e), (losses_g, upd_g) = eager, graph
    print("eager", losses_e, upd_e, "\ngraph", losses_g, upd_g)
    assert [lr for _, lr in upd_g] == [lr for _, lr in upd_e], "metrics['lr'] is the LR the trainer logs, value for value"
    assert all(isinstance(lr, float) for _, lr in upd_g)
    assert len(losses_g) == len(losses_e)
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-6 * abs(a), (losses_e, losses_g)
    for (a, _), (b, _) in zip(upd_e, upd_g):
        assert abs(a - b) <= 1e-5 * abs(a), (upd_e, upd_g)
    worst = max(float((p.detach() - params_e[k]).abs().max() / params_e[k].abs().max().clamp_min(1e-12)) for k, p in model.named_parameters())
    moved = max(float((p.detach() - init[k]).abs().max()) for k, p in model.named_parameters())
    assert moved > 1e-4, "parameters did not train"
    assert worst < 1e-5, f"parameters differ from the eager loop by {worst:.3e}"


class _Schedule:
    """after update 1 (LR 0) every parameter is bitwise its initial value while the first moments are not zero; after update 2 the
    parameters have moved: what catches an LR frozen into the graph, whichever value was frozen"""

    def __init__(self, model, opt, init):
        self.model, self.opt, self.init, self.seen = model, opt, init, set()

    def __call__(self, n):
        self.seen.add(n)
        if n == 1:
            same = [k for k, p in self.model.named_parameters() if not torch.equal(p.detach(), self.init[k])]
            assert not same, f"LR 0, and yet {len(same)} parameters changed, e.g. {same[:3]}"
            states = [self.opt.state[p] for p in self.model.parameters() if p in self.opt.state]
            assert states and sum(float(st["exp_avg"].abs().sum()) for st in states) > 0, "the update ran: the moments moved"
            assert all(float(st["step"]) == 1.0 for st in states)
        if n == 2:
            moved = max(float((p.detach() - self.init[k]).abs().max()) for k, p in self.model.named_parameters())
            assert moved > 1e-5, f"LR {BASE_LR / WARMUP:g} (an Adam update of that size per element), and the parameters moved by {moved:.3e}"


def _schedule_case(make, fwd_of, build, calls, k, parameters_against_a_tensor_lr=False):
    """both arms from the same state_dict; asserts everything of the schedule tests.  parameters_against_a_tensor_lr: the final
    parameters are compared with a second run of the eager loop whose optimizer reads the LR from the same fp32 device tensor
    (test_warmup_schedule_survives_replay_rew_end_model says why); everything else is compared with the float-LR loop."""
    from diamond_amd.train_graph import _lr_to_device_tensors

    m, batches = make()
    init = copy.deepcopy(m.state_dict())
    opt = _fused(m)
    eager = _trainer_loop(m, fwd_of(m), opt, _warmup(opt), batches, calls, k)
    params_e = _params(m)
    if parameters_against_a_tensor_lr:
        m, batches = make()
        m.load_state_dict(init)
        opt = _fused(m)
        sched = _warmup(opt)
        _lr_to_device_tensors(opt, DEV)
        _trainer_loop(m, fwd_of(m), opt, sched, batches, calls, k)
        params_e = _params(m)

    m2, batches2 = make()
    m2.load_state_dict(init)
    init_p = _params(m2)
    opt2 = _fused(m2)
    sched2 = _warmup(opt2)
    step = build(m2, opt2, batches2[0], lr_scheduler=sched2, grad_acc_steps=k, preserve_state=True)
    for g in opt2.param_groups:
        assert torch.is_tensor(g["lr"]) and g["lr"].is_cuda and g["lr"].dtype == torch.float32 and g["lr"].dim() == 0
    watch = _Schedule(m2, opt2, init_p)
    graph = _graph_loop(step, batches2, calls, k, after_update=watch)
    assert watch.seen >= {1, 2}
    assert sched2.last_epoch == calls // k, "the object steps the scheduler once per update"
    _compare(eager, graph, params_e, m2, init_p)
    return step, m2, opt2


def _den_step(m, opt, batch, **kw):
    from diamond_amd.train_graph import GraphedTrainStep

    return GraphedTrainStep(m, opt, CLIP, batch, warmup_steps=3, **kw)


def test_warmup_schedule_survives_replay_denoiser():
    """base LR 3e-4, warm-up over 3 updates, clip 1.0, 6 updates"""
    _schedule_case(_denoiser, lambda m: m, _den_step, calls=6, k=1)


def test_gradient_accumulation_over_two_calls():
    """grad_acc_steps=2 over 8 calls: odd calls carry neither `lr` nor `grad_norm_before_clip`; after an update call the gradients
    are zero, in the buffers they always had, and the packed copies are those of the parameters"""
    from diamond_amd import engine as E

    step, m, opt = _schedule_case(_denoiser, lambda m: m, _den_step, calls=8, k=2)
    ptrs = [p.grad.data_ptr() for p in m.parameters()]
    assert all(not bool(p.grad.any()) for p in m.parameters()), "the next micro-step starts from zero gradients"
    batch = SimpleNamespace(**step.static)
    step(batch)
    assert any(bool(p.grad.any()) for p in m.parameters())
    step(batch)
    assert all(not bool(p.grad.any()) for p in m.parameters())
    assert [p.grad.data_ptr() for p in m.parameters()] == ptrs, "the static gradient buffers were re-allocated"
    E.run_weight_audits()
    E.check_weight_audits(wait=True)


def test_construction_with_preserve_state_leaves_no_trace():
    """an optimizer that has taken two eager steps at LR 1e-4: parameters, buffers, optimizer state, LR, scheduler state and both
    generators after construction equal snapshots from before; the first replay is the eager loop's third step (1e-6), which it
    is only if the packed weights were rebuilt from the restored parameters"""
    from diamond_amd import engine as E

    def two_steps():
        m, batches = _denoiser()
        opt = _fused(m, lr=1e-4)
        sched = LambdaLR(opt, lambda s: 1.0)
        _trainer_loop(m, m, opt, sched, batches, 2, 1)
        return m, batches, opt, sched

    m, batches, opt, sched = two_steps()
    third, _ = _trainer_loop(m, m, opt, sched, batches[2:], 1, 1)

    m, batches, opt, sched = two_steps()
    torch.manual_seed(1234)
    torch.cuda.manual_seed(4321)
    before = SimpleNamespace(model=copy.deepcopy(m.state_dict()), buffers=[b.detach().clone() for b in m.buffers()],
                             state={p: {k: v.detach().clone() for k, v in opt.state[p].items()} for p in m.parameters() if p in opt.state},
                             sched=copy.deepcopy(sched.state_dict()), cpu=torch.get_rng_state(), dev=torch.cuda.get_rng_state())
    step = _den_step(m, opt, batches[0], lr_scheduler=sched, preserve_state=True)
    assert torch.equal(torch.get_rng_state(), before.cpu) and torch.equal(torch.cuda.get_rng_state(), before.dev)
    now = m.state_dict()
    assert now.keys() == before.model.keys() and all(torch.equal(now[k], v) for k, v in before.model.items())
    assert all(torch.equal(a, b) for a, b in zip(m.buffers(), before.buffers))
    assert before.state and {p for p in m.parameters() if p in opt.state} == set(before.state)
    for p, saved in before.state.items():
        assert opt.state[p].keys() == saved.keys()
        for k, v in saved.items():
            assert torch.equal(opt.state[p][k], v), k
        assert float(opt.state[p]["step"]) == 2.0
    assert sched.state_dict() == before.sched and sched.last_epoch == 2
    assert all(float(g["lr"]) == float(torch.tensor(1e-4, dtype=torch.float32)) for g in opt.param_groups)
    loss, metrics = step(batches[2])
    assert abs(float(loss) - third[0]) <= 1e-6 * abs(third[0]), (float(loss), third)
    assert metrics["lr"] == 1e-4
    E.run_weight_audits()
    E.check_weight_audits(wait=True)


def test_fresh_optimizer_state_is_zero_after_a_traceless_construction():
    """no optimizer state before: zero moments and step 0 afterwards (the entries exist: the graph holds their pointers)"""
    m, batches = _denoiser()
    init = _params(m)
    opt = _plain_two_groups(m)
    _den_step(m, opt, batches[0], lr_scheduler=_warmup(opt), preserve_state=True, adopt_optimizer=True)
    assert len(opt.state) > 0
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), init[k]), k
        if p not in opt.state:
            continue
        st = opt.state[p]
        assert float(st["step"]) == 0.0 and st["step"].is_cuda and not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()), k
    assert [g["weight_decay"] for g in opt.param_groups] == [1e-2, 0.0]


def test_adopted_optimizer_resumes_from_a_checkpoint():
    """3 graphed updates on an adopted configure_opt-style optimizer, a checkpoint through torch.save, fresh objects, a new step
    with adopt_optimizer + preserve_state, 3 more updates: the losses and the final parameters of 6 uninterrupted updates"""
    kw = dict(preserve_state=True, adopt_optimizer=True)

    m, batches = _denoiser()
    init = copy.deepcopy(m.state_dict())
    opt = _plain_two_groups(m)
    sched = _warmup(opt)
    whole = _graph_loop(_den_step(m, opt, batches[0], lr_scheduler=sched, **kw), batches, 6, 1)
    params_whole = _params(m)

    m1, batches1 = _denoiser()
    m1.load_state_dict(init)
    init_p = _params(m1)
    opt1 = _plain_two_groups(m1)
    sched1 = _warmup(opt1)
    first = _graph_loop(_den_step(m1, opt1, batches1[0], lr_scheduler=sched1, **kw), batches1, 3, 1)
    buf = io.BytesIO()
    torch.save({"model": m1.state_dict(), "opt": opt1.state_dict(), "sched": sched1.state_dict()}, buf)
    buf.seek(0)
    ckpt = torch.load(buf, weights_only=False)

    m2, batches2 = _denoiser()
    opt2 = _plain_two_groups(m2)
    sched2 = _warmup(opt2)
    m2.load_state_dict(ckpt["model"])
    opt2.load_state_dict(ckpt["opt"])
    sched2.load_state_dict(ckpt["sched"])
    step2 = _den_step(m2, opt2, batches2[0], lr_scheduler=sched2, **kw)
    assert len(opt2.state) > 0 and all(float(st["step"]) == 3.0 for st in opt2.state.values())
    second = _graph_loop(step2, batches2, 3, 1, first=3)
    assert all(float(st["step"]) == 6.0 for st in opt2.state.values())
    assert [g["weight_decay"] for g in opt2.param_groups] == [1e-2, 0.0]
    _compare(whole, (first[0] + second[0], first[1] + second[1]), params_whole, m2, init_p)


def test_warmup_schedule_survives_replay_rew_end_model():
    """test_warmup_schedule_survives_replay_denoiser's assertions through graphed_rew_end_step(..., lr_scheduler=...): the logged LRs,
    the parameters bitwise untouched by update 1 and moved by update 2, losses (1e-6) and gradient norms (1e-5) against the eager
    float-LR loop.  The final parameters (1e-5) are compared with the same eager loop on an optimizer whose LR is the fp32 device
    tensor: this fixture's encoder has attention, and the gradient of the KEY third of a `qkv_proj.bias` is analytically zero (a
    soft-max does not see a constant added to every key), i.e. rounding noise of ~1e-11 that Adam's m / sqrt(v) turns into
    updates of the order of the LR, whose sign follows the last bit of everything before it.  Measured on the MI355X: the eager
    loop twice, bitwise equal; the graphed step against the eager loop on the tensor LR, bitwise equal (every parameter); either
    against the eager float-LR loop (3e-4 / 3 is not an fp32 number), 1.35e-4, 5.5e-5 and 4.4e-5 on the three `attn.qkv_proj.bias`
    and at most 2.2e-6 on every other parameter.  The denoiser of the tests above and the default reward / end model have no
    attention, and are compared with the float-LR loop."""
    from diamond_amd.train_graph import graphed_rew_end_step
    from tests.test_rew_end_graph import _group_batch, _group_model

    def fwd_of(m):
        def fwd(batch):
            m.put_back_final_observations(batch)
            return m.forward_static(batch)
        return fwd

    _schedule_case(lambda: (_group_model(DEV), [_group_batch(DEV)]), fwd_of,
                   lambda m, opt, batch, **kw: graphed_rew_end_step(m, opt, CLIP, batch, warmup_steps=3, **kw), calls=6, k=1,
                   parameters_against_a_tensor_lr=True)


@pytest.mark.parametrize("arm", ["plain", "lr_scheduler"])
def test_the_call_does_not_synchronise_with_the_host(arm):
    """calls 2-8 under torch.cuda.set_sync_debug_mode("error"): copy into the static buffers, replay, the scheduler's fill_ of the
    device LR, and the metrics -- nothing reads the device or waits for it (`plain`: the call as it was before the new arguments)"""
    m, batches = _denoiser()
    opt = _fused(m)
    step = _den_step(m, opt, batches[0], **({} if arm == "plain" else dict(lr_scheduler=_warmup(opt), preserve_state=True)))
    kept = [step(batches[0])[0].clone()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(1, 8):
            loss, metrics = step(batches[i % 3])
            kept.append(loss.clone())
            if arm == "lr_scheduler":
                assert isinstance(metrics["lr"], float)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    losses = [float(x) for x in kept]
    assert len(set(losses)) == 8 and all(x == x for x in losses), losses


def test_defaults_are_unchanged():
    """passing lr_scheduler=None, grad_acc_steps=1 (and the other defaults) explicitly against passing nothing: the losses of 4
    replays bit for bit; a plain AdamW without adopt_optimizer is still rejected"""
    from diamond_amd.train_graph import GraphedTrainStep

    got = []
    for kw in ({}, dict(lr_scheduler=None, step_scheduler=True, grad_acc_steps=1, preserve_state=False, adopt_optimizer=False)):
        m, batches = _denoiser()
        step = GraphedTrainStep(m, _fused(m), CLIP, batches[0], **kw)
        out = []
        for i in range(4):
            loss, metrics = step(batches[i % 3])
            assert "lr" not in metrics and metrics is step.metrics
            out.append(float(loss))
        got.append(out)
    print("defaults", got)
    assert got[0] == got[1] and len(set(got[0])) == 4, got
    m, batches = _denoiser()
    with pytest.raises(AssertionError, match="capturable"):
        GraphedTrainStep(m, torch.optim.AdamW(m.parameters(), lr=1e-4), CLIP, batches[0])
    with pytest.raises(AssertionError, match="capturable"):
        GraphedTrainStep(m, torch.optim.AdamW(m.parameters(), lr=1e-4), CLIP, batches[0], adopt_optimizer=False, lr_scheduler=None)
