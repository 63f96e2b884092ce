"""The reward / end model's training step as one replayed hipGraph (train_graph.graphed_rew_end_step) and the pieces it is made of:

  dmd_rew_end_loss            both masked cross-entropies, their gradient and both confusion matrices in one launch
  lstm_native.LstmSegmentFn   the segment LSTM as one autograd node (one dW_hh GEMM, one bias sum)
  RewEndModel.put_back_final_observations / forward_static     `forward` without a host round trip or a data-dependent shape
  GraphedTrainStep(step_fn=, stage=)

CPU: the kernels on the SIMT interpreter (tests/simt), every kernel argument of the loss between inaccessible pages.  GPU (`-m gpu`):
the reference's fixtures, the replayed graph against the eager loop, and a repeat over poisoned free memory."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import group_width_configs as W
from tests.conftest import WEIGHT_SEED, load_golden
from tests.simt import loader as S
from tests.simt.fence import fenced as G
from tests.simt.host_harness import engine_on_interpreter

DEV = "cuda"


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------------------------------
# dmd_rew_end_loss against an fp64 numpy restatement (reference rew_end_model.py:72-88)
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_ref(logits, rew, end, mask):
    """fp64: (losses (2,), dlogits (R, 5), counts (13,)) of the masked means; an empty mask: NaN, zeros, zeros"""
    m = mask.astype(bool)
    n = int(m.sum())
    rows = np.arange(logits.shape[0])
    losses, ds, cms = [], [], []
    for cols, tgt, k in ((slice(0, 3), np.sign(rew).astype(np.int64) + 1, 3), (slice(3, 5), (end != 0).astype(np.int64), 2)):
        lg = logits[:, cols].astype(np.float64)
        z = lg - lg.max(axis=1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        nll = -logp[rows, tgt]
        losses.append(nll[m].sum() / n if n else np.nan)
        d = (np.exp(logp) - np.eye(k)[tgt]) * m[:, None]
        ds.append(d / n if n else np.zeros_like(d))
        cm = np.zeros((k, k), dtype=np.int64)
        np.add.at(cm, (tgt[m], lg.argmax(axis=1)[m]), 1)  # (numpy's argmax: the first maximum, like torch's on the CPU)
        cms.append(cm.reshape(-1))
    return np.array(losses), np.concatenate(ds, axis=1), np.concatenate(cms)


def _loss_inputs(r, mask_kind, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((r, 5)) * 3).astype(np.float32)
    for i in range(r):
        if i % 7 == 0:
            logits[i, 1] = logits[i, 0] = np.float32(abs(logits[i, 2]) + 0.5)  # a tie at the top of the reward head
        if i % 7 == 3:
            logits[i, 2] = logits[i, 1]  # a tie that may or may not be the maximum
        if i % 5 == 0:
            logits[i, 4] = logits[i, 3]  # a tie in the end head
        if i % 11 == 2:
            logits[i] = np.float32(80) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), 5)
    if seed % 2:
        rew = rng.choice(np.array([-2.5, -0.0, 0.0, 3.0], dtype=np.float32), r)
    else:
        rew = rng.integers(-2, 3, r).astype(np.float32)
    end = (rng.random(r) < 0.3).astype(np.int64)
    mask = {"all": np.ones(r, np.uint8), "none": np.zeros(r, np.uint8)}.get(mask_kind)
    if mask_kind == "tail":
        mask = (np.arange(r) < max(1, (2 * r) // 3)).astype(np.uint8)
    elif mask_kind == "single":
        mask = np.zeros(r, np.uint8)
        mask[r // 2] = 1
    return logits, rew, end, mask


def _run_loss(logits, rew, end, mask):
    r = logits.shape[0]
    losses, dlogits, counts = G(np.full(2, 7.0, np.float32)), G(np.full((r, 5), np.nan, np.float32)), G(np.full(13, -1, np.int64))
    S.check(S.lib().dmd_rew_end_loss(S.ptr(G(logits)), S.ptr(G(rew)), S.ptr(G(end)), S.ptr(G(mask)), S.ptr(losses), S.ptr(dlogits),
                                     S.ptr(counts), r, None), "dmd_rew_end_loss")
    return losses.copy(), dlogits.copy(), counts.copy()


@pytest.mark.parametrize("mask_kind", ["all", "tail", "single", "none"])
@pytest.mark.parametrize("r", [1, 5, 63, 64, 65, 255, 256, 257, 1000])
def test_rew_end_loss_kernel_vs_fp64(r, mask_kind, monkeypatch):
    """wave and workgroup boundaries, several strides per thread; losses within 1e-6 * max(1, |ref|) (an fp32 log-soft-max over at
    most 3 entries is a few ulp, the sums are fp64), dlogits within 1e-6 of its max-abs and exactly zero on unmasked rows, counts
    equal, an empty mask NaN / zeros / zeros; the same bits under two wave schedules of the interpreter"""
    for seed in (r, r + 1):  # rewards in {-2 ... 2} (even seed) and in {-2.5, -0.0, 0.0, 3} (odd seed)
        logits, rew, end, mask = _loss_inputs(r, mask_kind, seed)
        want_l, want_d, want_c = _loss_ref(logits, rew, end, mask)
        monkeypatch.setenv("SIMT_SCHEDULE", "0")
        losses, dlogits, counts = _run_loss(logits, rew, end, mask)
        np.testing.assert_array_equal(counts, want_c)
        assert np.all(dlogits[mask == 0] == 0.0)
        if mask.sum() == 0:
            assert np.isnan(losses).all() and np.all(dlogits == 0.0) and np.all(counts == 0)
        else:
            assert np.all(np.abs(losses - want_l) <= 1e-6 * np.maximum(1.0, np.abs(want_l))), (losses, want_l)
            assert np.abs(dlogits - want_d).max() <= 1e-6 * np.abs(want_d).max(), (np.abs(dlogits - want_d).max(), np.abs(want_d).max())
        monkeypatch.setenv("SIMT_SCHEDULE", "1")
        again = _run_loss(logits, rew, end, mask)
        for a, b in zip((losses, dlogits, counts), again):
            assert a.tobytes() == b.tobytes(), "the result depends on the wave schedule"


def test_rew_end_loss_rejects_row_counts_outside_its_range():
    logits, rew, end, mask = _loss_inputs(4, "all", 0)
    out = (np.zeros(2, np.float32), np.zeros((4, 5), np.float32), np.zeros(13, np.int64))
    for r in (0, -3, (1 << 20) + 1):
        rc = S.lib().dmd_rew_end_loss(S.ptr(logits), S.ptr(rew), S.ptr(end), S.ptr(mask), *(S.ptr(o) for o in out), r, None)
        assert rc != 0 and b"rew_end_loss" in S.lib().dmd_last_error()


def test_rew_end_loss_autograd_scales_the_two_heads_by_their_upstream_gradients():
    """grad_ops.rew_end_loss: backward = dlogits times the two upstream scalars over columns [0, 0, 0, 1, 1] (2e-6 of the max-abs:
    the kernel's 1e-6 plus the rounding of that one fp32 multiply)"""
    from diamond_amd import grad_ops as GO

    logits, rew, end, mask = (torch.from_numpy(a) for a in _loss_inputs(37, "tail", 4))
    lg = logits.clone().requires_grad_(True)
    with engine_on_interpreter():
        losses, counts = GO.rew_end_loss(lg, rew, end, mask.bool())
        (2.0 * losses[0] - 0.5 * losses[1]).backward()
    _, want_d, want_c = _loss_ref(*(a.numpy() for a in (logits, rew, end, mask)))
    want = torch.from_numpy(want_d) * torch.tensor([2.0, 2.0, 2.0, -0.5, -0.5], dtype=torch.float64)
    assert counts.dtype == torch.int64 and not counts.requires_grad and np.array_equal(counts.numpy(), want_c)
    assert float((lg.grad.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# LstmSegmentFn against T chained LstmStepFn calls and against torch.nn.LSTM in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _lstm_case(t, b=3, f=48, hd=32, seed=3):
    g = torch.Generator().manual_seed(seed)
    lstm = torch.nn.LSTM(f, hd, batch_first=True)
    for p in lstm.parameters():
        p.data = torch.randn(p.shape, generator=g) * 0.3
    x = torch.randn(t, b, f, generator=g)
    gx = (x.reshape(t * b, f) @ lstm.weight_ih_l0.detach().t() + lstm.bias_ih_l0.detach()).reshape(t, b, 4 * hd)
    wts = torch.randn(t, b, hd, generator=g)
    return lstm, gx, wts


def _lstm_run(kind, lstm, gx, wts):
    """(ys (T, B, hd), dgx, dW_hh, db_hh) of loss = sum(ys * wts)"""
    from diamond_amd import engine as E
    from diamond_amd.lstm_native import LstmStepFn, lstm_segment

    t, b, hd = wts.shape
    gx = gx.clone().requires_grad_(True)
    lstm.zero_grad()
    cache = E.PackCache()
    with engine_on_interpreter():
        if kind == "segment":
            ys = lstm_segment(cache, gx, lstm)
        else:
            gx_bt = gx.transpose(0, 1)  # (B, T, 4 hd) as logits_with_grad slices it
            hx, cx, out = torch.zeros(b, hd), torch.zeros(b, hd), []
            for i in range(t):
                hx, cx = LstmStepFn.apply(cache, gx_bt[:, i], hx, cx, lstm.weight_hh_l0, lstm.bias_hh_l0)
                out.append(hx)
            ys = torch.stack(out, dim=0)
        (ys * wts).sum().backward()
    return ys.detach(), gx.grad.clone(), lstm.weight_hh_l0.grad.clone(), lstm.bias_hh_l0.grad.clone()


def _lstm_fp64(lstm, gx, wts):
    """torch.nn.LSTM in fp64 autograd; the input projection enters through an identity weight_ih, so that gx is its input"""
    t, b, hd = wts.shape
    ref = torch.nn.LSTM(4 * hd, hd).double()
    with torch.no_grad():
        ref.weight_ih_l0.copy_(torch.eye(4 * hd))
        ref.bias_ih_l0.zero_()
        ref.weight_hh_l0.copy_(lstm.weight_hh_l0.double())
        ref.bias_hh_l0.copy_(lstm.bias_hh_l0.double())
    g64 = gx.double().requires_grad_(True)
    ys, _ = ref(g64)
    (ys * wts.double()).sum().backward()
    return ys.detach(), g64.grad, ref.weight_hh_l0.grad, ref.bias_hh_l0.grad


def test_lstm_segment_is_the_chained_steps_with_one_weight_gradient():
    """B = 3, T = 5, F = 48, hd = 32: ys and dgx bitwise the T chained LstmStepFn calls; dW_hh / db_hh within 1e-6 of the chained
    path's max-abs (a reordering of at most 15 fp32 addends); everything within 1e-5 of torch.nn.LSTM in fp64"""
    lstm, gx, wts = _lstm_case(5)
    seg = _lstm_run("segment", lstm, gx, wts)
    chain = _lstm_run("chain", lstm, gx, wts)
    assert torch.equal(seg[0], chain[0]), "ys"
    assert torch.equal(seg[1], chain[1]), "dgx"
    for name, a, c in (("dW_hh", seg[2], chain[2]), ("db_hh", seg[3], chain[3])):
        assert float((a - c).abs().max()) <= 1e-6 * float(c.abs().max()), name
    for name, a, r in zip(("ys", "dgx", "dW_hh", "db_hh"), seg, _lstm_fp64(lstm, gx, wts)):
        assert rel_err(a, r) < 1e-5, (name, rel_err(a, r))


def test_lstm_segment_of_one_step_has_no_recurrent_weight_gradient():
    lstm, gx, wts = _lstm_case(1)
    ys, dgx, dw_hh, db_hh = _lstm_run("segment", lstm, gx, wts)
    ys_c, dgx_c, _, db_c = _lstm_run("chain", lstm, gx, wts)
    assert torch.equal(ys, ys_c) and torch.equal(dgx, dgx_c)
    assert dw_hh.shape == lstm.weight_hh_l0.shape and bool((dw_hh == 0).all())
    assert float((db_hh - db_c).abs().max()) <= 1e-6 * float(db_c.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# the whole step on groups.pt["rew_end_train"] (32 x 32, b = 2, t = 4), on the interpreter
# ---------------------------------------------------------------------------------------------------------------------------
class _LaunchCounter:
    """nv.PROFILER stand-in: counts the dmd_* launches, the dmd_linear ones by (M, N)"""

    def __init__(self):
        self.counts, self.linears, self._pending = {}, {}, None

    def annotate(self, key, flops, nbytes):
        self._pending = key

    def call(self, name, fn, args):
        self._pending = None
        self.counts[name] = self.counts.get(name, 0) + 1
        if name == "dmd_linear":
            p = args[0]._obj
            self.linears[(p.M, p.N)] = self.linears.get((p.M, p.N), 0) + 1
        return fn(*args)


def _group_model(dev="cpu"):
    from diamond_amd.rew_end_model import RewEndModel, RewEndModelConfig
    from diamond_amd.testing import fill_module_

    m = RewEndModel(RewEndModelConfig(**W.REW_END))
    fill_module_(m, W.WEIGHT_SEED + 1)
    return m.to(dev).train()


def _group_batch(dev="cpu"):
    d = W.rew_end_train_batch(torch.Generator().manual_seed(41))
    batch = SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()})
    batch.info[1]["final_observation"] = batch.info[1]["final_observation"].to(dev)
    return batch


@pytest.fixture(scope="module")
def group_step():
    """One run of everything the CPU tests below look at (the interpreter needs seconds per pass): `forward` on one copy of the
    batch, then on another copy put_back_final_observations, logits_with_grad, forward_static and backward."""
    from diamond_amd import grad_ops as GO
    from diamond_amd import native as nv

    m = _group_model()
    out = SimpleNamespace(model=m)
    seen = {}
    real = GO.rew_end_loss

    def spy(logits, *a):
        seen["logits"] = logits.detach().clone()
        return real(logits, *a)

    saved = nv.PROFILER
    try:
        with engine_on_interpreter():
            b0 = _group_batch()
            _, out.logs_forward = m(b0)
            out.obs_forward = b0.obs.clone()
            b1 = _group_batch()
            out.obs_before = b1.obs.clone()
            m.put_back_final_observations(b1)
            out.obs_static = b1.obs.clone()
            nv.PROFILER = out.chained = _LaunchCounter()
            out.logits_chained = m.logits_with_grad(b1.obs[:, :-1], b1.act[:, :-1], b1.obs[:, 1:]).detach().clone()
            nv.PROFILER = out.static = _LaunchCounter()
            GO.rew_end_loss = spy
            m.zero_grad()
            out.loss, out.logs = m.forward_static(b1)
            out.static_forward_launches = dict(out.static.counts)
            out.loss.backward()
            out.obs_after = b1.obs.clone()
    finally:
        nv.PROFILER, GO.rew_end_loss = saved, real
    out.logits_static = seen["logits"].reshape(out.logits_chained.shape)
    return out


def test_static_step_meets_the_reference_fixture(group_step):
    """losses, every gradient and every gradient norm at the 1e-4 bars of test_group_width_rew_end_model_vs_reference_golden"""
    from tests.test_group_widths import GOLD, _grad_errors

    r = torch.load(GOLD, weights_only=False)["rew_end_train"]
    s = group_step
    errs = {"loss": rel_err(s.loss.detach(), r["loss"]), "loss_rew": rel_err(s.logs["loss_rew"], r["loss_rew"]),
            "loss_end": rel_err(s.logs["loss_end"], r["loss_end"]), **_grad_errors(s.model, r)}
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


def test_static_step_has_forwards_logits_bit_for_bit_and_its_metrics(group_step):
    s = group_step
    assert torch.equal(s.logits_static, s.logits_chained)
    assert set(s.logs) == set(s.logs_forward) == {"loss_rew", "loss_end", "loss_total", "confusion_matrix"}
    for k, shape in (("rew", (3, 3)), ("end", (2, 2))):
        cm = s.logs["confusion_matrix"][k]
        assert cm.dtype == torch.int64 and tuple(cm.shape) == shape and torch.equal(cm, s.logs_forward["confusion_matrix"][k])
    for k in ("loss_rew", "loss_end", "loss_total"):
        assert s.logs[k].dtype == s.logs_forward[k].dtype and not s.logs[k].requires_grad
        assert rel_err(s.logs[k], s.logs_forward[k]) < 1e-6
    assert torch.equal(s.logs["loss_total"], s.loss.detach())


def test_put_back_writes_what_forward_writes(group_step):
    s = group_step
    assert torch.equal(s.obs_static, s.obs_forward) and not torch.equal(s.obs_static, s.obs_before)
    assert torch.equal(s.obs_after, s.obs_static), "forward_static must leave the batch alone"


def test_put_back_leaves_a_batch_without_an_end_untouched():
    """key presence alone decides nothing: a sample that carries a final_observation but does not end inside the segment keeps its
    frames (the device-side `where`); so does a batch without the key, and one whose only end is the segment's last step"""
    m = _group_model()
    for case in ("key without end", "no key", "end at the last step only"):
        b = _group_batch()
        b.end.zero_()
        if case == "no key":
            b.info = [{} for _ in b.info]
        if case == "end at the last step only":
            b.end[1, -1] = 1  # end[:, :-1] is what the reference looks at
        before = b.obs.clone()
        m.put_back_final_observations(b)
        assert torch.equal(b.obs, before), case


def test_segment_has_one_recurrent_weight_gradient_gemm(group_step):
    """dW_hh is a (4 hd, hd) GEMM: one launch for the segment, against one per step on the chained path (counted in the forward
    only there: the shapes of the step's other dmd_linear launches differ)"""
    s, m = group_step, group_step.model
    hd, t = m.cfg.lstm_dim, 3
    assert s.static.linears.get((4 * hd, hd), 0) == 1, s.static.linears
    assert s.static.counts["dmd_lstm_pointwise"] == s.chained.counts["dmd_lstm_pointwise"] == t
    assert s.static.counts["dmd_lstm_pointwise_bwd"] == t
    assert s.static.counts["dmd_rew_end_loss"] == 1
    # per step the launches LstmStepFn issues; everything else of the forward is logits_with_grad's, launch for launch
    fwd = dict(s.static_forward_launches)
    assert fwd.pop("dmd_rew_end_loss") == 1
    assert fwd == s.chained.counts, (fwd, s.chained.counts)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _default_model(img_size=64):
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    agent = D.Agent(D.default_agent_config(img_size=img_size))
    fill_module_(agent, WEIGHT_SEED)
    return agent.to(DEV).eval().rew_end_model.train()


def _on_dev(d):
    batch = SimpleNamespace(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()})
    batch.info = [{k: v.to(DEV) for k, v in i.items()} for i in batch.info]
    return batch


def _static_step(m, batch):
    m.zero_grad(set_to_none=True)
    m.put_back_final_observations(batch)
    loss, logs = m.forward_static(batch)
    loss.backward()
    return loss.detach(), logs


FIXTURES = ["rew_end_train.pt", "rew_end_train_72x72.pt", "groups.pt"]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x2", "f32"])
@pytest.mark.parametrize("fixture", FIXTURES)
def test_static_training_step_vs_reference_golden(fixture, precision):
    """forward_static + backward against the reference's losses, gradients and gradient norms at the fixtures' 1e-4 bars, and its
    confusion matrices where the fixture has them"""
    from diamond_amd import unet_train as UT
    from diamond_amd.testing import rew_end_train_batch

    if fixture == "groups.pt":
        gold = load_golden(fixture)["rew_end_train"]
        m, batch = _group_model(DEV), _group_batch(DEV)
        sample = W.sample_grad
    else:
        gold = load_golden(fixture)
        size = gold.get("size", 64)
        m = _default_model(size)
        batch = _on_dev(rew_end_train_batch(torch.Generator().manual_seed(gold["seed"]), h=size, w=size))
        stride = gold.get("stride", 13)
        sample = lambda g, ref: g if ref.shape == g.shape else g.flatten()[::stride]
    UT.TRAIN_PRECISION = precision
    try:
        loss, logs = _static_step(m, batch)
    finally:
        UT.TRAIN_PRECISION = "f16x2"
    if "cm_rew" in gold:
        assert torch.equal(logs["confusion_matrix"]["rew"].cpu(), gold["cm_rew"])
        assert torch.equal(logs["confusion_matrix"]["end"].cpu(), gold["cm_end"])
    errs = {"loss": rel_err(loss, gold["loss"]), "loss_rew": rel_err(logs["loss_rew"], gold["loss_rew"]),
            "loss_end": rel_err(logs["loss_end"], gold["loss_end"])}
    for k, p in m.named_parameters():
        assert p.grad is not None, f"no gradient for {k}"
        gref = gold["grads"][k]
        errs["grad " + k] = rel_err(sample(p.grad) if fixture == "groups.pt" else sample(p.grad, gref), gref)
        n = float(gold["grad_norms"][k])
        errs["|grad| " + k] = abs(float(p.grad.double().norm()) - n) / (n + 1e-30)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print(f"{fixture} [{precision}]: loss {float(loss):.6f} (ref {float(gold['loss']):.6f}); worst:", [(k, f"{v:.2e}") for k, v in worst])
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, (fixture, precision, bad)


def _graph_batches():
    """three (3, 6) segments at 64 x 64: the end in another sample and step each time and none at all in the second, other padding"""
    from diamond_amd.testing import rew_end_train_batch

    g = torch.Generator().manual_seed(21)
    batches = []
    for k, (who, when, pad) in enumerate([(1, 3, {1: 4, 2: 4}), (None, None, {0: 3}), (2, 1, {2: 2, 0: 5})]):
        d = rew_end_train_batch(g)
        final = d["info"][1]["final_observation"]
        d["end"].zero_()
        d["mask_padding"].fill_(True)
        d["info"] = [{} for _ in range(3)]
        if who is not None:
            d["end"][who, when] = 1
            d["info"][who]["final_observation"] = final
        for row, start in pad.items():
            d["mask_padding"][row, start:] = False
        batches.append(_on_dev(d))
    return batches


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True], ids=["foreach", "fused"])
def test_graphed_rew_end_step_matches_the_eager_loop(fused):
    """graphed_rew_end_step against the eager loop on forward_static, same weights: two warm-up and four measured steps over three
    cycled batches, AdamW capturable, clip at 100 -- at the bars of tests/test_gpu_train_graph.py, and the confusion matrices of
    every replay equal to the eager step's"""
    from diamond_amd.train_graph import graphed_rew_end_step

    warm, steps = 2, 4
    m = _default_model()
    init = copy.deepcopy(m.state_dict())
    opt = torch.optim.AdamW(m.parameters(), lr=3e-4, capturable=True, fused=fused)
    batches = _graph_batches()
    losses_e, cms_e = [], []
    for i in range(warm + steps):
        batch = batches[0] if i < warm else batches[(i - warm) % 3]
        loss, logs = _static_step(m, batch)
        torch.nn.utils.clip_grad_norm_(m.parameters(), 100.0)
        opt.step()
        if i >= warm:
            losses_e.append(float(loss))
            cms_e.append({k: v.cpu().clone() for k, v in logs["confusion_matrix"].items()})
        del loss, logs
    opt.zero_grad(set_to_none=True)
    params_e = {k: v.detach().clone() for k, v in m.named_parameters()}

    m2 = _default_model()
    m2.load_state_dict(init)
    opt2 = torch.optim.AdamW(m2.parameters(), lr=3e-4, capturable=True, fused=fused)
    batches2 = _graph_batches()
    gstep = graphed_rew_end_step(m2, opt2, 100.0, batches2[0], warmup_steps=warm)
    losses_g = []
    for i in range(steps):
        loss, metrics = gstep(batches2[i % 3])
        losses_g.append(float(loss))
        assert float(metrics["loss_total"]) == losses_g[-1]
        for k in ("rew", "end"):
            cm = metrics["confusion_matrix"][k]
            assert cm.dtype == torch.int64 and torch.equal(cm.cpu(), cms_e[i][k]), (i, k, cm, cms_e[i][k])
    torch.cuda.synchronize()
    print("eager", losses_e, "graph", losses_g)
    assert len(set(losses_g)) == steps, "the replayed step must see the new batch / the updated weights"
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-6 * abs(a), (losses_e, losses_g)
    worst = max(float((p.detach() - params_e[k]).abs().max() / params_e[k].abs().max().clamp_min(1e-12)) for k, p in m2.named_parameters())
    moved = max(float((p.detach() - init[k]).abs().max()) for k, p in m2.named_parameters())
    assert moved > 1e-4, "parameters did not train"
    assert worst < 1e-5, f"parameters after {warm}+{steps} steps differ from the eager loop by {worst:.3e}"


def test_graphed_step_without_the_new_arguments_is_the_model_call():
    """step_fn defaults to the model, stage to nothing"""
    import inspect

    from diamond_amd.train_graph import GraphedTrainStep

    sig = inspect.signature(GraphedTrainStep.__init__).parameters
    assert sig["step_fn"].default is None and sig["stage"].default is None
    assert sig["fields"].default == ("obs", "act", "mask_padding")


@pytest.mark.gpu
def test_static_step_is_bitwise_reproducible_over_poisoned_memory():
    """forward_static + backward twice from the same weights, the allocator's free blocks holding NaN before the first and 1e30
    before the second: the loss and every gradient bit for bit (but act_emb.weight's, which torch's own embedding backward forms
    with atomics)"""
    from diamond_amd.testing import rew_end_train_batch
    from tests.test_offgrid_train import _poison_free_memory

    m = _default_model()
    got = []
    for poison in (float("nan"), 1e30):
        batch = _on_dev(rew_end_train_batch(torch.Generator().manual_seed(17)))
        _poison_free_memory(poison)
        loss, _ = _static_step(m, batch)
        got.append((loss.clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = got
    assert torch.equal(l0, l1) and bool(torch.isfinite(l0))
    diff = [k for k in g0 if k != "act_emb.weight" and not torch.equal(g0[k], g1[k])]
    assert not diff, diff
    assert all(bool(torch.isfinite(v).all()) for v in g0.values())
