"""Open-loop evaluation (diamond_amd/openloop.py, dmd_openloop_step) without a GPU:

  * the kernel's own source on the SIMT interpreter (tests/simt): the inputs between inaccessible pages, every output inside
    guard bands, exactly equal to the numpy restatement of tests/openloop_cases.py;
  * the host layer on the interpreter's host harness with stub sampler / reward-end objects that return fixed tensors (the real
    networks take minutes there): id validation, the order of calls, the ring head arithmetic over a wrapping horizon, and
    `summary()` against a numpy computation from the report's tensors.
"""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import openloop_cases as OC
from tests.replay_cases import assert_same, bits, dequant
from tests.simt import loader as S
from tests.simt.fence import fenced as G
from tests.simt.host_harness import engine_on_interpreter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 64  # bytes of guard on both sides of every output


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _banded(init: np.ndarray, misalign: int = 0):
    """A copy of `init` in the middle of a poisoned buffer: (the view the kernel gets, the whole buffer as bytes, its offset).
    The view starts 64-byte aligned (+ `misalign` bytes)."""
    init = np.ascontiguousarray(init)
    raw = np.full(init.nbytes + 2 * BAND + 64 + misalign, 0xA5, np.uint8)
    off = BAND + (-(raw.ctypes.data + BAND) % 64) + misalign
    view = raw[off:off + init.nbytes].view(init.dtype).reshape(init.shape)
    view[...] = init
    return view, raw, off


def _poison(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xFF if np.issubdtype(np.dtype(dtype), np.floating) else 0x5A
    return a


def _run(case, teacher_forced, with_levels=True, tight="end", misalign_pred=False):
    from diamond_amd import native as nv

    L = S.lib()
    arena, seg, pred = case["arena"], case["seg"], case["pred"]
    b, pf = pred.shape
    ins = {k: G(arena[k], tight=tight) for k in ("frames", "act", "rew", "end", "finals")}
    segf = G(seg, tight=tight)
    if misalign_pred:  # 4 bytes off a 16-byte boundary: the entry must leave its vector paths
        predf = G(np.concatenate([np.zeros(1, np.float32), pred.ravel()]))[1:].reshape(b, pf)
        assert predf.ctypes.data % 16 == 4
    else:
        predf = G(pred, tight=tight)
    outs = {"ctx_obs": _banded(case["ctx_obs"]), "ctx_act": _banded(case["ctx_act"]), "metrics": _banded(_poison((b, 4), np.int64)),
            "rew": _banded(_poison(b, np.float32)), "end": _banded(_poison(b, np.uint8)), "valid": _banded(_poison((b, 2), np.uint8))}
    if with_levels:
        outs["levels"] = _banded(_poison((b, pf), np.uint8))
    p = nv.OpenLoopParams()
    p.B, p.T, p.per_frame, p.step, p.head, p.teacher_forced = b, case["T"], pf, case["step"], case["head"], int(teacher_forced)
    p.frames, p.act, p.rew, p.end = (ins[k].ctypes.data for k in ("frames", "act", "rew", "end"))
    p.finals = ins["finals"].ctypes.data if len(arena["finals"]) else None
    p.seg, p.pred = segf.ctypes.data, predf.ctypes.data
    for field, k in (("ctx_obs", "ctx_obs"), ("ctx_act", "ctx_act"), ("metrics", "metrics"), ("out_rew", "rew"), ("out_end", "end"),
                     ("out_valid", "valid"), ("out_levels", "levels")):
        setattr(p, field, outs[k][0].ctypes.data if k in outs else None)
    S.check(L.dmd_openloop_step(ctypes.byref(p), None), "dmd_openloop_step")
    for k, (view, raw, off) in outs.items():
        assert (raw[:off] == 0xA5).all() and (raw[off + view.nbytes:] == 0xA5).all(), f"{k}: bytes around the output were written"
    assert np.array_equal(bits(predf), bits(pred))
    return {k: v[0] for k, v in outs.items()}


def _check(case, teacher_forced, what, **kw):
    got = _run(case, teacher_forced, **kw)
    want = OC.restate(case, teacher_forced)
    assert_same(got, want, tuple(k for k in OC.OUTPUTS if k in got), what)
    head = case["head"]
    others = [s for s in range(case["T"]) if s != head]
    assert np.array_equal(bits(got["ctx_obs"][:, others]), bits(case["ctx_obs"][:, others])), f"{what}: a ring slot other than head changed"
    assert np.array_equal(got["ctx_act"][:, others], case["ctx_act"][:, others])
    return got, want


@pytest.mark.parametrize("teacher_forced", [False, True])
@pytest.mark.parametrize("head", [0, 3])
@pytest.mark.parametrize("per_frame", OC.PER_FRAMES)
def test_openloop_step_matches_the_restatement(per_frame, head, teacher_forced):
    """Every kind of sample in one descriptor (B = 9) and in batches of B = 3, T = 4, for the three lane widths, both ring heads
    and both modes, with and without `out_levels`; the inputs fenced at their ends or (teacher forced) at their starts."""
    case = OC.make_case(per_frame, head, seed=per_frame + head)
    tight = "start" if teacher_forced else "end"
    got, want = _check(case, teacher_forced, "all kinds", tight=tight)
    for i, kind in enumerate(OC.KINDS):
        assert tuple(got["valid"][i]) == OC.EXPECTED_VALID[kind], kind
    eq = OC.KINDS.index("equal to its target")
    assert got["metrics"][eq].tolist() == [0, 0, 0, 0] and (want["metrics"][[0, 1, 2, 6]] > 0).all()
    assert got["ctx_act"][OC.KINDS.index("final observation"), head] == 0  # a final observation has no next action
    forced_differs = [not np.array_equal(bits(got["ctx_obs"][i, head]), bits(case["pred"][i])) for i in range(len(OC.KINDS))]
    assert forced_differs == [bool(teacher_forced and v[0] and k != "equal to its target") for k, v in ((k, OC.EXPECTED_VALID[k]) for k in OC.KINDS)]
    for rows in ([0, 1, 2], [2, 3, 4], [5, 7, 8]):
        _check(OC.rows_of(case, rows), teacher_forced, f"rows {rows}", with_levels=rows[0] != 2, tight=tight)


@pytest.mark.parametrize("step", [0, 2, 3, 200])
def test_openloop_step_other_steps(step):
    """The same descriptor at other steps: the kinds shift along the episodes (step 200: everything is beyond the end)."""
    case = OC.make_case(48, 1, step=step, seed=step)
    got, _ = _check(case, True, f"step {step}", with_levels=False)
    if step == 200:
        assert not got["valid"].any() and not got["metrics"].any()


def test_openloop_step_unaligned_prediction_and_no_finals():
    """per_frame = 48 with a prediction that is not 16-byte aligned (the one-level path must be taken), and an arena without
    final observations (finals = NULL: final_row is never followed)."""
    case = OC.make_case(48, 2, seed=5)
    _check(case, True, "misaligned pred", misalign_pred=True)
    bare = dict(case, arena=dict(case["arena"], finals=case["arena"]["finals"][:0]))
    got, _ = _check(bare, True, "finals = NULL")
    assert tuple(got["valid"][OC.KINDS.index("final observation")]) == (0, 1)


def test_openloop_step_levels_round_and_clamp_like_quantize_u8():
    """Every level +- 0.499 of a level and far outside [-1, 1] through the kernel and through dmd_quantize_u8: the same levels
    (one device function), and the ones the restatement expects."""
    L = S.lib()
    lv = np.arange(256, dtype=np.float64)
    v = np.concatenate([(x / 255.0) * 2.0 - 1.0 for x in (lv, lv + 0.499, lv - 0.499)] + [np.array([-7.0, 9.0, -1.0001, 1.0001])]).astype(np.float32)
    case = OC.make_case(len(v), 0, seed=2)
    case["pred"][:] = v
    got, _ = _check(case, False, "levels")
    q, flag = G(np.zeros(len(v), np.uint8)), G(np.zeros(1, np.int32))
    S.check(L.dmd_quantize_u8(G(v).ctypes.data, q.ctypes.data, flag.ctypes.data, len(v), None), "dmd_quantize_u8")
    assert np.array_equal(got["levels"][0], q)
    assert q[:768].tolist() == 3 * list(range(256)) and q[768:].tolist() == [0, 255, 0, 255]


def test_openloop_step_refuses_bad_arguments():
    from diamond_amd import native as nv

    L = S.lib()
    case = OC.make_case(20, 0)
    arena, b = case["arena"], len(case["seg"])
    keep = {k: G(arena[k]) for k in ("frames", "act", "rew", "end", "finals")}
    keep.update(seg=G(case["seg"]), pred=G(case["pred"]), ctx_obs=G(case["ctx_obs"]), ctx_act=G(case["ctx_act"]), metrics=G(np.zeros((b, 4), np.int64)),
                out_rew=G(np.zeros(b, np.float32)), out_end=G(np.zeros(b, np.uint8)), out_valid=G(np.zeros((b, 2), np.uint8)))

    def params(**kw):
        p = nv.OpenLoopParams()
        p.B, p.T, p.per_frame, p.step, p.head, p.teacher_forced = b, OC.T, 20, 1, 0, 0
        for k, v in keep.items():
            setattr(p, k, v.ctypes.data)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert L.dmd_openloop_step(ctypes.byref(params()), None) == 0
    assert L.dmd_openloop_step(ctypes.byref(params(B=0)), None) == 0
    for bad in (dict(T=0), dict(B=-1), dict(per_frame=0), dict(step=-1), dict(head=-1), dict(head=OC.T), dict(teacher_forced=2), dict(frames=None),
                dict(act=None), dict(rew=None), dict(end=None), dict(seg=None), dict(pred=None), dict(ctx_obs=None), dict(ctx_act=None),
                dict(metrics=None), dict(out_rew=None), dict(out_end=None), dict(out_valid=None)):
        assert L.dmd_openloop_step(ctypes.byref(params(**bad)), None) != 0, bad
        assert b"openloop_step" in L.dmd_last_error()
    assert L.dmd_openloop_step(None, None) != 0


def test_openloop_params_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of the ctypes mirror against the C struct (compiled with gcc from include/diamond_hip.h)."""
    from diamond_amd import native as nv

    fields = [f for f, _ in nv.OpenLoopParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_openloop_params));' + "".join(f'printf("%zu ", offsetof(dmd_openloop_params, {f}));' for f in fields)
    src = tmp_path / "s.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    mine = [ctypes.sizeof(nv.OpenLoopParams)] + [getattr(nv.OpenLoopParams, f).offset for f in fields]
    assert got == mine, list(zip(["sizeof"] + fields, got, mine))
    assert "dmd_openloop_step" in nv.EXPORTS and "dmd_openloop_step" in nv.LAUNCHERS


# ---------------------------------------------------------------------------------------------------------------------------
# the host layer, on stubs
# ---------------------------------------------------------------------------------------------------------------------------
FRAME = (3, 4, 4)
T = 4


def _ep(n, seed, end_last=False, final=False):
    g = torch.Generator().manual_seed(seed)
    end = torch.zeros(n, dtype=torch.uint8)
    end[-1] = int(end_last)
    info = {"final_observation": torch.randint(0, 256, FRAME, generator=g, dtype=torch.uint8)} if final else {}
    return SimpleNamespace(obs=torch.randint(0, 256, (n,) + FRAME, generator=g, dtype=torch.uint8), act=torch.randint(0, 4, (n,), generator=g),
                           rew=torch.randint(-1, 2, (n,), generator=g).float(), end=end, trunc=torch.zeros(n, dtype=torch.uint8), info=info)


class _StubSampler:
    """`sample_ring` returns a fixed frame per call (on the grid, a few levels off the ring's newest frame) and records the call."""

    def __init__(self, log):
        self.denoiser = SimpleNamespace(cfg=SimpleNamespace(inner_model=SimpleNamespace(num_steps_conditioning=T)))
        self.log = log
        self.preds = []

    def sample_ring(self, ctx_obs, ctx_act, obs_head, act_head):
        assert ctx_obs.is_contiguous() and ctx_act.dtype == torch.int64
        self.log.append(("sample", obs_head, act_head, ctx_obs.clone(), ctx_act.clone()))
        g = torch.Generator().manual_seed(len(self.preds))
        lv = torch.randint(0, 256, (ctx_obs.shape[0],) + FRAME, generator=g)
        self.preds.append(lv)
        return lv.float().div(255).mul(2).sub(1), []


class _StubRewEnd:
    def __init__(self, log):
        self.log = log
        self.calls = 0

    def predict_rew_end(self, obs, act, next_obs, hx_cx=None):
        b, t = act.shape
        self.log.append(("rew_end", obs.clone(), act.clone(), next_obs.clone(), hx_cx))
        g = torch.Generator().manual_seed(100 + self.calls)
        self.calls += 1
        return torch.randn(b, t, 3, generator=g), torch.randn(b, t, 2, generator=g), (torch.full((1, b, 2), float(self.calls)), torch.zeros(1, b, 2))


@pytest.fixture()
def store():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        eps = [_ep(14, 1), _ep(9, 2, end_last=True, final=True), _ep(8, 3, end_last=True)]
        for e in eps:
            s.add_episode(e)
        yield s, eps


def test_open_loop_eval_refuses_bad_ids_before_any_launch(store, monkeypatch):
    from diamond_amd import native as nv
    from diamond_amd.openloop import open_loop_eval

    s, _ = store
    log = []
    launches = []
    monkeypatch.setattr(nv, "_lib", SimpleNamespace(dmd_segment_gather=lambda *a: launches.append(a) or 0, dmd_openloop_step=lambda *a: launches.append(a) or 0,
                                                    dmd_last_error=lambda: b""))
    for bad, why in (([(0, 0, 9)], "steps"),                  # stop - start != T + horizon
                     ([(0, 0, 10), (1, 0, 9)], "steps"),
                     ([(0, 14, 24)], "outside"),              # start >= len
                     ([(0, -10, 0)], "outside"),              # stop <= 0
                     ([(3, 0, 10)], "episode 3"), ([(-1, 0, 10)], "episode -1"), ([], "no segment")):
        with pytest.raises(ValueError, match=why):
            open_loop_eval(_StubSampler(log), _StubRewEnd(log), s, bad, 6)
    with pytest.raises(ValueError, match="horizon"):
        open_loop_eval(_StubSampler(log), _StubRewEnd(log), s, [(0, 0, 4)], 0)
    assert launches == [] and log == []


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_open_loop_eval_call_order_ring_arithmetic_and_summary(store, teacher_forced):
    """horizon = T + 2: the ring wraps.  Against a shadow that ROLLS its context like the reference's env, built from the
    episodes themselves: what every sampler / reward-end call saw, the report's fields, the final rings, and summary()."""
    from diamond_amd.openloop import open_loop_eval
    from diamond_amd.replay import SegmentId

    s, eps = store
    horizon = T + 2
    ids = [SegmentId(0, 2, 2 + T + horizon), (1, -2, -2 + T + horizon), (2, 0, T + horizon), (1, 3, 3 + T + horizon)]
    b = len(ids)
    log = []
    sampler, rem = _StubSampler(log), _StubRewEnd(log)
    with engine_on_interpreter():
        rep = open_loop_eval(sampler, rem, s, ids, horizon, teacher_forced=teacher_forced, return_levels=True)

    def recorded(e, k):  # (levels or None, act, rew, end, transition into it valid) of step k of episode e
        ep, n = eps[e], eps[e].obs.shape[0]
        if 0 <= k < n:
            return ep.obs[k], int(ep.act[k])
        if k == n and "final_observation" in ep.info and int(ep.end[-1]):
            return ep.info["final_observation"], 0
        return None, 0

    deq = lambda u8: u8.float().div(255).mul(2).sub(1)
    sh_obs = torch.zeros((b, T) + FRAME)
    sh_act = torch.zeros(b, T, dtype=torch.int64)
    for i, (e, start) in enumerate([(0, 2), (1, -2), (2, 0), (1, 3)]):
        for k in range(T):
            if start + k >= 0:
                sh_obs[i, k], sh_act[i, k] = deq(eps[e].obs[start + k]), eps[e].act[start + k]
    assert [x[0] for x in log] == ["rew_end"] + ["sample", "rew_end"] * horizon
    burn = log[0]
    assert torch.equal(burn[1], sh_obs[:, :-1]) and torch.equal(burn[2], sh_act[:, :-1]) and torch.equal(burn[3], sh_obs[:, 1:]) and burn[4] is None
    want = {k: torch.zeros(b, horizon, dtype=torch.int64) for k in ("sq_err", "abs_err", "max_err", "pixels_off", "fv", "tv", "end")}
    want["rew"] = torch.zeros(b, horizon)
    for i in range(horizon):
        kind, oh, ah, c_obs, c_act = log[1 + 2 * i]
        assert (kind, oh, ah) == ("sample", i % T, i % T)
        order = [(oh + k) % T for k in range(T)]
        assert torch.equal(c_obs[:, order], sh_obs) and torch.equal(c_act[:, order], sh_act), f"step {i}: the ring is not the rolled context"
        _, r_obs, r_act, r_next, r_state = log[2 + 2 * i]
        pred = deq(sampler.preds[i])
        assert torch.equal(r_obs[:, 0], sh_obs[:, -1]) and torch.equal(r_act[:, 0], sh_act[:, -1]) and torch.equal(r_next, pred)
        assert float(r_state[0][0, 0, 0]) == i + 1  # the state the previous call returned
        nxt, nact = pred.clone(), torch.zeros(b, dtype=torch.int64)
        for j, (e, start) in enumerate([(0, 2), (1, -2), (2, 0), (1, 3)]):
            k = start + T + i
            lv, nact[j] = recorded(e, k)
            if lv is not None:
                d = (sampler.preds[i][j] - lv.long()).abs()
                want["sq_err"][j, i], want["abs_err"][j, i], want["max_err"][j, i], want["pixels_off"][j, i] = (d * d).sum(), d.sum(), d.max(), (d != 0).sum()
                want["fv"][j, i] = 1
                if teacher_forced:
                    nxt[j] = deq(lv)
            if 0 <= k - 1 < eps[e].obs.shape[0]:
                want["tv"][j, i], want["rew"][j, i], want["end"][j, i] = 1, eps[e].rew[k - 1], eps[e].end[k - 1]
        sh_obs, sh_act = sh_obs.roll(-1, dims=1), sh_act.roll(-1, dims=1)
        sh_obs[:, -1], sh_act[:, -1] = nxt, nact
        assert torch.equal(rep.levels[:, i], sampler.preds[i].to(torch.uint8))
    for k in ("sq_err", "abs_err", "max_err", "pixels_off"):
        assert getattr(rep, k).dtype == torch.int64 and torch.equal(getattr(rep, k), want[k]), k
    assert rep.frame_valid.dtype == torch.bool and torch.equal(rep.frame_valid, want["fv"].bool()) and torch.equal(rep.transition_valid, want["tv"].bool())
    assert torch.equal(rep.rew_true, want["rew"]) and rep.end_true.dtype == torch.uint8 and torch.equal(rep.end_true.long(), want["end"])
    assert want["fv"].sum(1).tolist() == [6, 6, 4, 3] and want["tv"].sum(1).tolist() == [6, 6, 5, 3]  # (what the ids were chosen for)
    assert rep.head == horizon % T and rep.per_frame == 48
    order = [(rep.head + k) % T for k in range(T)]
    assert torch.equal(rep.ctx_obs[:, order], sh_obs) and torch.equal(rep.ctx_act[:, order], sh_act)
    assert rep.logits_rew.shape == (b, horizon, 3) and rep.logits_end.shape == (b, horizon, 2)
    for i in range(horizon):
        g = torch.Generator().manual_seed(101 + i)
        assert torch.equal(rep.logits_rew[:, i], torch.randn(b, 1, 3, generator=g)[:, 0]) and torch.equal(rep.logits_end[:, i], torch.randn(b, 1, 2, generator=g)[:, 0])

    # summary() against numpy, from the report's tensors
    sm = rep.summary()
    fv, tv = rep.frame_valid.numpy(), rep.transition_valid.numpy()
    assert sm["horizon"] == horizon and sm["valid_frames"] == fv.sum(0).tolist() and sm["valid_transitions"] == tv.sum(0).tolist()
    for i in range(horizon):
        n = fv[:, i].sum() * 48
        mse = float(rep.sq_err.numpy()[fv[:, i], i].sum()) / n * (2.0 / 255.0) ** 2
        assert sm["mse"][i] == pytest.approx(mse, rel=1e-12) and sm["psnr"][i] == pytest.approx(10 * math.log10(4.0 / mse), rel=1e-12)
        assert sm["pixels_off"][i] == pytest.approx(float(rep.pixels_off.numpy()[fv[:, i], i].sum()) / n, rel=1e-12)
        assert sm["max_err"][i] == int(rep.max_err.numpy()[fv[:, i], i].max())
        cm_r, cm_e = np.zeros((3, 3), np.int64), np.zeros((2, 2), np.int64)
        for j in np.flatnonzero(tv[:, i]):
            cm_r[int(np.sign(rep.rew_true[j, i].item())) + 1, int(rep.logits_rew[j, i].argmax())] += 1
            cm_e[int(rep.end_true[j, i]), int(rep.logits_end[j, i].argmax())] += 1
        assert sm["confusion_matrix_rew"][i] == cm_r.tolist() and sm["confusion_matrix_end"][i] == cm_e.tolist()
    assert all(isinstance(x, float) for x in sm["mse"] + sm["psnr"] + sm["pixels_off"])


def test_open_loop_eval_accepts_a_context_that_is_padding_only(store):
    """start <= -T: the whole context lies in front of the episode (zeros, action 0), the first evaluated steps too."""
    from diamond_amd.openloop import open_loop_eval

    s, eps = store
    log = []
    sampler = _StubSampler(log)
    with engine_on_interpreter():
        rep = open_loop_eval(sampler, _StubRewEnd(log), s, [(0, -6, 4)], 6)
    first = log[1]
    assert first[0] == "sample" and not first[3].any() and not first[4].any()
    assert rep.frame_valid.tolist() == [[False, False, True, True, True, True]]
    assert rep.transition_valid.tolist() == [[False, False, False, True, True, True]]
    assert rep.ctx_act[0, [(rep.head + k) % T for k in range(T)]].tolist() == eps[0].act[:4].tolist()


def test_summary_of_exact_and_empty_steps():
    """A step whose valid frames all match has mse 0 and psnr inf; a step without valid samples has nan."""
    from diamond_amd.openloop import OpenLoopReport

    z = torch.zeros(2, 2, dtype=torch.int64)
    fv = torch.tensor([[True, False], [True, False]])
    rep = OpenLoopReport(sq_err=z, abs_err=z, max_err=z, pixels_off=z, frame_valid=fv, transition_valid=fv, logits_rew=torch.zeros(2, 2, 3),
                         logits_end=torch.zeros(2, 2, 2), rew_true=torch.zeros(2, 2), end_true=torch.zeros(2, 2, dtype=torch.uint8), levels=None,
                         ctx_obs=torch.zeros(2, 4, 1), ctx_act=torch.zeros(2, 4, dtype=torch.int64), head=0, per_frame=12)
    sm = rep.summary()
    assert sm["mse"][0] == 0.0 and sm["psnr"][0] == float("inf") and math.isnan(sm["mse"][1]) and math.isnan(sm["psnr"][1])
    assert sm["confusion_matrix_rew"] == [[[0, 0, 0], [2, 0, 0], [0, 0, 0]], [[0] * 3] * 3] and sm["confusion_matrix_end"][1] == [[0, 0], [0, 0]]
