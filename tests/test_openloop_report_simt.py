"""The open-loop report's motion fields and the whole-store pass (diamond_amd/openloop.py) without a GPU: the host layer on the
interpreter's host harness with stub sampler / reward-end objects, as tests/test_openloop_simt.py does.

The two stubs that give the new numbers their meaning: one that returns the RECORDING (every skill and change score exactly 1, the
split errors exactly 0) and one that hands its NEWEST CONTEXT FRAME back (it changes nothing, and teacher forced its error IS the
error of copying the previous recorded frame: skill exactly 0)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.simt.host_harness import engine_on_interpreter

FRAME = (1, 12, 12)  # (the smallest frames dmd_frame_ssim takes)
PF = 144
T, HORIZON = 4, 6    # the ring wraps
TODAY = {"horizon", "valid_frames", "valid_transitions", "mse", "psnr", "pixels_off", "max_err", "confusion_matrix_rew", "confusion_matrix_end"}
MOTION_KEYS = {"valid_prev", "valid_anchor", "skill_prev", "skill_anchor", "change_recall", "change_precision", "share_changed", "mse_changed",
               "mse_static", "exact_changed"}


def _moved(rng, frame):
    out = frame.copy().reshape(-1)
    at = rng.choice(PF, 3, replace=False)
    out[at] = (out[at].astype(np.int64) + rng.randint(1, 256, 3)) % 256
    return out.reshape(frame.shape)


def _ep(n, seed, end_last=False, final=False):
    """A static background, three values changing per step, every fourth step a repeat of the one before it."""
    rng = np.random.RandomState(seed)
    obs = np.empty((n,) + FRAME, np.uint8)
    obs[0] = rng.randint(0, 256, FRAME)
    for k in range(1, n):
        obs[k] = obs[k - 1] if k % 4 == 3 else _moved(rng, obs[k - 1])
    end = torch.zeros(n, dtype=torch.uint8)
    end[-1] = int(end_last)
    info = {"final_observation": torch.from_numpy(_moved(rng, obs[-1]))} if final else {}
    return SimpleNamespace(obs=torch.from_numpy(obs), act=torch.from_numpy(rng.randint(0, 4, n)), rew=torch.from_numpy(rng.randint(-1, 2, n)).float(),
                           end=end, trunc=torch.zeros(n, dtype=torch.uint8), info=info)


LENGTHS = (14, 9, 3, 6)  # (one episode shorter than T + 1; none a multiple of the stride plus T)


@pytest.fixture()
def store():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        eps = [_ep(14, 1), _ep(9, 2, end_last=True, final=True), _ep(3, 3), _ep(6, 4, end_last=True)]
        for e in eps:
            s.add_episode(e)
        yield s, eps


# left padded from s = 0 on | into the final observation and past it | past an end without a final frame | inside | context of padding only
IDS = [(0, -4, -4 + T + HORIZON), (1, 1, 1 + T + HORIZON), (3, 0, T + HORIZON), (0, 3, 3 + T + HORIZON), (0, -5, -5 + T + HORIZON)]


def _deq(u8):
    return u8.float().div(255).mul(2).sub(1)


def _recorded(eps, e, k):
    ep, n = eps[e], eps[e].obs.shape[0]
    if 0 <= k < n:
        return ep.obs[k]
    if k == n and "final_observation" in ep.info and int(ep.end[-1]):
        return ep.info["final_observation"]
    return None


class _Sampler:
    """kind "recording": the recorded frame of the step (a frame of level 7 where there is none); "newest": the ring's newest
    frame; "rolled": the ring's newest frame shifted by one column -- each row a function of that row's context alone."""

    def __init__(self, kind, eps=None, ids=None):
        self.denoiser = SimpleNamespace(cfg=SimpleNamespace(inner_model=SimpleNamespace(num_steps_conditioning=T)))
        self.kind, self.eps, self.ids, self.calls = kind, eps, ids, 0

    def sample_ring(self, ctx_obs, ctx_act, obs_head, act_head):
        i, self.calls = self.calls, self.calls + 1
        newest = ctx_obs[:, (obs_head - 1) % T]
        if self.kind == "newest":
            return newest.clone(), []
        if self.kind == "rolled":
            return newest.roll(1, dims=-1).contiguous(), []
        out = torch.full((len(self.ids),) + FRAME, 7, dtype=torch.uint8)
        for j, (e, start, _) in enumerate(self.ids):
            lv = _recorded(self.eps, e, start + T + i)
            if lv is not None:
                out[j] = lv
        return _deq(out), []


class _RewEnd:
    """logits that are a function of each row's own inputs (exact integer arithmetic): equal for a window in any batch"""

    def predict_rew_end(self, obs, act, next_obs, hx_cx=None):
        b, t = act.shape
        lv = ((next_obs.reshape(b, -1)[:, :1] + 1) / 2 * 255).round().long()  # (b, 1): one level of the predicted frame
        key = (act + lv) % 6
        l_rew = torch.stack([(key % 3 == c).float() for c in range(3)], dim=-1)
        l_end = torch.stack([(key % 2 == c).float() for c in range(2)], dim=-1)
        return l_rew, l_end, (torch.zeros(1, b, 2), torch.zeros(1, b, 2))


def _same(a, b):
    """equal numbers, lists or dicts of them; nan equals nan"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_a_sampler_that_returns_the_recording_scores_exactly_one(store):
    from diamond_amd.openloop import open_loop_eval

    s, eps = store
    with engine_on_interpreter():
        rep = open_loop_eval(_Sampler("recording", eps, IDS), _RewEnd(), s, IDS, HORIZON, teacher_forced=True, motion=True)
    fv = rep.frame_valid
    assert not bool((rep.sq_err * fv).any()) and fv.sum(1).tolist() == [6, 5, 2, 6, 5]
    # what was asked of the ids: a first frame without a predecessor, contexts of padding only, frames behind an end
    assert rep.prev_valid.sum(1).tolist() == [5, 5, 2, 6, 4] and rep.anchor_valid.sum(1).tolist() == [0, 5, 2, 6, 0]
    assert rep.frame_valid[0].tolist() == [True] * 6 and rep.prev_valid[0].tolist() == [False] + [True] * 5
    assert rep.frame_valid[4].tolist() == [False] + [True] * 5 and rep.prev_valid[4].tolist() == [False] * 2 + [True] * 4
    # the prediction changed exactly the values the recording changed, to the recorded level
    assert torch.equal(rep.changed_both, rep.changed_true) and torch.equal(rep.exact_changed, rep.changed_true)
    assert torch.equal(rep.changed_pred * rep.prev_valid, rep.changed_true) and not bool(rep.sq_err_changed.any())
    sm = rep.summary()
    assert sm["valid_frames"] == fv.sum(0).tolist() and all(n > 0 for n in sm["valid_frames"])
    for i in range(HORIZON):
        for k in ("skill_prev", "skill_anchor", "change_recall", "change_precision", "exact_changed"):
            assert sm[k][i] == 1.0, (k, i, sm[k])
        assert sm["mse_changed"][i] == 0.0 and sm["mse_static"][i] == 0.0
        assert 0.0 < sm["share_changed"][i] <= 3.0 / PF


@pytest.mark.parametrize("teacher_forced", [True, False])
def test_a_sampler_that_copies_its_newest_frame_has_no_skill(store, teacher_forced):
    from diamond_amd.openloop import open_loop_eval

    s, eps = store
    with engine_on_interpreter():
        rep = open_loop_eval(_Sampler("newest"), _RewEnd(), s, IDS, HORIZON, teacher_forced=teacher_forced, motion=True)
    assert not bool(rep.changed_pred.any()) and not bool(rep.changed_both.any()) and not bool(rep.exact_changed.any())
    sm = rep.summary()
    pv = rep.prev_valid
    if teacher_forced:  # its newest frame IS the previous recorded frame
        assert torch.equal(rep.sq_err * pv, rep.sq_copy_prev) and bool(rep.sq_copy_prev.any())
        assert torch.equal(rep.sq_err_changed, rep.sq_copy_prev)  # all of its error sits on the values that changed
        for i in range(HORIZON):
            assert int(pv[:, i].sum()) > 0 and sm["skill_prev"][i] == 0.0 and sm["mse_static"][i] == 0.0 and sm["change_recall"][i] == 0.0
    else:  # free running it freezes the context: step 0 as above, then the anchor's error wherever the anchor was recorded
        assert sm["skill_prev"][0] == 0.0
        av = rep.anchor_valid
        assert torch.equal(rep.sq_err * av, rep.sq_copy_anchor) and int(av.sum()) == 13
        assert all(x == 0.0 for x in sm["skill_anchor"])
    assert all(math.isnan(x) for x in sm["change_precision"])  # 0 / 0: it predicted no change at all


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_summary_matches_numpy_and_motion_false_is_todays_report(store, teacher_forced):
    from diamond_amd.openloop import MOTION_FIELDS, open_loop_eval

    s, eps = store
    with engine_on_interpreter():
        rep = open_loop_eval(_Sampler("rolled"), _RewEnd(), s, IDS, HORIZON, teacher_forced=teacher_forced, motion=True, return_levels=True)
        off = open_loop_eval(_Sampler("rolled"), _RewEnd(), s, IDS, HORIZON, teacher_forced=teacher_forced, return_levels=True)
    sm, sm_off = rep.summary(), off.summary()
    assert set(sm_off) == TODAY and set(sm) == TODAY | MOTION_KEYS
    assert _same({k: sm[k] for k in TODAY}, sm_off)
    for k in MOTION_FIELDS:
        assert getattr(off, k) is None and getattr(rep, k).shape == (len(IDS), HORIZON), k
    for k in ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true", "end_true", "levels",
              "ctx_act"):
        assert torch.equal(getattr(rep, k), getattr(off, k)), k
    assert torch.equal(rep.ctx_obs.view(torch.int32), off.ctx_obs.view(torch.int32)) and rep.head == off.head

    # the fields against the episodes: y, r, a from the recording, q from the levels, m from the previous levels / the recording
    n = {k: getattr(rep, k).numpy() for k in MOTION_FIELDS + ("sq_err", "frame_valid")}
    for j, (e, start, _) in enumerate(IDS):
        for i in range(HORIZON):
            k = start + T + i
            y, r, a = _recorded(eps, e, k), (_recorded(eps, e, k - 1) if k >= 1 else None), (_recorded(eps, e, start + T - 1) if start + T - 1 < LENGTHS[e] else None)
            assert n["frame_valid"][j, i] == (y is not None) and n["prev_valid"][j, i] == (y is not None and r is not None)
            assert n["anchor_valid"][j, i] == (y is not None and a is not None)
            if y is None:
                continue
            y, q = y.long(), rep.levels[j, i].long()
            prev_rec = _recorded(eps, e, k - 1)
            if i == 0 or (teacher_forced and prev_rec is not None):
                m = prev_rec.long() if prev_rec is not None else torch.full(FRAME, 128)  # (padding is 0.0: level 128 by round-half-even)
            else:
                m = rep.levels[j, i - 1].long()
            assert n["changed_pred"][j, i] == int((q != m).sum()), (j, i)
            if r is not None:
                ch = y != r.long()
                want = (int(((y - r.long()) ** 2).sum()), int(ch.sum()), int((ch & (q != m)).sum()), int(((q - y) ** 2)[ch].sum()), int((ch & (q == y)).sum()))
                got = tuple(int(n[f][j, i]) for f in ("sq_copy_prev", "changed_true", "changed_both", "sq_err_changed", "exact_changed"))
                assert got == want, (j, i)
            if a is not None:
                assert n["sq_copy_anchor"][j, i] == int(((y - a.long()) ** 2).sum())

    # summary() against numpy, from the report's tensors
    unit = (2.0 / 255.0) ** 2

    def div(x, y):
        return float("nan") if y == 0 else float(x) / float(y)

    for i in range(HORIZON):
        pv, av = n["prev_valid"][:, i], n["anchor_valid"][:, i]
        tot = {f: int(n[f][pv, i].sum()) for f in ("sq_err", "sq_copy_prev", "changed_true", "changed_pred", "changed_both", "sq_err_changed", "exact_changed")}
        want = {"skill_prev": 1.0 - div(tot["sq_err"], tot["sq_copy_prev"]),
                "skill_anchor": 1.0 - div(int(n["sq_err"][av, i].sum()), int(n["sq_copy_anchor"][av, i].sum())),
                "change_recall": div(tot["changed_both"], tot["changed_true"]), "change_precision": div(tot["changed_both"], tot["changed_pred"]),
                "share_changed": div(tot["changed_true"], int(pv.sum()) * PF), "mse_changed": div(tot["sq_err_changed"], tot["changed_true"]) * unit,
                "mse_static": div(tot["sq_err"] - tot["sq_err_changed"], int(pv.sum()) * PF - tot["changed_true"]) * unit,
                "exact_changed": div(tot["exact_changed"], tot["changed_true"])}
        assert sm["valid_prev"][i] == int(pv.sum()) and sm["valid_anchor"][i] == int(av.sum())
        for k, v in want.items():
            assert isinstance(sm[k][i], float) and sm[k][i] == pytest.approx(v, rel=1e-12, nan_ok=True), (k, i)


def test_store_windows_matches_a_hand_written_list(store):
    from diamond_amd.openloop import store_windows
    from diamond_amd.replay import SegmentId

    s, _ = store  # lengths 14, 9, 3, 6; T = 4: a window starts at a while a + 4 < length
    got = list(store_windows(s, 3, t=T))
    assert got == [SegmentId(0, 0, 7), SegmentId(0, 3, 10), SegmentId(0, 6, 13), SegmentId(0, 9, 16), SegmentId(1, 0, 7), SegmentId(1, 3, 10),
                   SegmentId(3, 0, 7)]
    assert [(w.episode_id, w.start, w.stop) for w in store_windows(s, 5, 4, t=T)] == [(0, 0, 9), (0, 4, 13), (0, 8, 17), (1, 0, 9), (1, 4, 13), (3, 0, 9)]
    assert [(w.episode_id, w.start) for w in store_windows(s, 2, 1, t=2)] == [(0, a) for a in range(12)] + [(1, a) for a in range(7)] + [(2, 0)] + [
        (3, a) for a in range(4)]
    for bad in (dict(horizon=0), dict(horizon=3, stride=0)):
        with pytest.raises(ValueError):
            list(store_windows(s, t=T, **bad))


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_evaluate_store_in_batches_of_three_equals_one_evaluation_of_all_windows(store, teacher_forced):
    from diamond_amd.openloop import OpenLoopTotals, evaluate_store, open_loop_eval, step_sums, store_windows

    s, _ = store
    ids = list(store_windows(s, 3, t=T))
    assert len(ids) == 7
    with engine_on_interpreter():
        totals = evaluate_store(_Sampler("rolled"), _RewEnd(), s, 3, batch_size=3, teacher_forced=teacher_forced, ssim=True)
        whole = open_loop_eval(_Sampler("rolled"), _RewEnd(), s, ids, 3, teacher_forced=teacher_forced, ssim=True, motion=True)
        capped = evaluate_store(_Sampler("rolled"), _RewEnd(), s, 3, batch_size=3, teacher_forced=teacher_forced, max_windows=4, motion=False)
        first4 = open_loop_eval(_Sampler("rolled"), _RewEnd(), s, ids[:4], 3, teacher_forced=teacher_forced)
    assert isinstance(totals, OpenLoopTotals) and totals.windows == 7
    want = step_sums(whole)
    assert set(totals.sums) == set(want) and {"prev_valid", "anchor_valid", "confusion_matrix_rew", "confusion_matrix_end", "sq_err_changed"} <= set(want)
    for k, v in want.items():
        if k not in ("ssim", "ssim_cs"):
            assert v.dtype == torch.int64 and totals.sums[k].dtype == torch.int64 and torch.equal(totals.sums[k], v), k
    sm, sm_whole = totals.summary(), whole.summary()
    assert set(sm) == set(sm_whole) | {"windows"} and sm["windows"] == 7
    assert _same({k: v for k, v in sm.items() if k not in ("ssim", "ssim_cs", "windows")}, {k: v for k, v in sm_whole.items() if k not in ("ssim", "ssim_cs")})
    assert sum(sm["valid_frames"]) > 14 and all(0.0 < x for x in sm["mse"])
    for k in ("ssim", "ssim_cs"):  # fp64 sums of n values in [-1, 1] in another order: the means agree within n * 2^-52
        for i in range(3):
            assert abs(sm[k][i] - sm_whole[k][i]) <= sm["valid_frames"][i] * 2.0 ** -52, (k, i)
            assert -1.0 <= sm[k][i] <= 1.0
    # max_windows, and motion=False through the totals: today's keys
    sm4 = capped.summary()
    assert set(sm4) == TODAY | {"windows"} and sm4["windows"] == 4 and _same({k: sm4[k] for k in TODAY}, first4.summary())
