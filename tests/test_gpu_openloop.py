"""Open-loop evaluation on the GPU (`-m gpu`): dmd_openloop_step exactly equal to the numpy restatement of
tests/openloop_cases.py (the interpreter's cases, and one production-shaped launch checked for every sample), `open_loop_eval` bit
for bit against the same loop written with the entry points that existed before it (gather, sample_ring, predict_rew_end,
dmd_quantize_u8, torch integer ops, explicit ring writes), two sanity properties, and no host synchronisation in the loop."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import openloop_cases as OC
from tests.conftest import WEIGHT_SEED
from tests.replay_cases import assert_same

DEV = "cuda"
pytestmark = pytest.mark.gpu
BAND = 128  # elements of guard on both sides of every output


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _banded(init: np.ndarray):
    """`init` on the device in the middle of a poisoned buffer: (the view the kernel gets, the guard elements)."""
    t = torch.from_numpy(np.ascontiguousarray(init))
    whole = torch.empty(t.numel() + 2 * BAND, dtype=t.dtype, device=DEV)
    whole.view(torch.uint8).fill_(0xA5)
    view = whole[BAND:BAND + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view, whole


def _poison(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xFF if np.issubdtype(np.dtype(dtype), np.floating) else 0x5A
    return a


def _run(case, teacher_forced, with_levels=True):
    from diamond_amd import native as nv

    arena, pred = case["arena"], case["pred"]
    b, pf = pred.shape
    ins = {k: torch.from_numpy(arena[k]).to(DEV) for k in ("frames", "act", "rew", "end", "finals")}
    seg, pred_d = torch.from_numpy(case["seg"]).to(DEV), torch.from_numpy(pred).to(DEV)
    outs = {"ctx_obs": _banded(case["ctx_obs"]), "ctx_act": _banded(case["ctx_act"]), "metrics": _banded(_poison((b, 4), np.int64)),
            "rew": _banded(_poison(b, np.float32)), "end": _banded(_poison(b, np.uint8)), "valid": _banded(_poison((b, 2), np.uint8))}
    if with_levels:
        outs["levels"] = _banded(_poison((b, pf), np.uint8))
    p = nv.OpenLoopParams()
    p.B, p.T, p.per_frame, p.step, p.head, p.teacher_forced = b, case["T"], pf, case["step"], case["head"], int(teacher_forced)
    p.frames, p.act, p.rew, p.end = (nv.ptr(ins[k]) for k in ("frames", "act", "rew", "end"))
    p.finals = nv.ptr(ins["finals"]) if len(arena["finals"]) else None
    p.seg, p.pred = nv.ptr(seg), nv.fptr(pred_d)
    for field, k in (("ctx_obs", "ctx_obs"), ("ctx_act", "ctx_act"), ("metrics", "metrics"), ("out_rew", "rew"), ("out_end", "end"),
                     ("out_valid", "valid"), ("out_levels", "levels")):
        setattr(p, field, nv.ptr(outs[k][0]) if k in outs else None)
    nv.check(nv.lib().dmd_openloop_step(ctypes.byref(p), nv.stream()), "dmd_openloop_step")
    for k, (view, whole) in outs.items():
        guard = torch.cat([whole[:BAND], whole[BAND + view.numel():]]).view(torch.uint8)
        assert bool((guard == 0xA5).all()), f"{k}: bytes around the output were written"
    return {k: v[0].cpu().numpy() for k, v in outs.items()}


def _check(case, teacher_forced, what, **kw):
    got = _run(case, teacher_forced, **kw)
    assert_same(got, OC.restate(case, teacher_forced), tuple(k for k in OC.OUTPUTS if k in got), what)  # (every ring slot: the others unchanged)
    return got


@pytest.mark.parametrize("teacher_forced", [False, True])
@pytest.mark.parametrize("head", [0, 3])
@pytest.mark.parametrize("per_frame", OC.PER_FRAMES)
def test_openloop_step_matches_the_restatement(per_frame, head, teacher_forced):
    """The cases of tests/test_openloop_simt.py on the device: every kind of sample in one descriptor and in batches of 3."""
    case = OC.make_case(per_frame, head, seed=per_frame + head)
    got = _check(case, teacher_forced, "all kinds")
    for i, kind in enumerate(OC.KINDS):
        assert tuple(got["valid"][i]) == OC.EXPECTED_VALID[kind], kind
    assert got["metrics"][OC.KINDS.index("equal to its target")].tolist() == [0, 0, 0, 0]
    for rows in ([0, 1, 2], [2, 3, 4], [5, 7, 8]):
        _check(OC.rows_of(case, rows), teacher_forced, f"rows {rows}", with_levels=rows[0] != 2)
    for step in (0, 3):
        _check(OC.make_case(per_frame, head, step=step, seed=step), teacher_forced, f"step {step}", with_levels=False)


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_openloop_step_production_shape_every_sample(teacher_forced):
    """B = 11 frames of 3 x 64 x 64 (three passes of the 16-level lanes per workgroup), every sample against the restatement."""
    pf = 3 * 64 * 64
    case = OC.make_case(pf, 2, seed=11)
    rows = list(range(9)) + [0, 2]
    case = OC.rows_of(case, rows)
    case["seg"][9, 1], case["seg"][10, 1] = 5, 0  # two more starts: inside episode 0, and episode 1's last recorded step
    case["pred"] = OC.predictions(case["arena"], case["seg"], OC.T, case["step"], seed=3, equal_rows=(8,))
    assert len(case["seg"]) == 11
    got = _check(case, teacher_forced, "B = 11, 3 x 64 x 64")
    assert got["valid"][:, 0].tolist() == [1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1] and got["metrics"][8].tolist() == [0, 0, 0, 0]
    assert (got["metrics"][[0, 1, 2, 6, 9, 10], 3] > pf // 4).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the composition
# ---------------------------------------------------------------------------------------------------------------------------
FRAME = (3, 64, 64)
T, HORIZON = 4, 3
# (length, ends, final observation): two end with a final observation, one ends without
EPISODES = ((9, False, False), (10, True, True), (11, False, False), (12, True, True), (9, True, False), (12, False, False))
#  left-padded | runs into its final observation | inside | the same | ends without a final frame | runs past an episode that did not end
IDS = [(0, -2, 5), (1, 4, 11), (2, 2, 9), (3, 6, 13), (4, 3, 10), (5, 8, 15)]


@pytest.fixture(scope="module")
def agent():
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    a = D.Agent(D.default_agent_config())
    fill_module_(a, WEIGHT_SEED)
    return a.to(DEV).eval()


@pytest.fixture(scope="module")
def store():
    from diamond_amd.replay import DeviceReplay

    s = DeviceReplay(DEV)
    g = torch.Generator().manual_seed(23)
    for n, ends, final in EPISODES:
        end = torch.zeros(n, dtype=torch.int64)
        end[-1] = int(ends)
        info = {"final_observation": torch.randint(0, 256, FRAME, generator=g, dtype=torch.uint8)} if final else {}
        s.add_episode(SimpleNamespace(obs=torch.randint(0, 256, (n,) + FRAME, generator=g, dtype=torch.uint8), act=torch.randint(0, 4, (n,), generator=g),
                                      rew=torch.randint(-1, 2, (n,), generator=g).float(), end=end, trunc=torch.zeros(n, dtype=torch.int64), info=info))
    return s


def _sampler(agent, seed=5):
    """A 3-step sampler whose draws come from a seeded CPU generator: the same sequence for every arm that makes the same calls."""
    import diamond_amd as D

    sampler = D.DiffusionSampler(agent.denoiser, D.DiffusionSamplerConfig(num_steps_denoising=3))
    g = torch.Generator().manual_seed(seed)
    sampler.noise_fn = lambda shape, dev: torch.randn(shape, generator=g).to(dev)
    return sampler


_FIELDS = ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true", "end_true", "levels")


@pytest.fixture(scope="module")
def reports(agent, store):
    """Both modes once, shared by the tests below: (open_loop_eval's report, the reference loop's results)."""
    from diamond_amd.openloop import open_loop_eval

    res = {}
    for tf in (False, True):
        rep = open_loop_eval(_sampler(agent), agent.rew_end_model, store, IDS, HORIZON, teacher_forced=tf, return_levels=True)
        res[tf] = (rep, OC.reference_loop(_sampler(agent), agent.rew_end_model, store, IDS, T, HORIZON, tf))
    return res


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_open_loop_eval_is_the_reference_loop_bit_for_bit(reports, store, teacher_forced):
    rep, (want, ctx_obs, ctx_act, head) = reports[teacher_forced]
    for k in _FIELDS:
        got = getattr(rep, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (k, got.dtype, want[k].dtype, got.shape, want[k].shape)
        assert torch.equal(got.contiguous().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k
    assert rep.head == head and torch.equal(rep.ctx_act, ctx_act)
    assert torch.equal(rep.ctx_obs.view(torch.int32), ctx_obs.view(torch.int32))
    # the ids were chosen for these: left padding, two final observations, an end without one, past an episode that did not end
    assert rep.frame_valid.tolist() == [[True] * 3, [True] * 3, [True] * 3, [True] * 3, [True, True, False], [False] * 3]
    assert rep.transition_valid.tolist() == [[True] * 3] * 5 + [[True, False, False]]
    assert rep.end_true.dtype == store.flag_dtype == torch.int64 and rep.end_true[:, 2].tolist() == [0, 1, 0, 1, 1, 0]
    sm = rep.summary()
    assert sm["valid_frames"] == [5, 5, 4] and all(0 < m < 4 for m in sm["mse"]) and all(0 < x <= 1 for x in sm["pixels_off"])
    assert [sum(map(sum, c)) for c in sm["confusion_matrix_rew"]] == [6, 5, 5] == [sum(map(sum, c)) for c in sm["confusion_matrix_end"]]


def test_free_running_and_teacher_forced_differ_from_the_second_step_on(reports):
    """The first prediction comes from the same context in both modes; from the second step on the contexts differ wherever the
    first prediction was not the recording."""
    free, forced = reports[False][0], reports[True][0]
    assert torch.equal(free.levels[:, 0], forced.levels[:, 0]) and torch.equal(free.sq_err[:, 0], forced.sq_err[:, 0])
    moved = free.frame_valid[:, 0] & (free.sq_err[:, 0] > 0)
    assert int(moved.sum()) == 5
    for i in (1, 2):
        differs = (free.levels[:, i] != forced.levels[:, i]).flatten(1).any(1)
        assert bool(differs[moved].all()), i
        assert not torch.equal(free.sq_err[moved, i], forced.sq_err[moved, i]), i
    assert not torch.equal(free.ctx_obs, forced.ctx_obs)


class _RecordingSampler:
    """A `sampler` that reproduces the recording (shifted by `shift` levels): the dequantised target of every evaluated step."""

    def __init__(self, agent, store, ids, shift):
        self.denoiser = agent.denoiser
        whole = OC.device_levels(store.gather(ids, put_back_final=True, info=False).obs).long()
        whole = torch.where(whole + shift > 255, whole - shift, whole + shift)
        self.frames = whole.float().div(255).mul(2).sub(1)
        self.calls = 0

    def sample_ring(self, ctx_obs, ctx_act, obs_head, act_head):
        self.calls += 1
        return self.frames[:, T + self.calls - 1].contiguous(), []


@pytest.mark.parametrize("teacher_forced", [False, True])
def test_a_sampler_that_reproduces_the_recording_has_no_error_and_one_level_off_has_one(agent, store, teacher_forced):
    from diamond_amd.openloop import open_loop_eval

    pf = int(np.prod(FRAME))
    exact = open_loop_eval(_RecordingSampler(agent, store, IDS, 0), agent.rew_end_model, store, IDS, HORIZON, teacher_forced=teacher_forced)
    fv = exact.frame_valid
    assert int(fv.sum()) == 14 and exact.levels is None
    for k in ("sq_err", "abs_err", "max_err", "pixels_off"):
        assert not bool(getattr(exact, k).any()), k
    sm = exact.summary()
    assert sm["mse"] == [0.0] * 3 and sm["psnr"] == [float("inf")] * 3 and sm["pixels_off"] == [0.0] * 3
    one = open_loop_eval(_RecordingSampler(agent, store, IDS, 1), agent.rew_end_model, store, IDS, HORIZON, teacher_forced=teacher_forced)
    for k in ("sq_err", "abs_err", "pixels_off"):
        assert torch.equal(getattr(one, k), fv.long() * pf), k
    assert torch.equal(one.max_err, fv.long())
    assert one.summary()["mse"] == pytest.approx([(2.0 / 255.0) ** 2] * 3, rel=1e-12)


def test_open_loop_eval_does_not_synchronise_inside_its_loop(agent, store, reports):
    """From the first sampler call to the return -- the loop and the report's assembly -- under
    torch.cuda.set_sync_debug_mode("error"); reading the numbers afterwards is the one wait.  (`reports` ran the same shapes
    before: the weights are packed.)"""
    from diamond_amd.openloop import open_loop_eval

    sampler = _sampler(agent)
    noise = [torch.randn(len(IDS), *FRAME, device=DEV) for _ in range(HORIZON)]
    sampler.noise_fn = lambda shape, dev: noise.pop()  # (no host-to-device copy in the guarded region)
    plain = sampler.sample_ring
    calls = []

    def guarded(*a, **k):
        if not calls:
            torch.cuda.set_sync_debug_mode("error")
        calls.append(1)
        return plain(*a, **k)

    sampler.sample_ring = guarded
    try:
        rep = open_loop_eval(sampler, agent.rew_end_model, store, IDS, HORIZON, teacher_forced=True, return_levels=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == HORIZON and noise == []
    assert rep.summary()["valid_frames"] == [5, 5, 4]
