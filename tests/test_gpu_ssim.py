"""Per-frame SSIM on the GPU (`-m gpu`): dmd_frame_ssim within 1e-10 of the 121-tap numpy restatement of tests/ssim_cases.py (the
interpreter's cases, then launches of 11 x 3 x 64 x 64, 2 x 3 x 256 x 256 and 2 x 3 x 68 x 76 with every sample checked), `out` and
the workspace inside poisoned guard bands, run-to-run bitwise equality, and `open_loop_eval(ssim=True)` on the real sampler and
reward / end model: its ssim fields bit for bit `frame_ssim` of the report's levels against the gathered targets, every other
field bit for bit the ssim=False report, no host synchronisation in the loop."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ssim_cases as SC
from tests.conftest import WEIGHT_SEED

DEV = "cuda"
pytestmark = pytest.mark.gpu
BAND = 128  # doubles of guard on both sides of `out` and the workspace
WORST = {"err": 0.0}


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _banded(n_doubles: int):
    whole = torch.empty(n_doubles + 2 * BAND, dtype=torch.float64, device=DEV)
    whole.view(torch.uint8).fill_(0xA5)
    view = whole[BAND:BAND + n_doubles]
    view.view(torch.uint8).fill_(0xFF)  # NaN: whatever the call does not write shows
    return view, whole


def _params(shape, **kw):
    from diamond_amd import native as nv

    p = nv.SsimParams()
    p.N, p.C, p.H, p.W = shape
    p.win[:] = list(SC.window())
    p.c1, p.c2 = SC.C1, SC.C2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _dev(arr, keep):
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)
    keep.append(t)
    return t.data_ptr() if t.numel() else None


def _launch(p, shape):
    from diamond_amd import native as nv

    n = shape[0]
    want_ws = int(nv.lib().dmd_ssim_workspace_doubles(*shape))
    assert want_ws == 2 * n * shape[1] * math.ceil((shape[2] - 10) / SC.S) * math.ceil((shape[3] - 10) / SC.S)
    out, ws = _banded(2 * n), _banded(want_ws)
    p.out, p.workspace = out[0].data_ptr(), ws[0].data_ptr()
    nv.check(nv.lib().dmd_frame_ssim(ctypes.byref(p), nv.stream()), "dmd_frame_ssim")
    for name, (view, whole) in (("out", out), ("workspace", ws)):
        guard = torch.cat([whole[:BAND], whole[BAND + view.numel():]]).view(torch.uint8)
        assert bool((guard == 0xA5).all()), f"{name}: bytes around it were written"
    return out[0].cpu().numpy().reshape(n, 2)


def _direct(a, b):
    keep = []
    p = _params(a.shape)
    for which, arr in (("a", a), ("b", b)):
        setattr(p, f"{which}_{'f32' if arr.dtype == np.float32 else 'u8'}", _dev(arr, keep))
    return _launch(p, a.shape)


def _arena(case, step=SC.STEP, finals=True):
    keep = []
    arena, shape = case["arena"], case["a"].shape
    p = _params(shape, frames=_dev(arena["frames"], keep), end=_dev(arena["end"], keep), finals=_dev(arena["finals"], keep) if finals else None,
                seg=_dev(case["seg"], keep), T=SC.T, step=step, a_u8=_dev(case["a"], keep))
    return _launch(p, shape)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("kind", SC.PAIRS)
def test_frame_ssim_matches_the_restatement(kind):
    """The interpreter's shapes on the device, for every operand pair."""
    for shape in SC.SMALL_SHAPES + SC.EDGE_SHAPES + ((2, 3, SC.S + 11, 2 * SC.S + 12),):
        a, b = SC.pair(kind, shape, seed=sum(shape))
        WORST["err"] = max(WORST["err"], SC.check_pair(kind, _direct(a, b), a, b))


@pytest.mark.parametrize("shape", [(11, 3, 64, 64), (2, 3, 256, 256), (2, 3, 68, 76)], ids=lambda s: "x".join(map(str, s)))
def test_frame_ssim_production_shapes_every_sample(shape):
    """Every sample against the restatement: the samples cycle through the operand pairs (random, a +- 2, identical, constants,
    0 / 255, 255 / 254), and a second run of the same launch gives the same bits."""
    ab = [SC.pair(SC.PAIRS[i % len(SC.PAIRS)], (1,) + shape[1:], seed=i) for i in range(shape[0])]
    a, b = np.concatenate([x for x, _ in ab]), np.concatenate([y for _, y in ab])
    got = _direct(a, b)
    err = float(np.abs(got - SC.restate(a, b)).max())
    WORST["err"] = max(WORST["err"], err)
    print(f"{shape}: largest difference from the restatement {err:.3e}; over this process so far {WORST['err']:.3e}")
    assert err <= SC.TOL, err
    for i in range(shape[0]):
        if SC.PAIRS[i % len(SC.PAIRS)] == "identical":
            assert got[i].tolist() == [1.0, 1.0]
    assert np.array_equal(_bits(_direct(a, b)), _bits(got))


def test_fp32_operand_is_taken_at_the_level_quantize_u8_stores():
    from tests.openloop_cases import device_levels

    shape = (2, 3, 13, 12)
    va, vb = SC.off_grid(shape, 1), SC.off_grid(shape, 2)
    qa, qb = (device_levels(torch.from_numpy(v).to(DEV)).cpu().numpy() for v in (va, vb))
    want = _direct(qa, qb)
    assert np.abs(want - SC.restate(qa, qb)).max() <= SC.TOL
    for a, b in ((va, qb), (qa, vb), (va, vb)):
        assert np.array_equal(_bits(_direct(a, b)), _bits(want))


@pytest.mark.parametrize("frame", [(1, 11, 11), (3, 12, 13), (3, 64, 64)])
def test_arena_mode_is_direct_mode_on_the_gathered_targets(frame):
    case = SC.arena_case(frame, seed=frame[1])
    for step, finals in ((SC.STEP, True), (SC.STEP, False), (0, True), (3, True), (200, True)):
        got = _arena(case, step=step, finals=finals)
        valid, targets = SC.arena_targets(case, step=step, finals=finals)
        assert np.isnan(got[~valid]).all() and not np.isnan(got[valid]).any(), (step, finals, got)
        if valid.any():
            assert np.array_equal(_bits(got[valid]), _bits(_direct(case["a"][valid], targets))), (step, finals)
            assert np.abs(got[valid] - SC.restate(case["a"][valid], targets)).max() <= SC.TOL


def test_frame_ssim_refusals_and_no_frames():
    from diamond_amd import native as nv

    L = nv.lib()
    keep = []
    a, b = SC.pair("random", (2, 1, 12, 13))
    base = dict(a_u8=_dev(a, keep), b_u8=_dev(b, keep), out=_dev(np.zeros((2, 2)), keep), workspace=_dev(np.zeros(4), keep))
    rc = lambda shape=(2, 1, 12, 13), **kw: L.dmd_frame_ssim(ctypes.byref(_params(shape, **{**base, **kw})), nv.stream())
    assert rc() == 0
    for kw in (dict(H=10), dict(W=10), dict(a_f32=base["a_u8"]), dict(a_u8=None), dict(b_f32=base["b_u8"]), dict(b_u8=None), dict(frames=base["a_u8"]),
               dict(seg=base["out"]), dict(out=None), dict(workspace=None), dict(step=-1)):
        assert rc(**kw) != 0 and b"frame_ssim" in L.dmd_last_error(), kw
    assert rc(shape=(0, 1, 12, 13), out=None, workspace=None, a_u8=None, a_f32=None) != 0  # (refusals come before N == 0)
    assert rc(shape=(0, 1, 12, 13)) == 0
    torch.cuda.synchronize()


def test_frame_ssim_host_function():
    from diamond_amd.metrics import frame_ssim

    shape = (3, 3, 24, 20)
    a, b = SC.pair("plus minus 2", shape, seed=1)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = frame_ssim(ta, tb)
    assert got.dtype == torch.float64 and got.shape == (3, 2) and got.is_cuda
    assert np.abs(got.cpu().numpy() - SC.restate(a, b)).max() <= SC.TOL
    assert torch.equal(frame_ssim(ta.float().div(255).mul(2).sub(1), tb).view(torch.int64), got.view(torch.int64))
    assert torch.equal(frame_ssim(ta[:, :, :, 2:18], tb[:, :, :, 2:18]).view(torch.int64), frame_ssim(ta[:, :, :, 2:18].contiguous(), tb[:, :, :, 2:18].contiguous()).view(torch.int64))
    assert frame_ssim(ta[:0], tb[:0]).shape == (0, 2)
    for x, y in ((ta[0], tb[0]), (ta, tb[:1]), (ta.double(), tb.double()), (ta[:, :, :10], tb[:, :, :10]), (ta, tb.cpu())):
        with pytest.raises(ValueError, match="frame_ssim"):
            frame_ssim(x, y)


# ---------------------------------------------------------------------------------------------------------------------------
# the composition
# ---------------------------------------------------------------------------------------------------------------------------
FRAME = (3, 64, 64)
T, HORIZON = 4, 3
# (length, ends, final observation)
EPISODES = ((9, False, False), (10, True, True), (11, False, False), (12, True, True), (9, True, False))
# left-padded | runs into its final observation | inside | the same | runs past its episode's end (no final frame)
IDS = [(0, -2, 5), (1, 4, 11), (2, 2, 9), (3, 6, 13), (4, 3, 10)]


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
    import diamond_amd as D

    sampler = D.DiffusionSampler(agent.denoiser, D.DiffusionSamplerConfig(num_steps_denoising=3))
    g = torch.Generator().manual_seed(seed)
    sampler.noise_fn = lambda shape, dev: torch.randn(shape, generator=g).to(dev)
    return sampler


@pytest.fixture(scope="module")
def reports(agent, store):
    from diamond_amd.openloop import open_loop_eval

    return {flag: open_loop_eval(_sampler(agent), agent.rew_end_model, store, IDS, HORIZON, return_levels=True, ssim=flag) for flag in (False, True)}


def test_open_loop_eval_ssim_is_frame_ssim_of_the_levels_against_the_targets(reports, store):
    from diamond_amd.metrics import frame_ssim

    rep = reports[True]
    assert rep.ssim.dtype == rep.ssim_cs.dtype == torch.float64 and rep.ssim.shape == rep.ssim_cs.shape == (len(IDS), HORIZON)
    fv = rep.frame_valid
    assert fv.tolist() == [[True] * 3] * 4 + [[True, True, False]]
    whole = store.gather(IDS, put_back_final=True, info=False).obs  # fp32, on the level grid
    for i in range(HORIZON):
        want = frame_ssim(rep.levels[:, i], whole[:, T + i])
        for got, col in ((rep.ssim, 0), (rep.ssim_cs, 1)):
            v = fv[:, i]
            assert torch.equal(got[v, i].view(torch.int64), want[v, col].view(torch.int64)), (i, col)
            assert bool(torch.isnan(got[~v, i]).all())
    vals = rep.ssim[fv]
    assert bool(((vals > -1) & (vals < 1)).all())
    sm = rep.summary()
    for k, t in (("ssim", rep.ssim), ("ssim_cs", rep.ssim_cs)):
        for i in range(HORIZON):
            assert sm[k][i] == pytest.approx(float(t[fv[:, i], i].cpu().numpy().mean()), rel=1e-14)


def test_open_loop_eval_ssim_changes_nothing_else(reports):
    off, on = reports[False], reports[True]
    assert off.ssim is None and off.ssim_cs is None and "ssim" not in off.summary()
    for k in ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true", "end_true",
              "levels", "ctx_obs", "ctx_act"):
        x, y = getattr(on, k).contiguous(), getattr(off, k).contiguous()
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
    assert on.head == off.head


def test_open_loop_eval_with_ssim_does_not_synchronise_inside_its_loop(agent, store, reports):
    """The method of tests/test_gpu_openloop.py: from the first sampler call to the return under
    torch.cuda.set_sync_debug_mode("error").  (`reports` ran the same shapes before: the weights are packed.)"""
    from diamond_amd.openloop import open_loop_eval

    sampler = _sampler(agent)
    noise = [torch.randn(len(IDS), *FRAME, device=DEV) for _ in range(HORIZON)]
    sampler.noise_fn = lambda shape, dev: noise.pop()
    plain = sampler.sample_ring
    calls = []

    def guarded(*a, **k):
        if not calls:
            torch.cuda.set_sync_debug_mode("error")
        calls.append(1)
        return plain(*a, **k)

    sampler.sample_ring = guarded
    try:
        rep = open_loop_eval(sampler, agent.rew_end_model, store, IDS, HORIZON, teacher_forced=True, ssim=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(calls) == HORIZON and noise == []
    assert len(rep.summary()["ssim"]) == HORIZON
