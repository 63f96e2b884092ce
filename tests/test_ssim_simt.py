"""Per-frame SSIM (dmd_frame_ssim, diamond_amd/metrics.py, open_loop_eval(ssim=True)) without a GPU:

  * the kernel's own source on the SIMT interpreter (tests/simt): the operands between inaccessible pages, `out` and the workspace
    inside guard bands, within 1e-10 of the 121-tap numpy restatement of tests/ssim_cases.py (the bound is derived there);
  * the host layer on the interpreter's host harness with a stub sampler / reward-end model: the report's ssim fields against the
    restatement applied to `report.levels` and the recorded frames, `summary()` against numpy, everything else untouched.
"""
import ctypes
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import ssim_cases as SC
from tests.simt import loader as S
from tests.simt.fence import fenced as G
from tests.simt.host_harness import engine_on_interpreter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 64  # bytes of guard on both sides of `out` and the workspace
WORST = {"err": 0.0}  # the largest difference from the restatement seen in this process (printed by the last kernel test)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _banded(n_doubles: int):
    """`n_doubles` poisoned (all-ones: NaN) doubles in the middle of a guarded buffer: (view, whole buffer as bytes, offset)."""
    raw = np.full(n_doubles * 8 + 2 * BAND + 64, 0xA5, np.uint8)
    off = BAND + (-(raw.ctypes.data + BAND) % 64)
    view = raw[off:off + n_doubles * 8].view(np.float64)
    view.view(np.uint8)[...] = 0xFF
    return view, raw, off


def _params(shape, **kw):
    from diamond_amd import native as nv

    p = nv.SsimParams()
    p.N, p.C, p.H, p.W = shape
    p.win[:] = list(SC.window())
    p.c1, p.c2 = SC.C1, SC.C2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _set(p, which, arr, keep, tight):
    f = G(arr, tight=tight)
    keep.append(f)
    setattr(p, f"{which}_{'f32' if arr.dtype == np.float32 else 'u8'}", f.ctypes.data)


def _launch(p, shape):
    """Run `p` with a guarded out / workspace; returns out (N, 2)."""
    L = S.lib()
    n = shape[0]
    want_ws = int(L.dmd_ssim_workspace_doubles(*shape))
    assert want_ws == 2 * n * shape[1] * math.ceil((shape[2] - 10) / SC.S) * math.ceil((shape[3] - 10) / SC.S)
    out, ws = _banded(2 * n), _banded(want_ws)
    p.out, p.workspace = out[0].ctypes.data, ws[0].ctypes.data
    S.check(L.dmd_frame_ssim(ctypes.byref(p), None), "dmd_frame_ssim")
    for name, (view, raw, off) in (("out", out), ("workspace", ws)):
        assert (raw[:off] == 0xA5).all() and (raw[off + view.nbytes:] == 0xA5).all(), f"{name}: bytes around it were written"
    return out[0].reshape(n, 2).copy()


def _direct(a, b, tight="end"):
    keep = []
    p = _params(a.shape)
    _set(p, "a", a, keep, tight)
    _set(p, "b", b, keep, tight)
    return _launch(p, a.shape)


def _arena(case, step=SC.STEP, finals=True, tight="end"):
    arena = case["arena"]
    keep = [G(arena[k], tight=tight) for k in ("frames", "end", "finals")] + [G(case["seg"], tight=tight)]
    shape = case["a"].shape
    p = _params(shape, frames=keep[0].ctypes.data, end=keep[1].ctypes.data, finals=keep[2].ctypes.data if finals else None,
                seg=keep[3].ctypes.data, T=SC.T, step=step)
    _set(p, "a", case["a"], keep, tight)
    return _launch(p, shape)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("kind", SC.PAIRS)
@pytest.mark.parametrize("shape", SC.SMALL_SHAPES + SC.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frame_ssim_matches_the_restatement(shape, kind):
    """One position; unaligned rows (per_frame 156); several frames and channels; S - 1, S and S + 1 positions per axis -- for
    every operand pair, the operands fenced at their ends (random pairs also at their starts)."""
    a, b = SC.pair(kind, shape, seed=sum(shape))
    WORST["err"] = max(WORST["err"], SC.check_pair(kind, _direct(a, b), a, b))
    if kind == "random":
        got = _direct(a, b, tight="start")
        assert np.array_equal(_bits(got), _bits(_direct(a, b)))


def test_frame_ssim_several_tiles_and_channels():
    """(2, 3, S + 11, 2 S + 12): 2 x 3 tiles per channel, partial tiles on both axes, six partials per channel and frame."""
    shape = (2, 3, SC.S + 11, 2 * SC.S + 12)
    for kind in ("random", "plus minus 2", "identical"):
        a, b = SC.pair(kind, shape, seed=3)
        WORST["err"] = max(WORST["err"], SC.check_pair(kind, _direct(a, b), a, b))
    print(f"largest difference from the restatement on the interpreter: {WORST['err']:.3e}")


def test_fp32_operand_is_taken_at_the_level_quantize_u8_stores():
    """Values off the grid and outside [-1, 1] as fp32 operand a, b, or both: bitwise the result of the uint8 operand that holds
    dmd_quantize_u8's levels of them."""
    L = S.lib()
    shape = (2, 3, 13, 12)
    va, vb = SC.off_grid(shape, 1), SC.off_grid(shape, 2)
    q = {}
    for k, v in (("a", va), ("b", vb)):
        lv, flag = G(np.zeros(shape, np.uint8)), G(np.zeros(1, np.int32))
        S.check(L.dmd_quantize_u8(G(v).ctypes.data, lv.ctypes.data, flag.ctypes.data, v.size, None), "dmd_quantize_u8")
        q[k] = np.array(lv)
        assert flag[0] == 1 and (q[k] == 0).any() and (q[k] == 255).any()
    want = _direct(q["a"], q["b"])
    assert np.abs(want - SC.restate(q["a"], q["b"])).max() <= SC.TOL
    for a, b in ((va, q["b"]), (q["a"], vb), (va, vb)):
        assert np.array_equal(_bits(_direct(a, b)), _bits(want))


@pytest.mark.parametrize("frame", [(1, 11, 11), (3, 12, 13)])
def test_arena_mode_is_direct_mode_on_the_gathered_targets(frame):
    """Every kind of descriptor row: bitwise the direct result on the gathered targets where there is one, NaN where not, at
    several steps and with finals = NULL.  The arena is fenced: nothing outside it is read."""
    case = SC.arena_case(frame, seed=frame[1])
    for step, finals in ((SC.STEP, True), (SC.STEP, False), (0, True), (3, True), (200, True)):
        got = _arena(case, step=step, finals=finals)
        valid, targets = SC.arena_targets(case, step=step, finals=finals)
        if step == SC.STEP:
            expect = [v and (finals or k != "final observation") for _, _, k, v in SC.ARENA_SAMPLES]
            assert valid.tolist() == expect
        if step == 200:
            assert not valid.any()
        assert np.isnan(got[~valid]).all() and not np.isnan(got[valid]).any(), (step, finals, got)
        if valid.any():
            want = _direct(case["a"][valid], targets)
            assert np.array_equal(_bits(got[valid]), _bits(want)), (step, finals)
            assert np.abs(want - SC.restate(case["a"][valid], targets)).max() <= SC.TOL
    got = _arena(case, tight="start")
    assert np.array_equal(_bits(got), _bits(_arena(case)))


def test_frame_ssim_refuses_bad_arguments():
    L = S.lib()
    shape = (2, 1, 12, 13)
    a, b = SC.pair("random", shape)
    case = SC.arena_case(shape[1:])
    keep = {"a_u8": G(a), "b_u8": G(b), "a_f32": G(SC.dequant(a)), "b_f32": G(SC.dequant(b)), "frames": G(case["arena"]["frames"]),
            "end": G(case["arena"]["end"]), "finals": G(case["arena"]["finals"]), "seg": G(case["seg"][:2]), "out": G(np.zeros((2, 2))),
            "workspace": G(np.zeros(int(L.dmd_ssim_workspace_doubles(*shape))))}
    at = lambda *names: {k: keep[k].ctypes.data for k in names}
    direct = at("a_u8", "b_u8", "out", "workspace")
    arena = dict(at("a_f32", "frames", "end", "finals", "seg", "out", "workspace"), T=SC.T, step=1)

    def rc(base, shape=shape, **kw):
        return L.dmd_frame_ssim(ctypes.byref(_params(shape, **{**base, **kw})), None)

    assert rc(direct) == 0 and rc(arena) == 0 and rc(arena, finals=None) == 0
    bad = [(direct, dict(H=10)), (direct, dict(W=10)), (direct, dict(H=0)), (direct, dict(C=0)), (direct, dict(N=-1)),
           (direct, at("a_f32")), (direct, dict(a_u8=None)), (direct, at("b_f32")), (direct, dict(b_u8=None)),      # both / neither pointer
           (direct, at("frames")), (direct, at("seg")), (direct, at("end")), (direct, at("finals")),                 # direct b + an arena field
           (arena, at("b_u8")), (arena, at("b_f32")), (arena, dict(frames=None)), (arena, dict(end=None)), (arena, dict(seg=None)),
           (direct, dict(out=None)), (direct, dict(workspace=None)), (arena, dict(out=None)), (arena, dict(workspace=None)),
           (arena, dict(step=-1)), (direct, dict(step=-1)), (arena, dict(T=-1))]
    for base, kw in bad:
        assert rc(base, **kw) != 0, kw
        assert b"frame_ssim" in L.dmd_last_error(), kw
    assert L.dmd_frame_ssim(None, None) != 0
    assert L.dmd_ssim_workspace_doubles(1, 1, 10, 11) == 0 and L.dmd_ssim_workspace_doubles(1, 0, 11, 11) == 0


def test_frame_ssim_of_no_frames_launches_nothing():
    """N == 0: status 0, and neither `out` nor the workspace is touched (both are inaccessible here)."""
    L = S.lib()
    empty = G(np.zeros(0, np.uint8))  # sits against a PROT_NONE page
    p = _params((0, 3, 16, 16), a_u8=empty.ctypes.data, b_u8=empty.ctypes.data, out=empty.ctypes.data, workspace=empty.ctypes.data)
    assert L.dmd_frame_ssim(ctypes.byref(p), None) == 0
    assert L.dmd_ssim_workspace_doubles(0, 3, 16, 16) == 0


def test_frame_ssim_is_the_same_under_every_lane_schedule(monkeypatch):
    """SIMT_SCHEDULE 0, 1, 2 (ascending, descending, odd waves first): the same bits -- the LDS stages are properly fenced by
    barriers and the summation order does not depend on who runs first."""
    shape = (2, 2, SC.S + 11, SC.S + 9)
    a, b = SC.pair("plus minus 2", shape, seed=9)
    case = SC.arena_case((3, 12, 13), seed=4)
    res = []
    for schedule in (0, 1, 2):
        monkeypatch.setenv("SIMT_SCHEDULE", str(schedule))
        res.append((_direct(a, b), _arena(case)))
    for d, ar in res[1:]:
        assert np.array_equal(_bits(d), _bits(res[0][0])) and np.array_equal(_bits(ar), _bits(res[0][1]))
    assert np.abs(res[0][0] - SC.restate(a, b)).max() <= SC.TOL


def test_ssim_params_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of the ctypes mirror against the C struct (compiled with gcc from include/diamond_hip.h)."""
    from diamond_amd import native as nv

    fields = [f for f, _ in nv.SsimParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_ssim_params));' + "".join(f'printf("%zu ", offsetof(dmd_ssim_params, {f}));' for f in fields)
    body += 'printf("%d ", DMD_SSIM_TAPS);'
    src = tmp_path / "s.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    mine = [ctypes.sizeof(nv.SsimParams)] + [getattr(nv.SsimParams, f).offset for f in fields] + [nv.SSIM_TAPS]
    assert got == mine, list(zip(["sizeof"] + fields + ["taps"], got, mine))
    assert "dmd_frame_ssim" in nv.EXPORTS and "dmd_ssim_workspace_doubles" in nv.EXPORTS
    assert "dmd_frame_ssim" in nv.LAUNCHERS and "dmd_ssim_workspace_doubles" not in nv.LAUNCHERS


# ---------------------------------------------------------------------------------------------------------------------------
# the host layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_frame_ssim_host_function_on_the_interpreter():
    """metrics.frame_ssim: the window and constants it forms, both dtypes, (N, 2) fp64, and its refusals (before any launch)."""
    from diamond_amd import native as nv
    from diamond_amd.metrics import frame_ssim, ssim_constants

    win, c1, c2 = ssim_constants()
    assert np.abs(np.array(win) - SC.window()).max() < 1e-16 and c1 == SC.C1 and c2 == SC.C2 and abs(sum(win) - 1.0) < 1e-15
    shape = (2, 3, 12, 13)
    a, b = SC.pair("plus minus 2", shape, seed=1)
    with engine_on_interpreter():
        got = frame_ssim(torch.from_numpy(a), torch.from_numpy(b))
        assert got.dtype == torch.float64 and got.shape == (2, 2)
        assert np.abs(got.numpy() - SC.restate(a, b)).max() <= SC.TOL
        mixed = frame_ssim(torch.from_numpy(SC.dequant(a)), torch.from_numpy(b))
        assert torch.equal(mixed.view(torch.int64), got.view(torch.int64))
        other = frame_ssim(torch.from_numpy(a), torch.from_numpy(b), sigma=1.0, k1=0.02, k2=0.05)
        g = np.exp(-((np.arange(11.0) - 5) ** 2) / 2.0)
        assert np.abs(other.numpy() - SC.restate(a, b, g / g.sum(), (0.02 * 255) ** 2, (0.05 * 255) ** 2)).max() <= SC.TOL
        assert frame_ssim(torch.zeros(0, 3, 12, 13, dtype=torch.uint8), torch.zeros(0, 3, 12, 13)).shape == (0, 2)
        launches = []
        saved = nv._lib
        nv._lib = SimpleNamespace(dmd_frame_ssim=lambda *x: launches.append(x) or 0, dmd_ssim_workspace_doubles=lambda *x: 1, dmd_last_error=lambda: b"")
        try:
            ta, tb = torch.from_numpy(a), torch.from_numpy(b)
            for x, y in ((ta[0], tb[0]), (ta, tb[:1]), (ta, tb[:, :, :, :12]), (ta.double(), tb.double()), (ta.long(), tb), (ta[:, :, :10], tb[:, :, :10]),
                         (ta[:, :, :, :10], tb[:, :, :, :10]), (a, b)):
                with pytest.raises(ValueError, match="frame_ssim"):
                    frame_ssim(x, y)
            with pytest.raises(ValueError, match="sigma"):
                frame_ssim(ta, tb, sigma=0.0)
        finally:
            nv._lib = saved
        assert launches == []


FRAME = (3, 12, 13)
T, HORIZON = 4, 6


def _ep(n, seed, end_last=False, final=False):
    g = torch.Generator().manual_seed(seed)
    end = torch.zeros(n, dtype=torch.uint8)
    end[-1] = int(end_last)
    info = {"final_observation": torch.randint(0, 256, FRAME, generator=g, dtype=torch.uint8)} if final else {}
    return SimpleNamespace(obs=torch.randint(0, 256, (n,) + FRAME, generator=g, dtype=torch.uint8), act=torch.randint(0, 4, (n,), generator=g),
                           rew=torch.randint(-1, 2, (n,), generator=g).float(), end=end, trunc=torch.zeros(n, dtype=torch.uint8), info=info)


class _StubSampler:
    """`sample_ring` returns the ring's newest frame moved by up to two levels (on the grid): a plausible prediction."""

    def __init__(self):
        self.denoiser = SimpleNamespace(cfg=SimpleNamespace(inner_model=SimpleNamespace(num_steps_conditioning=T)))
        self.calls = 0

    def sample_ring(self, ctx_obs, ctx_act, obs_head, act_head):
        g = torch.Generator().manual_seed(self.calls)
        self.calls += 1
        newest = ctx_obs[:, (obs_head - 1) % T]
        lv = (newest.add(1).div(2).mul(255).round() + torch.randint(-2, 3, newest.shape, generator=g)).clamp(0, 255)
        return lv.div(255).mul(2).sub(1), []


class _StubRewEnd:
    def __init__(self):
        self.calls = 0

    def predict_rew_end(self, obs, act, next_obs, hx_cx=None):
        b, t = act.shape
        g = torch.Generator().manual_seed(100 + self.calls)
        self.calls += 1
        return torch.randn(b, t, 3, generator=g), torch.randn(b, t, 2, generator=g), (torch.zeros(1, b, 2), torch.zeros(1, b, 2))


class _LaunchLog:
    """native.PROFILER stand-in: the names of the C-ABI launches, in order."""

    def __init__(self):
        self.names = []

    def annotate(self, key, flops, nbytes):
        pass

    def call(self, name, fn, args):
        self.names.append(name)
        return fn(*args)


IDS = [(0, 2, 2 + T + HORIZON), (1, -2, -2 + T + HORIZON), (2, 0, T + HORIZON), (1, 3, 3 + T + HORIZON)]


@pytest.fixture(scope="module")
def runs():
    """open_loop_eval on the stubs three times: without the keyword, ssim=False, ssim=True: (report, launch log, summary) each."""
    from diamond_amd import native as nv
    from diamond_amd.openloop import open_loop_eval
    from diamond_amd.replay import DeviceReplay

    out = {}
    with engine_on_interpreter():
        store = DeviceReplay("cpu")
        eps = [_ep(14, 1), _ep(9, 2, end_last=True, final=True), _ep(8, 3, end_last=True)]
        for e in eps:
            store.add_episode(e)
        for name, kw in (("plain", {}), ("off", dict(ssim=False)), ("on", dict(ssim=True))):
            log = _LaunchLog()
            nv.PROFILER = log
            try:
                rep = open_loop_eval(_StubSampler(), _StubRewEnd(), store, IDS, HORIZON, return_levels=True, **kw)
            finally:
                nv.PROFILER = None
            out[name] = (rep, log.names, rep.summary())
    out["episodes"] = eps
    return out


def _recorded(eps, e, k):
    ep, n = eps[e], eps[e].obs.shape[0]
    if 0 <= k < n:
        return ep.obs[k].numpy()
    if k == n and "final_observation" in ep.info and int(ep.end[-1]):
        return ep.info["final_observation"].numpy()
    return None


def test_open_loop_eval_ssim_fields_match_the_restatement(runs):
    rep, _, sm = runs["on"]
    b = len(IDS)
    assert rep.ssim.dtype == rep.ssim_cs.dtype == torch.float64 and rep.ssim.shape == rep.ssim_cs.shape == (b, HORIZON)
    fv = rep.frame_valid.numpy()
    assert fv.sum(1).tolist() == [6, 6, 4, 3] and fv.sum() < fv.size
    got = np.stack([rep.ssim.numpy(), rep.ssim_cs.numpy()], axis=-1)
    assert np.isnan(got[~fv]).all() and not np.isnan(got[fv]).any()
    worst = 0.0
    for j, (e, start, _) in enumerate(IDS):
        for i in range(HORIZON):
            tgt = _recorded(runs["episodes"], e, start + T + i)
            assert (tgt is not None) == bool(fv[j, i])
            if tgt is not None:
                want = SC.restate(rep.levels[j, i].numpy()[None], tgt[None])[0]
                worst = max(worst, float(np.abs(got[j, i] - want).max()))
    assert worst <= SC.TOL, worst
    assert (np.abs(got[fv]) < 1.0).all()
    for k, col in (("ssim", 0), ("ssim_cs", 1)):
        assert len(sm[k]) == HORIZON and all(isinstance(x, float) for x in sm[k])
        for i in range(HORIZON):
            assert sm[k][i] == pytest.approx(float(got[fv[:, i], i, col].mean()), rel=1e-14)


def test_open_loop_eval_ssim_changes_nothing_else(runs):
    (plain, log_plain, sm_plain), (off, log_off, sm_off), (on, log_on, sm_on) = runs["plain"], runs["off"], runs["on"]
    assert log_off == log_plain and "dmd_frame_ssim" not in log_plain
    assert [n for n in log_on if n != "dmd_frame_ssim"] == log_plain and log_on.count("dmd_frame_ssim") == HORIZON
    step_at = [i for i, n in enumerate(log_on) if n == "dmd_openloop_step"]
    assert [log_on[i + 1] for i in step_at] == ["dmd_frame_ssim"] * HORIZON  # once per evaluated step
    assert off.ssim is None and off.ssim_cs is None and plain.ssim is None
    assert set(sm_off) == set(sm_plain) and "ssim" not in sm_off and "ssim_cs" not in sm_off
    assert set(sm_on) == set(sm_plain) | {"ssim", "ssim_cs"}
    for k in ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "rew_true", "end_true",
              "levels", "ctx_obs", "ctx_act"):
        for other in (off, on):
            x, y = getattr(other, k).contiguous(), getattr(plain, k).contiguous()
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
    assert on.head == plain.head and on.per_frame == plain.per_frame
    assert all(str(sm_on[k]) == str(sm_plain[k]) == str(sm_off[k]) for k in sm_plain)  # (nan != nan: compare the printed form)


def test_summary_ssim_of_a_step_without_valid_frames_is_nan():
    from diamond_amd.openloop import OpenLoopReport

    z = torch.zeros(2, 2, dtype=torch.int64)
    fv = torch.tensor([[True, False], [True, False]])
    nan = float("nan")
    rep = OpenLoopReport(sq_err=z, abs_err=z, max_err=z, pixels_off=z, frame_valid=fv, transition_valid=fv, logits_rew=torch.zeros(2, 2, 3),
                         logits_end=torch.zeros(2, 2, 2), rew_true=torch.zeros(2, 2), end_true=torch.zeros(2, 2, dtype=torch.uint8), levels=None,
                         ctx_obs=torch.zeros(2, 4, 1), ctx_act=torch.zeros(2, 4, dtype=torch.int64), head=0, per_frame=12,
                         ssim=torch.tensor([[0.25, nan], [0.75, nan]], dtype=torch.float64), ssim_cs=torch.tensor([[1.0, nan], [0.5, nan]], dtype=torch.float64))
    sm = rep.summary()
    assert sm["ssim"][0] == 0.5 and sm["ssim_cs"][0] == 0.75 and math.isnan(sm["ssim"][1]) and math.isnan(sm["ssim_cs"][1])
