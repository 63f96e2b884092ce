"""dmd_openloop_motion on the SIMT interpreter and on the device (tests/abi.py's runner pair), exactly equal to the numpy
restatement of tests/motion_cases.py: every kind of descriptor row, the three lane widths, both ends of the ring, T = 1, sub-batches,
finals = NULL, a misaligned prediction, sums beyond 2^32, the refused arguments, and on the device one production-shaped launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import abi
from tests import motion_cases as MC
from tests.openloop_motion_launch import openloop_motion
from tests.replay_cases import assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(run, case, what, **kw):
    got = openloop_motion(run, case, **kw)
    assert_same(got, MC.restate(case), ("out", "valid"), what)
    return got


@pytest.mark.parametrize("run,per_frame,t,head", abi.arms(abi.Simt, abi.Gpu, [(pf, t, h) for pf in MC.PER_FRAMES for t, h in ((4, 0), (4, 3), (1, 0))]))
def test_motion_matches_the_restatement(run, per_frame, t, head):
    """Every kind of sample in one descriptor and in batches of 3, for the three lane widths, head 0 and T - 1, and T = 1 (the
    newest slot is the head's); every other ring slot holds NaN."""
    case = MC.make_case(per_frame, head, t=t, seed=per_frame + head)
    got = _check(run, case, "all kinds")
    want = MC.restate(case)
    for i, kind in enumerate(MC.KINDS):
        assert tuple(got["valid"][i]) == MC.EXPECTED_VALID[kind], kind
        if not got["valid"][i, 0]:
            assert not got["out"][i].any(), kind
    k = MC.KINDS.index
    assert (got["out"][k("inside"), :4] > 0).all()
    assert got["out"][k("prediction equal to the recording"), 5] == 0
    assert got["out"][k("prediction equal to the recording"), 6] == got["out"][k("prediction equal to the recording"), 2] > 0
    assert got["out"][k("prediction equal to m"), 3] == 0 == got["out"][k("prediction equal to m"), 4]
    assert got["out"][k("an unchanged step"), [0, 2, 4, 5, 6]].tolist() == [0] * 5 and got["out"][k("an unchanged step"), 3] > 0
    assert got["out"][k("s = 0"), 3] > 0 and got["out"][k("s = 0"), [0, 1, 2, 4, 5, 6]].tolist() == [0] * 6
    assert got["out"][k("context of padding only"), 1] == 0 < got["out"][k("context of padding only"), 0]
    assert (want["out"][:, 7] == 0).all()
    for rows in ([0, 1, 2], [2, 3, 4], [5, 7, 8], [9, 10, 11], [12, 13, 14]):
        _check(run, MC.rows_of(case, rows), f"rows {rows}")


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_motion_without_finals_and_with_a_misaligned_prediction(run):
    """finals = NULL: final_row is never followed, the two final-observation rows become invalid.  per_frame = 48 with a prediction
    4 bytes off a 16-byte boundary: the one-level path must be taken."""
    case = MC.make_case(48, 2, seed=5)
    got = _check(run, MC.without_finals(case), "finals = NULL")
    for kind in ("final observation", "final observation after the last step"):
        assert tuple(got["valid"][MC.KINDS.index(kind)]) == (0, 0, 0)
    _check(run, case, "misaligned pred", misalign_pred=True)


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_motion_sums_are_64_bit(run):
    """B = 1, 66,064 values, y = 255 against r = a = q = 0 everywhere: 66,064 * 255^2 = 4,295,811,600 > 2^32 in entries 0, 1, 5."""
    pf = 66064
    arena = {"frames": np.stack([np.zeros(pf, np.uint8), np.full(pf, 255, np.uint8)]), "end": np.zeros(2, np.uint8), "finals": np.zeros((0, pf), np.uint8)}
    case = {"arena": arena, "seg": np.array([[0, 0, 2, -1]], np.int64), "T": 1, "head": 0, "step": 0, "pred": np.full((1, pf), -1.0, np.float32),
            "ctx_obs": np.full((1, 1, pf), -1.0, np.float32)}
    got = _check(run, case, "64-bit sums")
    assert got["out"][0].tolist() == [4295811600, 4295811600, pf, 0, 0, 4295811600, 0, 0] and got["valid"][0].tolist() == [1, 1, 1]


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_motion_refuses_bad_arguments(run):
    case = MC.make_case(20, 0)
    rc, _, _ = openloop_motion(run, case, status=True)
    assert rc == 0
    rc, _, got = openloop_motion(run, case, status=True, B=0)
    assert rc == 0 and (got["out"].view(np.uint8) == 0xA5).all() and (got["valid"] == 0xA5).all()  # nothing launched
    for bad in (dict(frames=None), dict(end=None), dict(seg=None), dict(pred=None), dict(ctx_obs=None), dict(out=None), dict(out_valid=None),
                dict(T=0), dict(per_frame=0), dict(step=-1), dict(head=-1), dict(head=MC.OC.T), dict(B=-1)):
        rc, msg, _ = openloop_motion(run, case, status=True, **bad)
        assert rc != 0 and "openloop_motion" in msg, bad
    assert run.lib().dmd_openloop_motion(None, run.stream()) != 0


@pytest.mark.gpu
def test_motion_production_shape_every_sample():
    """B = 256 frames of 3 x 64 x 64 (three passes of the 16-level lanes per workgroup): the descriptor's kinds in turn, each row's
    prediction and ring rotated by its own offset, every sample against the restatement."""
    pf, b = 3 * 64 * 64, 256
    base = MC.make_case(pf, 2, seed=11)
    case = MC.rows_of(base, [i % len(MC.KINDS) for i in range(b)])
    newest = (case["head"] + case["T"] - 1) % case["T"]
    for i in range(len(MC.KINDS), b):
        case["pred"][i] = np.roll(case["pred"][i], i)
        case["ctx_obs"][i, newest] = np.roll(case["ctx_obs"][i, newest], 2 * i)
    got = _check(abi.Gpu, case, "B = 256, 3 x 64 x 64")
    valid = np.array([MC.EXPECTED_VALID[MC.KINDS[i % len(MC.KINDS)]] for i in range(b)], np.uint8)
    assert np.array_equal(got["valid"], valid)
    assert len({tuple(r) for r in got["out"][valid[:, 0] == 1].tolist()}) > 100  # (the rotations made the rows differ)


def test_motion_params_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of the ctypes mirror against the C struct (compiled with gcc from include/diamond_hip.h)."""
    from diamond_amd import native as nv

    fields = [f for f, _ in nv.MotionParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_openloop_motion_params));' + "".join(f'printf("%zu ", offsetof(dmd_openloop_motion_params, {f}));' for f in fields)
    src = tmp_path / "s.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    mine = [ctypes.sizeof(nv.MotionParams)] + [getattr(nv.MotionParams, f).offset for f in fields]
    assert got == mine, list(zip(["sizeof"] + fields, got, mine))
    assert "dmd_openloop_motion" in nv.EXPORTS and "dmd_openloop_motion" in nv.LAUNCHERS
