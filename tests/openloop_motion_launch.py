"""TEST INFRASTRUCTURE: the launcher of dmd_openloop_motion against a runner of tests/abi.py (interpreter or device), on a case of
tests/motion_cases.py.  Inputs go through run.put (fenced on the interpreter); the two outputs sit in the middle of poisoned
buffers whose bands are checked after the launch, and every input is read back and compared bit for bit with what went in."""
import ctypes as C

import numpy as np

from diamond_amd import native as nv
from tests import abi
from tests.replay_cases import bits

BAND = 64  # bytes of guard on both sides of an output (a multiple of 16: the output stays aligned)


def _banded(run, shape, dtype):
    """(handle of the poisoned buffer, address of the output inside it, its bytes)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    body = -(-nbytes // 16) * 16
    h = run.put(np.full(body + 2 * BAND, 0xA5, np.uint8))
    assert run.ptr(h) % 16 == 0
    return h, run.ptr(h) + BAND, nbytes


def _unband(run, h, nbytes, shape, dtype, what):
    raw = run.get(h)
    assert (raw[:BAND] == 0xA5).all() and (raw[BAND + nbytes:] == 0xA5).all(), f"{what}: bytes around the output were written"
    return raw[BAND:BAND + nbytes].copy().view(dtype).reshape(shape)


def openloop_motion(run, case, misalign_pred=False, status=False, **override):
    """dmd_openloop_motion on `case` -> {"out": (B, 8) int64, "valid": (B, 3) uint8}.  misalign_pred: `pred` sits 4 bytes past a
    16-byte boundary.  override: parameter fields set last (None: a NULL pointer) -- the refused-argument tests."""
    arena, seg, pred, ring = case["arena"], case["seg"], case["pred"], case["ctx_obs"]
    b, pf = pred.shape
    ins = {"frames": arena["frames"], "end": arena["end"], "seg": seg, "ctx_obs": ring}
    if len(arena["finals"]):
        ins["finals"] = arena["finals"]
    hs = {k: run.put(v) for k, v in ins.items()}
    if misalign_pred:
        hs["pred"], pred_at = abi._aligned(run, pred, 1)
        assert pred_at % 16 == 4
    else:
        hs["pred"] = run.put(pred)
        pred_at = run.ptr(hs["pred"])
    before = {k: bits(run.get(h)).copy() for k, h in hs.items()}
    (ho, out_at, out_n), (hv, valid_at, valid_n) = _banded(run, (b, 8), np.int64), _banded(run, (b, 3), np.uint8)
    p = nv.MotionParams()
    p.B, p.T, p.per_frame, p.step, p.head = b, case["T"], pf, case["step"], case["head"]
    p.frames, p.end, p.finals, p.seg = run.ptr(hs["frames"]), run.ptr(hs["end"]), run.ptr(hs.get("finals")), run.ptr(hs["seg"])
    p.pred, p.ctx_obs, p.out, p.out_valid = pred_at, run.ptr(hs["ctx_obs"]), out_at, valid_at
    for k, v in override.items():
        setattr(p, k, v)
    rc = run.lib().dmd_openloop_motion(C.byref(p), run.stream())

    def outs():
        got = {"out": _unband(run, ho, out_n, (b, 8), np.int64, "out"), "valid": _unband(run, hv, valid_n, (b, 3), np.uint8, "out_valid")}
        for k, h in hs.items():
            assert np.array_equal(bits(run.get(h)), before[k]), f"{k}: an input changed"
        return got

    return abi._finish(run, rc, "dmd_openloop_motion", status, outs)
