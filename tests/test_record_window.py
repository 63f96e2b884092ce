"""dmd_record_window (include/diamond_hip.h): a window of env steps written into the replay arena in one launch, on the SIMT
interpreter (every array between inaccessible pages) and on the device (`-m gpu`), bit for bit against the numpy restatement of
tests/record_cases.py -- every destination pre-filled with a poison pattern, so a row the launch must not touch shows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from diamond_amd import native as nv
from tests import abi
from tests import record_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ("obs", "act", "rew", "end", "trunc", "final_obs", "frames", "arena_act", "arena_rew", "arena_end", "arena_trunc", "finals",
            "runs", "off_grid")


def record_window(run, c, misalign=False, tight="end", status=False, **override):
    """The launcher: case `c` (tests/record_cases.py) through dmd_record_window -> the arena arrays and off_grid afterwards.
    misalign: the frame source sits 4 bytes past a 16-byte boundary; tight="start": the interpreter's arrays begin at their fence
    instead of ending at it; override: parameter fields set last (None: a NULL pointer)."""
    def put(a):
        if a is None or run.name != "simt" or tight == "end":
            return run.put(a)
        from tests.simt.fence import fenced
        return fenced(np.ascontiguousarray(a), tight="start")

    win = {k: put(c["window"][k]) for k in ("act", "rew", "end", "trunc")}
    win["final_obs"] = put(c["window"]["final_obs"] if c["K"] else None)
    obs = c["window"]["obs"]
    if misalign:
        obs = np.concatenate([np.full(1, np.nan, np.float32), obs.reshape(-1), np.full(-(obs.size + 1) % 4, np.nan, np.float32)])
    win["obs"] = put(obs)
    assert run.ptr(win["obs"]) % 16 == 0
    arena = {k: put(c[k]) for k in RC.ARENA}
    runs, off_grid = put(c["runs"]), put(np.zeros(1, np.int32))
    p = nv.RecordWindowParams()
    p.R, p.flag_size, p.per_frame = len(c["runs"]), c["window"]["end"].dtype.itemsize, c["per_frame"]
    p.total, p.steps, p.K, p.F, p.E = int(c["runs"][:, 2].sum()), c["steps"], c["K"], c["F"], c["E"]
    p.obs = run.ptr(win["obs"]) + (4 if misalign else 0)
    p.act, p.rew, p.end, p.trunc, p.final_obs = (run.ptr(win[k]) for k in ("act", "rew", "end", "trunc", "final_obs"))
    p.frames, p.arena_act, p.arena_rew, p.arena_end, p.arena_trunc, p.finals = (run.ptr(arena[k]) for k in RC.ARENA)
    p.runs, p.off_grid = run.ptr(runs), run.ptr(off_grid)
    for k, v in override.items():
        setattr(p, k, v)
    rc = run.lib().dmd_record_window(ctypes.byref(p), run.stream())

    def outs(keep=(win, runs)):  # (the sources stay alive until the result is back)
        got = {k: run.get(arena[k]) for k in RC.ARENA}
        got["off_grid"] = run.get(off_grid)
        return got

    return abi._finish(run, rc, "dmd_record_window", status, outs)


@pytest.mark.parametrize("run,per_frame,flag_size,r", abi.arms(abi.Simt, abi.Gpu, [(pf, fs, r) for pf in RC.PER_FRAMES for fs in (1, 8)
                                                                              for r in RC.RUN_COUNTS]))
def test_record_window_matches_the_restatement(run, per_frame, flag_size, r):
    """The three access paths x both flag sizes x R = 1 ... 37 runs of all three kinds in one launch: run lengths 1, 2 and T, an
    episode moved (kind 2) with an append of the same episode directly behind it, final observations between the steps."""
    c = RC.make_case(per_frame, np.uint8 if flag_size == 1 else np.int64, r)
    kinds = set(c["runs"][:, 0].tolist())
    assert kinds == ({0} if r == 1 else {0, 2} if r <= 3 else {0, 1, 2}) and (r < 5 or {1, 2, RC.T} <= set(c["runs"][:, 2].tolist()))
    want = RC.restate(c)
    assert want["off_grid"][0] == 0
    assert (want["frames"][0] == RC.POISON).all() and (want["frames"][-1] == RC.POISON).all()  # rows in front and behind stay untouched
    RC.assert_same(record_window(run, c), want, f"per_frame {per_frame}, flags of {flag_size} bytes, {r} runs")


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_record_window_source_off_the_16_byte_boundary_and_arrays_fenced_at_their_starts(run):
    """per_frame = 192 with the frame source 4 bytes past a 16-byte boundary: the entry must leave its 16-byte loads (on the
    interpreter a torn access faults on the fence).  Then the same case with every array BEGINNING at its fence."""
    c = RC.make_case(192, np.uint8, 37, seed=2)
    want = RC.restate(c)
    RC.assert_same(record_window(run, c, misalign=True), want, "misaligned obs")
    RC.assert_same(record_window(run, c, tight="start"), want, "fenced at the start")


@pytest.mark.parametrize("run,per_frame", abi.arms(abi.Simt, abi.Gpu, [256, 260, 257]))
def test_record_window_all_256_levels_at_every_position(run, per_frame):
    """Every level at every position of a frame, through the three paths (per_frame 256 / 260 / 257): the stored bytes are the
    levels the frames were made from, and nothing is off the grid."""
    c = RC.levels_case(per_frame)
    got = record_window(run, c)
    assert np.array_equal(got["frames"][1:257], c["levels"]) and got["off_grid"][0] == 0
    RC.assert_same(got, RC.restate(c), f"levels, per_frame {per_frame}")


@pytest.mark.parametrize("run,per_frame", abi.arms(abi.Simt, abi.Gpu, list(RC.PER_FRAMES)))
def test_record_window_off_grid_flag(run, per_frame):
    """One value off the grid -- among the steps, among the final observations, beyond [-1, 1] -- sets the flag (and is stored
    as its nearest level); a window on the grid leaves it 0 (the cases above)."""
    for where, index, value in (("obs", (17, per_frame - 1), np.float32(0.3333)), ("final_obs", (2, 0), np.nextafter(np.float32(1), np.float32(0))),
                                ("obs", (0, 0), np.float32(1.5)), ("obs", (47, 3), np.float32(np.nan))):
        c = RC.make_case(per_frame, np.uint8, 37, seed=5)
        c["window"][where][index] = value
        want = RC.restate(c)
        assert want["off_grid"][0] == 1
        RC.assert_same(record_window(run, c), want, f"{where}{index} = {value}")
    c = RC.make_case(per_frame, np.uint8, 37, seed=5)
    c["runs"] = c["runs"][:5]
    c["window"]["obs"][40, 0] = 0.123  # a step no run takes: not looked at
    want = RC.restate(c)
    assert want["off_grid"][0] == 0
    RC.assert_same(record_window(run, c), want, "off-grid value outside every run")


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_record_window_without_runs_touches_nothing(run):
    c = RC.make_case(108, np.int64, 5)
    c["runs"] = c["runs"][:0]
    rc, msg, got = record_window(run, c, status=True)
    assert rc == 0
    RC.assert_same(got, RC.restate(c), "R = 0")
    assert (got["frames"][8:] == RC.POISON).all() and got["off_grid"][0] == 0
    rc, _, _ = record_window(run, c, status=True, **{k: None for k in POINTERS})  # nothing is followed
    assert rc == 0


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_record_window_refuses_bad_arguments(run):
    c = RC.make_case(25, np.uint8, 5)
    want = {k: c[k] for k in RC.ARENA}
    bad = [{k: None} for k in POINTERS if k not in ("final_obs", "finals")]
    bad += [dict(flag_size=4), dict(flag_size=0), dict(final_obs=None), dict(finals=None), dict(per_frame=0), dict(R=-1), dict(total=-1),
            dict(steps=-1), dict(K=-1), dict(F=-1), dict(E=-1), dict(total=1 << 31), dict(per_frame=1 << 40)]
    for kw in bad:
        rc, msg, got = record_window(run, c, status=True, **kw)
        assert rc != 0 and "record_window" in msg, (kw, rc, msg)
        for k in RC.ARENA:  # refused before anything was launched
            assert np.array_equal(got[k], want[k]), (kw, k)
    rc, msg, got = record_window(run, c, status=True)
    assert rc == 0, msg
    RC.assert_same(got, RC.restate(c), "the same case, accepted")


def test_record_window_params_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of the ctypes mirror against the C struct (compiled with gcc from include/diamond_hip.h)."""
    fields = [f for f, _ in nv.RecordWindowParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_record_window_params));' + "".join(
        f'printf("%zu ", offsetof(dmd_record_window_params, {f}));' for f in fields)
    src = tmp_path / "s.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    mine = [ctypes.sizeof(nv.RecordWindowParams)] + [getattr(nv.RecordWindowParams, f).offset for f in fields]
    assert got == mine, list(zip(["sizeof"] + fields, got, mine))
    assert set(fields) >= set(POINTERS)
    assert "dmd_record_window" in nv.EXPORTS and "dmd_record_window" in nv.LAUNCHERS
