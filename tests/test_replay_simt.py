"""The device-resident replay store (diamond_amd/replay.py, dmd_segment_gather) without a GPU:

  * the kernel's own source on the SIMT interpreter (tests/simt), every array between inaccessible pages, bit for bit against
    the numpy restatement of tests/replay_cases.py;
  * DeviceReplay / DeviceSegmentLoader against what the REFERENCE's Dataset, BatchSampler, make_segment,
    collate_segments_to_batch and DatasetTraverser produced (tests/golden/replay_segments.pt, make_replay_golden.py);
  * the host logic: growth, replacement, compaction, validation, the ctypes mirror of the parameter block.
"""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests.conftest import load_golden
from tests.simt import loader as S
from tests.simt.fence import fenced as G
from tests.simt.host_harness import engine_on_interpreter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _poisoned(shape, dtype):
    """An output the kernel must overwrite completely: NaN (floats) / a bit pattern no result has (integers)."""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = 0xFF if np.issubdtype(dtype, np.floating) else 0x5A
    return G(a)


def _run(arena, seg, t, flag_dtype, put_back, tight="end", skip=(), misalign=False):
    from diamond_amd import native as nv

    L = S.lib()
    b, pf = len(seg), arena["frames"].shape[1]
    ins = {k: G(arena[k], tight=tight) for k in ("frames", "act", "rew", "end", "trunc", "finals")}
    segf = G(seg, tight=tight)
    shapes = {"obs": ((b, t, pf), np.float32), "act": ((b, t), np.int64), "rew": ((b, t), np.float32), "end": ((b, t), flag_dtype),
              "trunc": ((b, t), flag_dtype), "mask_padding": ((b, t), np.uint8), "final_obs": ((b, pf), np.float32)}
    out = {k: _poisoned(*v) for k, v in shapes.items() if k not in skip}
    if misalign:  # a frame output 4 bytes off a 16-byte boundary: the entry must leave its vector paths
        big = _poisoned((b * t * pf + 1,), np.float32)
        out["obs"] = big[1:].reshape(b, t, pf)
        assert out["obs"].ctypes.data % 16 == 4
    p = nv.SegmentGatherParams()
    p.B, p.T, p.per_frame, p.flag_size, p.put_back_final = b, t, pf, np.dtype(flag_dtype).itemsize, int(put_back)
    p.frames, p.act, p.rew, p.end, p.trunc = (ins[k].ctypes.data for k in ("frames", "act", "rew", "end", "trunc"))
    p.finals = ins["finals"].ctypes.data if len(arena["finals"]) else None
    p.seg = segf.ctypes.data
    for field, k in (("out_obs", "obs"), ("out_act", "act"), ("out_rew", "rew"), ("out_end", "end"), ("out_trunc", "trunc"),
                     ("out_mask", "mask_padding"), ("out_final", "final_obs")):
        setattr(p, field, out[k].ctypes.data if k in out else None)
    S.check(L.dmd_segment_gather(ctypes.byref(p), None), "dmd_segment_gather")
    return out


@pytest.mark.parametrize("put_back", [False, True])
@pytest.mark.parametrize("flag_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("t", RC.SEQ_LENGTHS)
@pytest.mark.parametrize("per_frame", RC.PER_FRAMES)
def test_segment_gather_matches_the_restatement(per_frame, t, flag_dtype, put_back):
    """Every segment of T steps that overlaps an episode (lengths 1, 2, 7, 30; last step end / trunc / neither), as B = 1 and in
    batches of 37, the inputs fenced at their ends or (put_back cases) at their starts, every output pre-filled with NaN."""
    arena = RC.make_arena(per_frame, seed=per_frame + t)
    seg_all = RC.all_segments(arena, t)
    for i, seg in enumerate(RC.batches(seg_all)):
        got = _run(arena, seg, t, flag_dtype, put_back, tight="start" if put_back else "end")
        RC.assert_same(got, RC.restate(arena, seg, t, flag_dtype, put_back), RC.OUTPUTS, f"batch {i} (B = {len(seg)})")


@pytest.mark.parametrize("misalign", [False, True], ids=["words", "scalar"])
def test_segment_gather_dequantises_all_256_levels_like_the_division(misalign):
    """The kernel forms q / 255 as a multiplication plus one residual step: every level, in the word path and the scalar path,
    must give the bits of the fp32 division the reference performs (numpy's, in the restatement)."""
    arena = RC.levels_arena()
    assert all(sorted(row.tolist()) == list(range(256)) for row in arena["frames"])
    seg = RC.all_segments(arena, 5)[::4]
    got = _run(arena, seg, 5, np.uint8, True, misalign=misalign)
    RC.assert_same(got, RC.restate(arena, seg, 5, np.uint8, True), RC.OUTPUTS, "all levels")
    assert len(np.unique(got["obs"])) == 257  # the 256 dequantised levels and the padding's 0.0


def test_segment_gather_puts_the_final_frame_back_only_after_an_end():
    """The property the put_back cases rest on, spelled out on the restatement's inputs: a frame of padding becomes the final
    observation exactly where the episode's LAST step has end != 0 and the segment reaches one step beyond it."""
    arena = RC.make_arena(192, seed=3)
    seg = RC.all_segments(arena, 5)
    off, on = (_run(arena, seg, 5, np.uint8, pb) for pb in (False, True))
    changed = (RC.bits(off["obs"]).reshape(len(seg), 5, -1) != RC.bits(on["obs"]).reshape(len(seg), 5, -1)).any(-1)
    expect = np.zeros_like(changed)
    for i, (first, start, n, row) in enumerate(seg):
        k = n - start
        if arena["end"][first + n - 1] and row >= 0 and 1 <= k < 5:
            expect[i, k] = True
    assert expect.sum() >= 10 and np.array_equal(changed, expect)
    assert not on["mask_padding"][changed].any()  # it stays padding for the loss
    for k in ("act", "rew", "end", "trunc", "mask_padding", "final_obs"):
        assert np.array_equal(RC.bits(off[k]), RC.bits(on[k]))


@pytest.mark.parametrize("skip", [("obs",), ("final_obs",), ("act", "rew", "end", "trunc", "mask_padding"), ("obs", "final_obs", "trunc")])
def test_segment_gather_null_outputs_are_left_alone(skip):
    arena = RC.make_arena(108, seed=9)
    seg = RC.all_segments(arena, 5)[::3]
    got = _run(arena, seg, 5, np.int64, True, skip=skip)
    RC.assert_same(got, RC.restate(arena, seg, 5, np.int64, True), tuple(k for k in RC.OUTPUTS if k not in skip), f"without {skip}")


def test_segment_gather_unaligned_output_and_no_finals():
    """per_frame = 192 with a frame output that is not 16-byte aligned (the scalar path must be taken: a 16-byte store there
    faults on the fence or tears), and an arena without any final frame (finals = NULL; final_row is then never followed)."""
    arena = RC.make_arena(192, seed=1)
    seg = RC.all_segments(arena, 5)[::2]
    got = _run(arena, seg, 5, np.uint8, True, misalign=True)
    RC.assert_same(got, RC.restate(arena, seg, 5, np.uint8, True), RC.OUTPUTS, "misaligned obs")
    bare = dict(arena, finals=arena["finals"][:0])
    want = RC.restate(dict(arena, final_row=np.full_like(arena["final_row"], -1)), np.concatenate([seg[:, :3], -np.ones((len(seg), 1), np.int64)], 1),
                      5, np.uint8, True)
    RC.assert_same(_run(bare, seg, 5, np.uint8, True), want, RC.OUTPUTS, "finals = NULL")


def test_segment_gather_refuses_bad_arguments():
    from diamond_amd import native as nv

    L = S.lib()
    arena = RC.make_arena(25)
    seg = RC.all_segments(arena, 5)[:2]
    keep = {k: G(arena[k]) for k in ("frames", "act", "rew", "end", "trunc")}
    segf = G(seg)
    obs = G(np.zeros((2, 5, 25), np.float32))

    def params(**kw):
        p = nv.SegmentGatherParams()
        p.B, p.T, p.per_frame, p.flag_size = 2, 5, 25, 1
        for k, v in keep.items():
            setattr(p, k, v.ctypes.data)
        p.seg, p.out_obs = segf.ctypes.data, obs.ctypes.data
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert L.dmd_segment_gather(ctypes.byref(params()), None) == 0
    for bad in (dict(T=0), dict(flag_size=4), dict(flag_size=0), dict(seg=None), dict(frames=None), dict(act=None), dict(rew=None),
                dict(end=None), dict(trunc=None), dict(per_frame=0)):
        assert L.dmd_segment_gather(ctypes.byref(params(**bad)), None) != 0, bad
        assert b"segment_gather" in L.dmd_last_error()


def test_segment_gather_params_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of the ctypes mirror against the C struct (compiled with gcc from include/diamond_hip.h)."""
    from diamond_amd import native as nv

    fields = [f for f, _ in nv.SegmentGatherParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_segment_gather_params));' + "".join(
        f'printf("%zu ", offsetof(dmd_segment_gather_params, {f}));' for f in fields)
    src = tmp_path / "s.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    mine = [ctypes.sizeof(nv.SegmentGatherParams)] + [getattr(nv.SegmentGatherParams, f).offset for f in fields]
    assert got == mine, list(zip(["sizeof"] + fields, got, mine))
    assert "dmd_segment_gather" in nv.EXPORTS and "dmd_segment_gather" in nv.LAUNCHERS


# ---------------------------------------------------------------------------------------------------------------------------
# the store against the reference's pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def _episode(e, as_float, flag_dtype=torch.uint8):
    obs = RC_dequant_t(e["obs"]) if as_float else e["obs"]
    info = {} if e["final"] is None else {"final_observation": RC_dequant_t(e["final"]) if as_float else e["final"]}
    return SimpleNamespace(obs=obs, act=e["act"], rew=e["rew"], end=e["end"].to(flag_dtype), trunc=e["trunc"].to(flag_dtype), info=info)


def RC_dequant_t(u8):
    return u8.div(255).mul(2).sub(1)


@pytest.fixture(scope="module")
def golden():
    return load_golden("replay_segments.pt")


@pytest.fixture()
def store(golden):
    """The golden episodes in a DeviceReplay on the interpreter: odd episodes arrive as fp32 frames (quantised by
    dmd_quantize_u8), even ones as uint8 levels."""
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        for i, e in enumerate(golden["episodes"]):
            assert s.add_episode(_episode(e, as_float=bool(i % 2))) == i
        yield s


def _assert_batch(batch, want, what):
    for k in ("obs", "act", "rew", "end", "trunc", "mask_padding"):
        g, w = getattr(batch, k), want[k]
        if k == "obs":
            g = g.reshape(w.shape)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(RC.bits(g.numpy()), RC.bits(w.numpy())), (what, k)
    assert [(s.episode_id, s.start, s.stop) for s in batch.segment_ids] == want["segment_ids"], what
    assert len(batch.info) == len(want["final_observation"])
    for info, fo in zip(batch.info, want["final_observation"]):
        if fo is None:
            assert info == {}
        else:
            assert set(info) == {"final_observation"} and info["final_observation"].dtype == fo.dtype
            assert np.array_equal(RC.bits(info["final_observation"].numpy()), RC.bits(fo.numpy())), what


def test_sample_ids_and_gather_reproduce_the_reference(golden, store):
    """The same numpy seed -> the reference BatchSampler's ids, for both padding modes, with and without sample_weights, and
    (rank, world) in {(0, 1), (1, 2), (2, 4)}; `gather` of those ids -> collate_segments_to_batch's fields, bit for bit."""
    assert len(golden["samples"]) == 12
    assert store.num_episodes == 6 and store.num_steps == sum(len(e["act"]) for e in golden["episodes"])
    assert store.lengths.tolist() == [len(e["act"]) for e in golden["episodes"]]
    assert store.start_idx.tolist() == np.cumsum([0] + store.lengths.tolist())[:-1].tolist()
    for s in golden["samples"]:
        np.random.seed(s["seed"])
        ids = store.sample_ids(s["batch_size"], s["seq_length"], can_sample_beyond_end=s["can_sample_beyond_end"],
                               sample_weights=s["sample_weights"], rank=s["rank"], world_size=s["world_size"])
        assert [(i.episode_id, i.start, i.stop) for i in ids] == s["ids"], s["seed"]
        with engine_on_interpreter():
            _assert_batch(store.gather(ids), s["batch"], f"seed {s['seed']}")
    # a private RandomState draws the same ids as the global state it was seeded like
    s = golden["samples"][3]
    ids = store.sample_ids(s["batch_size"], s["seq_length"], can_sample_beyond_end=s["can_sample_beyond_end"],
                           sample_weights=s["sample_weights"], rank=s["rank"], world_size=s["world_size"], rng=np.random.RandomState(s["seed"]))
    assert [(i.episode_id, i.start, i.stop) for i in ids] == s["ids"]


def test_traverse_reproduces_the_reference_traverser(golden, store):
    tr = golden["traverser"]
    with engine_on_interpreter():
        got = list(store.traverse(tr["batch_num_samples"], tr["chunk_size"]))
    assert len(got) == len(tr["batches"]) >= 3
    assert len(tr["batches"][-1]["act"]) < tr["batch_num_samples"]  # the short last batch is among the cases
    for i, (b, w) in enumerate(zip(got, tr["batches"])):
        _assert_batch(b, w, f"traverser batch {i}")


def test_loader_yields_the_sampled_batches_without_torch_draws(golden, store, monkeypatch):
    from diamond_amd.replay import DeviceSegmentLoader
    from diamond_amd.world_model_env import _no_random_draws

    monkeypatch.setenv("DIAMOND_CHECK_RESET_RNG", "1")
    s = golden["samples"][0]
    loader = DeviceSegmentLoader(store, s["batch_size"], s["seq_length"], rng=np.random.RandomState(s["seed"]))
    assert loader.batch_sampler.batch_size == s["batch_size"]
    with engine_on_interpreter(), _no_random_draws(torch.device("cpu"), "DeviceSegmentLoader"):
        it = iter(loader)
        first, second = next(it), next(it)
    _assert_batch(first, s["batch"], "loader")
    assert [(i.episode_id, i.start, i.stop) for i in first.segment_ids] != [(i.episode_id, i.start, i.stop) for i in second.segment_ids]
    assert first.to("cpu").obs.shape == first.obs.shape


def test_gather_into_preallocated_tensors_and_int64_flags(golden):
    """`out=`: the batch's fields ARE the given tensors; end / trunc keep the dtype of the first episode (int64 here)."""
    from diamond_amd.replay import DeviceReplay

    s = golden["samples"][5]
    with engine_on_interpreter():
        store = DeviceReplay.from_episodes((_episode(e, False, torch.int64) for e in golden["episodes"]), device="cpu")
        plain = store.gather(s["ids"], put_back_final=True)
        out = {k: torch.full_like(getattr(plain, k), 77) for k in ("obs", "act", "rew", "end", "mask_padding")}
        batch = store.gather(s["ids"], out=out, put_back_final=True, info=False)
        static = store.descriptor(s["ids"])
        out2 = {k: torch.full_like(v, 55) for k, v in out.items()}
        store.gather_static(static, out2, put_back_final=True)
    assert plain.end.dtype == plain.trunc.dtype == torch.int64 and batch.info == [{}] * len(s["ids"])
    for k, v in out.items():
        assert getattr(batch, k) is v or getattr(batch, k).data_ptr() == v.data_ptr()
        assert torch.equal(v, getattr(plain, k)) and torch.equal(out2[k], v), k
    assert torch.equal(plain.end, s["batch"]["end"].long()) and torch.equal(plain.mask_padding, s["batch"]["mask_padding"])
    with engine_on_interpreter():
        with pytest.raises(ValueError, match="out\\['obs'\\]"):
            store.gather(s["ids"], out={"obs": torch.zeros(1, 2, 3)})


# ---------------------------------------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------------------------------------
def _ep(n, seed, frame=(3, 8, 8), end_last=False, final=False):
    g = torch.Generator().manual_seed(seed)
    end = torch.zeros(n, dtype=torch.uint8)
    end[-1] = int(end_last)
    info = {"final_observation": torch.randint(0, 256, frame, generator=g, dtype=torch.uint8)} if final else {}
    return SimpleNamespace(obs=torch.randint(0, 256, (n,) + frame, generator=g, dtype=torch.uint8), act=torch.randint(0, 4, (n,), generator=g),
                           rew=torch.randn(n, generator=g), end=end, trunc=torch.zeros(n, dtype=torch.uint8), info=info)


def _whole(store, eid):
    n = int(store.lengths[eid])
    return store.gather([(eid, 0, n)])


def _assert_holds(store, eid, ep):
    b = _whole(store, eid)
    assert torch.equal(b.obs[0], RC_dequant_t(ep.obs)) and torch.equal(b.act[0], ep.act) and torch.equal(b.rew[0], ep.rew)
    assert torch.equal(b.end[0], ep.end) and bool(b.mask_padding.all())
    if "final_observation" in ep.info:
        assert torch.equal(b.info[0]["final_observation"], RC_dequant_t(ep.info["final_observation"]))
    else:
        assert b.info[0] == {}


def test_growth_reserve_and_generation():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu", frame_shape=(3, 8, 8), capacity_frames=8)
        assert s.generation == 1 and s.frames.shape == (8, 192) and s.nbytes == 8 * (192 + 8 + 4 + 1 + 1)
        eps = [_ep(n, i) for i, n in enumerate((3, 5, 2, 9))]
        s.add_episode(eps[0]), s.add_episode(eps[1])
        assert s.generation == 1  # within the reservation: no reallocation
        s.add_episode(eps[2])     # 10 rows > 8: the arena doubles
        assert s.generation == 2 and s.frames.shape[0] == 16
        s.add_episode(eps[3])     # 19 rows > 16: doubles again
        assert s.generation == 3 and s.frames.shape[0] == 32
        s.reserve(20)
        assert s.generation == 3
        s.reserve(100)            # beyond twice the capacity: exactly what was asked for
        assert s.generation == 4 and s.frames.shape[0] == 100
        assert (s.num_episodes, s.num_steps, len(s)) == (4, 19, 19) and s.wasted_frames == 0
        assert s.lengths.tolist() == [3, 5, 2, 9] and s.start_idx.tolist() == [0, 3, 8, 10]
        for i, e in enumerate(eps):
            _assert_holds(s, i, e)
        lazy = DeviceReplay("cpu", capacity_frames=64)  # the frame shape comes with the first episode
        lazy.add_episode(eps[0])
        assert lazy.frames.shape == (64, 192) and lazy.generation == 1


def test_collector_style_replacement_wasted_frames_and_compact():
    """The collector re-adds a growing episode under its id (reference data/dataset.py:101-109): in place while it is the arena's
    last episode or fits its slot; otherwise appended, the old slot counted in wasted_frames until compact()."""
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        a, b = _ep(4, 1), _ep(3, 2)
        s.add_episode(a), s.add_episode(b)
        b2 = _ep(7, 3, end_last=True, final=True)  # the last episode grows where it is
        assert s.add_episode(b2, episode_id=1) == 1
        assert s.wasted_frames == 0 and s._used == 11 and s.lengths.tolist() == [4, 7] and s.num_steps == 11
        a2 = _ep(2, 4)  # shrinks inside its slot
        s.add_episode(a2, episode_id=0)
        assert s.wasted_frames == 0 and s._used == 11 and s.start_idx.tolist() == [0, 2] and s.num_steps == 9
        a3 = _ep(4, 5)  # regrows within the slot it always had
        s.add_episode(a3, episode_id=0)
        assert s.wasted_frames == 0 and s._used == 11
        a4 = _ep(6, 6, final=True)  # no longer fits and is not last: appended, the old 4 rows are a hole
        s.add_episode(a4, episode_id=0)
        assert s.wasted_frames == 4 and s._used == 17 and s.lengths.tolist() == [6, 7] and s.start_idx.tolist() == [0, 6]
        c = _ep(5, 7)
        s.add_episode(c)
        for i, e in enumerate((a4, b2, c)):
            _assert_holds(s, i, e)
        gen = s.generation
        s.compact()
        assert s.wasted_frames == 0 and s._used == 18 == s.num_steps and s.generation == gen + 1
        assert s._first.tolist() == s.start_idx.tolist() == [0, 6, 13]
        for i, e in enumerate((a4, b2, c)):
            _assert_holds(s, i, e)
        b3 = _ep(7, 8)  # the final observation goes away with the replacement
        s.add_episode(b3, episode_id=1)
        _assert_holds(s, 1, b3)
        s.compact()
        assert s._finals_used == 1
        for i, e in enumerate((a4, b3, c)):
            _assert_holds(s, i, e)


def test_off_grid_frames_and_invalid_ids_raise_before_any_launch(monkeypatch):
    from diamond_amd import native as nv
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        good = _ep(5, 1)
        s.add_episode(good)
        off = _ep(3, 2)
        off.obs = RC_dequant_t(off.obs)
        off.obs[1, 2, 3, 4] += 1e-3
        with pytest.raises(ValueError, match="episode 1.*not on the uint8 grid"):
            s.add_episode(off)
        off2 = _ep(3, 2, final=True)
        off2.info["final_observation"] = RC_dequant_t(off2.info["final_observation"]) * 0.999
        with pytest.raises(ValueError, match="episode 1: final_observation.*not on the uint8 grid"):
            s.add_episode(off2)
        with pytest.raises(ValueError, match="episode 0: final_observation.*not on the uint8 grid"):
            s.add_episode(off2, episode_id=0)
        with pytest.raises(ValueError, match="frames of shape"):
            s.add_episode(_ep(3, 2, frame=(3, 6, 6)))
        assert s.num_episodes == 1 and s.num_steps == 5
        _assert_holds(s, 0, good)  # the refused episodes left the stored one alone
        s.add_episode(_ep(4, 3))

        launches = []
        real = nv._lib
        monkeypatch.setattr(nv, "_lib", SimpleNamespace(dmd_segment_gather=lambda *a: launches.append(a) or 0, dmd_last_error=lambda: b""))
        for bad, why in (([(0, 5, 8)], "outside"),            # start >= len
                         ([(0, -4, 0)], "outside"),           # stop <= 0
                         ([(0, 3, 3)], "outside"),            # start >= stop
                         ([(0, 4, 2)], "outside"),
                         ([(0, 0, 3), (1, 0, 4)], "steps"),   # unequal lengths
                         ([(2, 0, 3)], "episode 2"), ([(-1, 0, 3)], "episode -1"), ([], "no segment")):
            with pytest.raises(ValueError, match=why):
                s.gather(bad)
        assert launches == []
        s.gather([(0, -2, 3), (1, 2, 7)])
        assert len(launches) == 1
        monkeypatch.setattr(nv, "_lib", real)
