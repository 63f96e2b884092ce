"""diamond_amd.collector and DeviceReplay.record_window without a GPU (the kernels on the SIMT interpreter):

  * the script of tests/collector_cases.py through diamond_amd.collector into a DeviceReplay, against what the REFERENCE's
    make_collector, make_env_loop, Dataset and Episode produced on the same scripted env and policy
    (tests/golden/collector_episodes.pt, make_collector_golden.py): logs, ids, lengths, counts, every episode bit for bit;
  * the host logic: slots that grow in place and by a move, wasted_frames and compact(), generation, end_collect both ways, the
    deferred off-grid error, the counters under add_episode's replacement.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import collector_cases as CC
from tests.conftest import load_golden
from tests.simt.host_harness import engine_on_interpreter

FRAME = CC.FRAME


@pytest.fixture(scope="module")
def golden():
    return load_golden("collector_episodes.pt")


def golden_episodes(g):
    """The golden's back-to-back episodes as add_episode takes them (uint8 levels)."""
    eps, at = [], 0
    for n, row in zip(g["lengths"], g["final_row"]):
        info = {} if row < 0 else {"final_observation": g["finals"][row]}
        eps.append(SimpleNamespace(**{k: g[k][at:at + n] for k in ("obs", "act", "rew", "end", "trunc")}, info=info))
        at += n
    return eps


def snapshot(store):
    return {"num_episodes": int(store.num_episodes), "num_steps": int(store.num_steps), "lengths": store.lengths.tolist(),
            "start_idx": store.start_idx.tolist(), "counts_rew": list(store.counts_rew), "counts_end": list(store.counts_end)}


def assert_episode(got, want, what):
    """`got`: load_episode's; `want`: a golden episode (levels).  The reference's fields and dtypes, bit for bit."""
    got = got.to("cpu")
    assert (got.obs.dtype, got.act.dtype, got.rew.dtype, got.end.dtype, got.trunc.dtype) == (torch.float32, torch.int64, torch.float32,
                                                                                               torch.uint8, torch.uint8), what
    assert torch.equal(got.obs, CC.dequant(want.obs)) and got.obs.shape[1:] == FRAME, what
    for k in ("act", "rew", "end", "trunc"):
        assert torch.equal(getattr(got, k), getattr(want, k)), (what, k)
    assert set(got.info) == set(want.info), what
    if want.info:
        assert got.info["final_observation"].shape == FRAME and torch.equal(got.info["final_observation"], CC.dequant(want.info["final_observation"])), what


def assert_store_holds(store, eps, what):
    from diamond_amd.replay import DeviceReplay

    assert store.num_episodes == len(eps), what
    for i, e in enumerate(eps):
        assert_episode(store.load_episode(i), e, f"{what}: episode {i}")
    ref = DeviceReplay.from_episodes(eps, device=store.device)
    for seed, beyond in ((1, False), (2, True)):
        ids = []
        for s in (store, ref):
            np.random.seed(seed)
            ids.append(s.sample_ids(5, 4, can_sample_beyond_end=beyond))
        assert ids[0] == ids[1], what
        a, b = store.gather(ids[0], put_back_final=True), ref.gather(ids[1], put_back_final=True)
        for k in ("obs", "act", "rew", "end", "trunc", "mask_padding"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
        assert [sorted(i) for i in a.info] == [sorted(i) for i in b.info]
        assert all(torch.equal(x["final_observation"], y["final_observation"]) for x, y in zip(a.info, b.info) if x), what


def run_golden_script(g, num_envs, device, window):
    from diamond_amd.collector import NumToCollect, make_collector
    from diamond_amd.replay import DeviceReplay

    store = DeviceReplay(device, name=CC.NAME)
    for i, logs in enumerate(CC.run_script(num_envs, make_collector, NumToCollect, store, device=device, window=window)):
        want = g["collects"][i]
        assert [list(d.items()) for d in logs] == [list(d.items()) for d in want["logs"]], (i, logs, want["logs"])
        assert snapshot(store) == want["dataset"], (i, snapshot(store), want["dataset"])
        if i in (2, 4):
            assert_store_holds(store, golden_episodes(g["episodes"]["train" if i == 2 else "test"]), f"collect {i}")
    assert i == 4
    return store


@pytest.mark.parametrize("window", [64, 2, 1])
@pytest.mark.parametrize("num_envs", CC.NUM_ENVS)
def test_collector_reproduces_the_reference_collector(golden, num_envs, window):
    """Whatever the window (the whole collect at once, two env steps, one), the logs of the five collects equal the reference's in
    order, and after each collect so do num_steps, lengths, start_idx and the counts; after each phase every episode is bitwise
    the reference's and sampled batches are those of a store the golden episodes were add_episode'd to."""
    with engine_on_interpreter():
        store = run_golden_script(golden[num_envs], num_envs, "cpu", window)
        assert store.wasted_frames >= 0 and store._open == {}  # (reset_every_collect lets go of the unfinished ones)


# ---------------------------------------------------------------------------------------------------------------------------
# host logic
# ---------------------------------------------------------------------------------------------------------------------------
def window_of(b, t, seed, deaths=(), flag_dtype=torch.uint8):
    """(obs, act, rew, end, trunc, final_observation or None): random frames on the grid; deaths: ((env, step, "end" | "trunc"), ...)"""
    g = torch.Generator().manual_seed(seed)
    obs = CC.dequant(torch.randint(0, 256, (b, t) + FRAME, generator=g, dtype=torch.uint8))
    act, rew = torch.randint(0, 4, (b, t), generator=g), torch.randint(-2, 3, (b, t), generator=g).float()
    end, trunc = torch.zeros(b, t, dtype=flag_dtype), torch.zeros(b, t, dtype=flag_dtype)
    for env, step, how in deaths:
        (end if how == "end" else trunc)[env, step] = 1
    order = sorted((step, env) for env, step, _ in deaths)
    final = CC.dequant(torch.randint(0, 256, (len(order),) + FRAME, generator=g, dtype=torch.uint8)) if order else None
    return obs, act, rew, end, trunc, final


def joined(windows, env, t0=0, t1=None):
    """env's steps of consecutive windows as one episode (levels), without a final observation"""
    cat = [torch.cat([w[k][env] for w in windows])[t0:t1] for k in range(5)]
    return SimpleNamespace(obs=CC.levels(cat[0]), act=cat[1], rew=cat[2], end=cat[3], trunc=cat[4], info={})


def test_slots_grow_in_place_and_by_a_move_within_one_reservation():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu", frame_shape=FRAME, capacity_frames=256, name="x")
        s.reserve(256, n_finals=8)
        gen = s.generation
        ws = [window_of(2, 6, 1, deaths=((1, 4, "end"),)), window_of(2, 3, 2), window_of(2, 4, 3)]
        # env 0: 6 rows in a slot of 12 at row 0; env 1: an episode of 5 rows (it ended: no spare rows), then 1 row in a slot of 2
        assert s.record_window(*ws[0]) == [{"episode_id": 0, "length": 5, "return": float(ws[0][2][1, :5].sum())}]
        assert (s._used, s.wasted_frames, s.num_episodes, s.num_steps) == (19, 0, 1, 5)  # the open ones are not stored before end_collect
        s.record_window(*ws[1])  # env 0: 9 rows, fits; env 1: 4 rows > 2 and the arena's last: grows where it is, to 8
        assert (s._used, s.wasted_frames) == (25, 0) and (s._open[1].first, s._open[1].slot) == (17, 8)
        s.record_window(*ws[2])  # env 0: 13 rows > 12 and not the arena's last: moves to its end, slot 26; env 1: 8 rows, fits
        assert (s._used, s.wasted_frames) == (51, 12) and (s._open[0].first, s._open[0].slot) == (25, 26)
        assert s.generation == gen and s.frames.shape[0] == 256  # inside the reservation: the arena's pointers held
        s.end_collect(keep_open=True)
        s.assert_on_grid()
        assert s.lengths.tolist() == [5, 13, 8] and s.start_idx.tolist() == [0, 5, 18] and s.num_steps == 26
        want = [joined(ws, 1, 0, 5), joined(ws, 0), joined(ws, 1, 5)]
        want[0].info = {"final_observation": CC.levels(ws[0][5][0])}
        assert_store_holds(s, want, "grown")
        s.compact()
        assert (s._used, s.wasted_frames, s.generation) == (26, 0, gen + 1) and s._first.tolist() == [0, 5, 18]
        assert_store_holds(s, want, "compacted")
        ws.append(window_of(2, 2, 4, deaths=((0, 1, "trunc"),)))  # the open episodes go on after compact(): env 0 ends, env 1 grows
        done = s.record_window(*ws[3])
        assert done == [{"episode_id": 1, "length": 15, "return": float(sum(w[2][0].sum() for w in ws))}]
        assert s.wasted_frames == 13 + 8  # (compact() left no spare rows: both moved)
        s.end_collect(keep_open=True)
        s.assert_on_grid()
        want = [want[0], joined(ws, 0), joined(ws, 1, 5)]
        want[1].info = {"final_observation": CC.levels(ws[3][5][0])}
        assert_store_holds(s, want, "extended after compact")
        assert s.counts_end == [29, 1] and s.counts_rew == [int(sum((w[2] < 0).sum() for w in ws)), int(sum((w[2] == 0).sum() for w in ws)),
                                                            int(sum((w[2] > 0).sum() for w in ws))]


def test_the_arena_grows_when_a_window_does_not_fit():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        ws = [window_of(3, 5, 7, flag_dtype=torch.int64), window_of(3, 5, 8, deaths=((1, 2, "end"), (0, 4, "end"), (2, 4, "trunc")), flag_dtype=torch.int64)]
        s.record_window(*ws[0])
        gen = s.generation
        done = s.record_window(*ws[1])
        assert s.generation > gen and s.flag_dtype == torch.int64
        assert [(d["episode_id"], d["length"]) for d in done] == [(0, 8), (1, 10), (2, 10)]  # by death: step 2 env 1, step 4 envs 0, 2
        s.end_collect(keep_open=True)
        s.assert_on_grid()
        assert s.lengths.tolist() == [8, 10, 10, 2]
        want = [joined(ws, 1, 0, 8), joined(ws, 0), joined(ws, 2), joined(ws, 1, 8)]
        for w, row in zip(want[:3], range(3)):
            w.info = {"final_observation": CC.levels(ws[1][5][row])}
            w.end, w.trunc = w.end.to(torch.uint8), w.trunc.to(torch.uint8)
        want[3].end, want[3].trunc = want[3].end.to(torch.uint8), want[3].trunc.to(torch.uint8)
        for i, w in enumerate(want):
            assert_episode(s.load_episode(i), w, f"episode {i}")
        assert s.gather([(0, 0, 8)]).end.dtype == torch.int64  # batches keep the env's flag dtype, load_episode gives the reference's


def test_end_collect_keeps_or_drops_the_unfinished_episodes():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu", name="t")
        w0 = window_of(2, 3, 11)
        s.record_window(*w0)
        s.end_collect(keep_open=False)  # never stored: the rows come back at once (both were the arena's last in turn)
        assert (s._used, s.wasted_frames, s.num_episodes, s._open) == (0, 0, 0, {})
        w1 = window_of(2, 3, 12, deaths=((0, 0, "end"),))
        done = s.record_window(*w1)
        assert [d["episode_id"] for d in done] == [0] and s.num_episodes == 1
        s.end_collect(keep_open=False)  # env 0's second episode and env 1's first are dropped; the arena's last rows come back
        assert s.num_episodes == 1 and s.num_steps == 1 and s.lengths.tolist() == [1] and s._open == {}
        assert s._used + s.wasted_frames <= 1 + 4 + 6 and s.counts_end == [0, 1]
        w2 = window_of(2, 2, 13)
        s.record_window(*w2)
        s.end_collect(keep_open=True)   # stored as far as they go, in env order, and still open
        assert s.lengths.tolist() == [1, 2, 2] and sorted(s._open) == [0, 1]
        w3 = window_of(2, 2, 14, deaths=((1, 1, "trunc"),))
        done = s.record_window(*w3)
        assert [(d["episode_id"], d["length"]) for d in done] == [(2, 4)] and s.lengths.tolist() == [1, 2, 4]  # env 0's waits for end_collect
        s.end_collect(keep_open=False)  # a STORED episode stays as it was last stored
        s.assert_on_grid()
        assert s.lengths.tolist() == [1, 2, 4] and s.num_steps == 7
        want = [joined([w1], 0, 0, 1), joined([w2], 0), joined([w2, w3], 1)]
        want[0].info = {"final_observation": CC.levels(w1[5][0])}
        want[2].info = {"final_observation": CC.levels(w3[5][0])}
        assert_store_holds(s, want, "kept")
        s.compact()
        assert s.wasted_frames == 0 and s._used == 7
        assert_store_holds(s, want, "compacted")
        s.clear()
        assert snapshot(s) == {"num_episodes": 0, "num_steps": 0, "lengths": [], "start_idx": [], "counts_rew": [0, 0, 0], "counts_end": [0, 0]}


def test_off_grid_frames_are_reported_later_and_by_episode():
    from diamond_amd.replay import DeviceReplay

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        s.record_window(*window_of(2, 3, 21))
        s.assert_on_grid()
        bad = list(window_of(2, 3, 22, deaths=((1, 1, "end"),)))
        bad[0][1, 2, 1, 3, 4] += 1e-3  # env 1's NEXT episode
        done = s.record_window(*bad)    # does not wait for its launch: nothing raises here
        assert [d["episode_id"] for d in done] == [0]
        s.end_collect(keep_open=True)
        with pytest.raises(ValueError, match=r"episodes \[0, 1, 2\]: fp32 frames are not on the uint8 grid"):
            s.assert_on_grid()
        s.assert_on_grid()  # the flag was reset, the list emptied
        s.record_window(*window_of(2, 2, 23))
        s.assert_on_grid()
        worse = list(window_of(2, 2, 24, deaths=((0, 0, "trunc"),)))
        worse[5][0, 0, 0, 0] = 0.5  # a final observation counts too
        s.record_window(*worse)
        s.end_collect(keep_open=False)  # env 0's new episode is dropped
        with pytest.raises(ValueError, match=r"episodes \[1, 2\] \(and 1 not stored\): .*not on the uint8 grid"):
            s.assert_on_grid()
        with pytest.raises(ValueError, match="3 final observations for the window's 1 deaths"):
            s.record_window(*window_of(2, 2, 25, deaths=((0, 0, "end"),))[:5], torch.zeros((3,) + FRAME))


def test_counters_follow_add_episode_and_its_replacement():
    from diamond_amd.replay import DeviceReplay

    def ep(rew, end):
        n = len(rew)
        return SimpleNamespace(obs=torch.zeros((n,) + FRAME, dtype=torch.uint8), act=torch.zeros(n, dtype=torch.long), rew=torch.tensor(rew),
                               end=torch.tensor(end, dtype=torch.uint8), trunc=torch.zeros(n, dtype=torch.uint8), info={})

    with engine_on_interpreter():
        s = DeviceReplay("cpu")
        s.add_episode(ep([-1.0, 0.0, 2.5], [0, 0, 1]))
        s.add_episode(ep([0.0, 0.0], [0, 0]))
        assert (s.counts_rew, s.counts_end) == ([1, 3, 1], [4, 1])
        assert s.counter_rew[-1.0] == 1 and s.counter_rew[1] == 1 and s.counter_end[1] == 1
        s.add_episode(ep([0.0, 0.0, 3.0, -2.0, -0.5], [0, 0, 0, 0, 0]), episode_id=1)  # the collector's re-add of a grown episode
        assert (s.counts_rew, s.counts_end) == ([3, 3, 2], [7, 1])
        s.add_episode(ep([1.0], [1]), episode_id=0)
        assert (s.counts_rew, s.counts_end) == ([2, 2, 2], [5, 1]) and s.num_steps == 6
        s.record_window(*window_of(1, 2, 5))
        s.end_collect(keep_open=True)
        with pytest.raises(ValueError, match="episode 2: record_window is still writing it"):
            s.add_episode(ep([1.0], [1]), episode_id=2)


def test_make_env_loop_kind_overrides_the_environment_variable(monkeypatch):
    from diamond_amd.env_loop import make_env_loop

    monkeypatch.setenv("DIAMOND_ENV_LOOP", "neither")
    with engine_on_interpreter():
        loop = make_env_loop(CC.ScriptedEnv(2), CC.ScriptedPolicy(), kind="sequential")
        out = loop.send(3)
        assert out[0].shape == (2, 3) + FRAME and len(out[-1]) == 3
        with pytest.raises(AssertionError, match="neither"):
            make_env_loop(CC.ScriptedEnv(2), CC.ScriptedPolicy()).send(1)
