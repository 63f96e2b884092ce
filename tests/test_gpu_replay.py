"""The device-resident replay store on the GPU (`-m gpu`): dmd_segment_gather bit for bit against the numpy restatement of
tests/replay_cases.py (eagerly and replayed from a captured graph whose descriptor changes), and gathered batches through the
unchanged consumers: RewEndModel.forward, graphed_rew_end_step (fed three ways) and WorldModelEnv."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import replay_cases as RC
from tests.conftest import WEIGHT_SEED

DEV = "cuda"
pytestmark = pytest.mark.gpu

_NP_FLAG = {torch.uint8: np.uint8, torch.int64: np.int64}
_POISON = {torch.float32: float("nan"), torch.int64: 0x5A5A5A5A, torch.uint8: 0x5A, torch.bool: True}


def _store_of(arena, frame_shape, flag_dtype):
    """The arena of tests/replay_cases.py as a DeviceReplay: its episodes added in order land at the same arena rows and final
    rows, so the descriptor rows of replay_cases.all_segments describe the store as they describe the numpy arena."""
    from diamond_amd.replay import DeviceReplay

    store = DeviceReplay(DEV, frame_shape=frame_shape)
    for f, n, r in zip(arena["first"], arena["len"], arena["final_row"]):
        sl = slice(f, f + n)
        info = {} if r < 0 else {"final_observation": torch.from_numpy(arena["finals"][r]).reshape(frame_shape)}
        store.add_episode(SimpleNamespace(obs=torch.from_numpy(arena["frames"][sl]).reshape((n,) + tuple(frame_shape)), act=torch.from_numpy(arena["act"][sl]),
                                          rew=torch.from_numpy(arena["rew"][sl]), end=torch.from_numpy(arena["end"][sl]).to(flag_dtype),
                                          trunc=torch.from_numpy(arena["trunc"][sl]).to(flag_dtype), info=info))
    assert store._first.tolist() == arena["first"].tolist() and store._final_row.tolist() == arena["final_row"].tolist()
    assert store.wasted_frames == 0
    return store


def _outputs(b, t, pf, flag_dtype, skip=()):
    shapes = {"obs": ((b, t, pf), torch.float32), "act": ((b, t), torch.int64), "rew": ((b, t), torch.float32), "end": ((b, t), flag_dtype),
              "trunc": ((b, t), flag_dtype), "mask_padding": ((b, t), torch.uint8), "final_obs": ((b, pf), torch.float32)}
    return {k: torch.empty(s, dtype=d, device=DEV) for k, (s, d) in shapes.items() if k not in skip}


def _poison(out):
    for v in out.values():
        v.fill_(_POISON[v.dtype])


def _to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("put_back", [False, True])
@pytest.mark.parametrize("flag_dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("t", RC.SEQ_LENGTHS)
@pytest.mark.parametrize("per_frame", RC.PER_FRAMES)
def test_segment_gather_matches_the_restatement_eager_and_replayed(per_frame, t, flag_dtype, put_back):
    """The cases of tests/test_replay_simt.py on the device: eager launches for every batch (B = 1, 37 and a shorter last one);
    then ONE captured gather_static of B = 37 replayed for each full batch after the descriptor's contents were overwritten
    (a linear graph: one kernel node).  Outputs are re-poisoned with NaN before every launch."""
    arena = RC.make_arena(per_frame, seed=per_frame + t)
    store = _store_of(arena, (per_frame,), flag_dtype)
    npf = _NP_FLAG[flag_dtype]
    full = []
    for i, seg in enumerate(RC.batches(RC.all_segments(arena, t))):
        out = _outputs(len(seg), t, per_frame, flag_dtype)
        _poison(out)
        store.gather_static(torch.from_numpy(seg).to(DEV), out, put_back_final=put_back)
        RC.assert_same(_to_numpy(out), RC.restate(arena, seg, t, npf, put_back), RC.OUTPUTS, f"eager batch {i} (B = {len(seg)})")
        if len(seg) == 37:
            full.append(seg)
    assert len(full) >= 3
    seg_dev = torch.from_numpy(full[0]).to(DEV)
    out = _outputs(37, t, per_frame, flag_dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        store.gather_static(seg_dev, out, put_back_final=put_back)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    generation = store.generation
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        store.gather_static(seg_dev, out, put_back_final=put_back)
    for i, seg in enumerate(full[1:] + full[:1]):
        seg_dev.copy_(torch.from_numpy(seg))
        _poison(out)
        graph.replay()
        RC.assert_same(_to_numpy(out), RC.restate(arena, seg, t, npf, put_back), RC.OUTPUTS, f"replay {i}")
    assert store.generation == generation


@pytest.mark.parametrize("skip", [("obs",), ("final_obs",), ("act", "rew", "end", "trunc", "mask_padding"), ("obs", "final_obs", "trunc")])
def test_segment_gather_null_outputs(skip):
    arena = RC.make_arena(108, seed=9)
    store = _store_of(arena, (3, 6, 6), torch.int64)
    seg = np.ascontiguousarray(RC.all_segments(arena, 5)[::3])
    out = _outputs(len(seg), 5, 108, torch.int64, skip=skip)
    _poison(out)
    store.gather_static(torch.from_numpy(seg).to(DEV), out, put_back_final=True)
    RC.assert_same(_to_numpy(out), RC.restate(arena, seg, 5, np.int64, True), tuple(k for k in RC.OUTPUTS if k not in skip), f"without {skip}")


def test_segment_gather_dequantises_all_256_levels_like_the_division():
    """q / 255 is formed as a multiplication plus one residual step: every level must give the bits of the fp32 division."""
    arena = RC.levels_arena()
    store = _store_of(arena, (256,), torch.uint8)
    seg = np.ascontiguousarray(RC.all_segments(arena, 5)[::4])
    out = _outputs(len(seg), 5, 256, torch.uint8)
    _poison(out)
    store.gather_static(torch.from_numpy(seg).to(DEV), out, put_back_final=True)
    RC.assert_same(_to_numpy(out), RC.restate(arena, seg, 5, np.uint8, True), RC.OUTPUTS, "all levels")
    assert int(out["obs"].unique().numel()) == 257


def test_segment_gather_unaligned_output_takes_the_scalar_path():
    arena = RC.make_arena(192, seed=1)
    store = _store_of(arena, (192,), torch.uint8)
    seg = np.ascontiguousarray(RC.all_segments(arena, 5)[::2])
    b = len(seg)
    big = torch.full((b * 5 * 192 + 1,), float("nan"), device=DEV)
    out = _outputs(b, 5, 192, torch.uint8, skip=("obs",))
    _poison(out)
    out["obs"] = big[1:].view(b, 5, 192)
    assert out["obs"].data_ptr() % 16 == 4
    store.gather_static(torch.from_numpy(seg).to(DEV), out, put_back_final=True)
    assert bool(big[0].isnan())  # the element in front of the output was not touched
    RC.assert_same(_to_numpy(out), RC.restate(arena, seg, 5, np.uint8, True), RC.OUTPUTS, "misaligned obs")


# ---------------------------------------------------------------------------------------------------------------------------
# gathered batches through the consumers (3 x 64 x 64 frames, int64 end / trunc as the losses need them)
# ---------------------------------------------------------------------------------------------------------------------------
FRAME = (3, 64, 64)
# (first, start, len, final_row) is looked up per episode below; T = 6:
#   episode 2 (7 steps, ends):     steps 3 .. 8, the end INSIDE a right-padded segment (position 4 takes the final observation)
#   episode 3 (30 steps, neither): unpadded;   episode 5 (30 steps, ends): left-padded;   episode 4 (7 steps, trunc only): right-padded
IDS_A = [(2, 3, 9), (3, 10, 16), (5, -2, 4), (4, 4, 10)]
IDS_B = [(5, 26, 32), (2, -1, 5), (0, -2, 4), (3, 24, 30)]  # ends at positions 3 (episode 5) and 2 (episode 0, one step long)


@pytest.fixture(scope="module")
def frames_store():
    arena = RC.make_arena(int(np.prod(FRAME)), seed=77)
    arena["act"] %= 4  # the default agent has 4 actions
    return arena, _store_of(arena, FRAME, torch.int64)


@pytest.fixture(scope="module")
def agent():
    import diamond_amd as D
    from diamond_amd.testing import fill_module_

    a = D.Agent(D.default_agent_config())
    fill_module_(a, WEIGHT_SEED)
    return a.to(DEV).eval()


def _seg_rows(arena, ids):
    return np.array([(arena["first"][e], s, arena["len"][e], arena["final_row"][e]) for e, s, _ in ids], np.int64)


def _uploaded(arena, ids):
    """The batch as the CPU pipeline would deliver it: built on the host by the restatement (no final observation put back: that is
    the consumer's job, from `info`), then uploaded."""
    t = ids[0][2] - ids[0][1]
    seg = _seg_rows(arena, ids)
    r = RC.restate(arena, seg, t, np.int64, False)
    info = [{} if row < 0 else {"final_observation": torch.from_numpy(r["final_obs"][i]).reshape(FRAME).to(DEV)} for i, row in enumerate(seg[:, 3])]
    return SimpleNamespace(obs=torch.from_numpy(r["obs"]).reshape((len(ids), t) + FRAME).to(DEV), act=torch.from_numpy(r["act"]).to(DEV),
                           rew=torch.from_numpy(r["rew"]).to(DEV), end=torch.from_numpy(r["end"]).to(DEV), trunc=torch.from_numpy(r["trunc"]).to(DEV),
                           mask_padding=torch.from_numpy(r["mask_padding"]).bool().to(DEV), info=info, segment_ids=None)


def test_rew_end_forward_on_a_gathered_batch_is_the_uploaded_batch(frames_store, agent):
    arena, store = frames_store
    m = agent.rew_end_model.train()
    results = []
    for batch in (_uploaded(arena, IDS_A), store.gather(IDS_A)):
        assert bool(batch.end[0, :-1].any()) and not bool(batch.mask_padding[0, 4:].any())  # the end inside the padded segment
        before = batch.obs[0, 4].clone()
        m.zero_grad(set_to_none=True)
        loss, logs = m(batch)
        loss.backward()
        assert not torch.equal(batch.obs[0, 4], before) and torch.equal(batch.obs[0, 4], batch.info[0]["final_observation"])
        results.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()},
                        {k: v.clone() for k, v in logs["confusion_matrix"].items()}, batch.obs.clone()))
    (l0, g0, c0, o0), (l1, g1, c1, o1) = results
    assert torch.isfinite(l0) and torch.equal(l0, l1) and torch.equal(o0, o1)
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0), [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert all(torch.equal(c0[k], c1[k]) for k in c0)
    m.zero_grad(set_to_none=True)
    agent.eval()


def test_graphed_rew_end_step_fed_three_ways(frames_store, agent):
    """The uploaded batch, a gathered batch, and a batch gathered STRAIGHT INTO the step's static buffers (put_back_final in the
    kernel, no `info`: the step's stage finds nothing to do and its `copy_` of each field onto itself is skipped): the same loss
    bits at each of two steps and the same parameters after them."""
    from diamond_amd.rew_end_model import RewEndModel
    from diamond_amd.train_graph import graphed_rew_end_step

    arena, store = frames_store
    init = copy.deepcopy(agent.rew_end_model.state_dict())
    outcomes = []
    for way in ("uploaded", "gathered", "static"):
        m = RewEndModel(agent.rew_end_model.cfg)
        m.load_state_dict(init)
        m = m.to(DEV).train()
        opt = torch.optim.AdamW(m.parameters(), lr=3e-4, capturable=True)
        make = (lambda ids: _uploaded(arena, ids)) if way == "uploaded" else (lambda ids: store.gather(ids))
        step = graphed_rew_end_step(m, opt, 100.0, make(IDS_A), warmup_steps=1)
        losses = []
        for ids in (IDS_B, IDS_A):
            if way == "static":
                batch = store.gather(ids, out=step.static, put_back_final=True, info=False)
                assert all(getattr(batch, k) is step.static[k] for k in step.static) and batch.info == [{}] * 4
            else:
                batch = make(ids)
            loss, _ = step(batch)
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        outcomes.append((losses, {k: p.detach().clone() for k, p in m.named_parameters()}))
    (la, pa), rest = outcomes[0], outcomes[1:]
    assert all(torch.isfinite(x) for x in la) and not torch.equal(la[0], la[1])
    assert max(float((pa[k] - init[k].to(DEV)).abs().max()) for k in pa) > 1e-5, "parameters did not train"
    for way, (lb, pb) in zip(("gathered", "static"), rest):
        assert all(torch.equal(a, b) for a, b in zip(la, lb)), (way, la, lb)
        assert all(torch.equal(pa[k], pb[k]) for k in pa), (way, [k for k in pa if not torch.equal(pa[k], pb[k])])


class _ListLoader:
    def __init__(self, batch_size, batches):
        self.batch_sampler = SimpleNamespace(batch_size=batch_size)
        self._batches = batches

    def __iter__(self):
        return iter(self._batches)


def test_world_model_env_from_a_device_segment_loader(frames_store, agent, monkeypatch):
    """reset() and the first step of a WorldModelEnv fed by a DeviceSegmentLoader against one fed by a list-backed loader that
    yields the same batches (the pool's no-torch-draws guard armed): observations and the reward / end state are bit-identical."""
    import diamond_amd as D
    from diamond_amd.replay import DeviceSegmentLoader

    monkeypatch.setenv("DIAMOND_CHECK_RESET_RNG", "1")
    _, store = frames_store
    b, t = 3, 4
    recorded = []
    twin = DeviceSegmentLoader(store, b, t, rng=np.random.RandomState(3))
    for _ in range(8):
        x = next(twin)
        recorded.append(SimpleNamespace(obs=x.obs.clone(), act=x.act.clone(), mask_padding=x.mask_padding.clone()))
    assert any(not bool(x.mask_padding.all()) for x in recorded[:2])  # the preloaded rounds hold left-padded segments
    cfg = D.WorldModelEnvConfig(horizon=3, num_batches_to_preload=2, diffusion_sampler=D.DiffusionSamplerConfig(num_steps_denoising=1))
    seen = []
    for loader in (DeviceSegmentLoader(store, b, t, rng=np.random.RandomState(3)), _ListLoader(b, recorded)):
        env = D.WorldModelEnv(agent.denoiser, agent.rew_end_model, loader, cfg)
        torch.manual_seed(11)
        obs0, _ = env.reset()
        act = torch.tensor([1, 3, 0], device=DEV)
        obs1, rew, end, trunc, _ = env.step(act)
        seen.append([v.clone() for v in (obs0, obs1, rew, end, trunc, env.hx_rew_end, env.cx_rew_end, env.obs_buffer, env.act_buffer)])
    assert env.pool.frames_u8 is not None, "the gathered frames are on the uint8 grid: the pool keeps them as levels"
    for i, (x, y) in enumerate(zip(*seen)):
        assert torch.equal(x, y), i
