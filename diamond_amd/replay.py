"""Device-resident replay store: the training data next to the kernels, a batch per launch.

The reference keeps episodes as fp32 tensors in host RAM and builds every batch on the CPU: `Dataset.__getitem__` ->
`make_segment` per sample (data/dataset.py:47-49, data/utils.py:18-41), `collate_segments_to_batch` per batch (:12-15), then an
fp32 upload (31 MB for a reward/end batch of 32 x 20 frames of 3 x 64 x 64).  Here the episodes live on the GPU as the uint8
levels they have on disk (data/episode.py:36-50) in one ARENA -- the episodes' steps back to back -- and a whole (B, T) batch,
padding, `mask_padding` and final observations included, is ONE `dmd_segment_gather` launch; per batch the host handles B
segment ids (a (B, 4) int64 descriptor), never a frame.  100k frames of 3 x 64 x 64 are 1.2 GB.

    store = DeviceReplay(device)
    for episode in dataset_episodes: store.add_episode(episode)          # or DeviceReplay.from_episodes(...)
    loader = DeviceSegmentLoader(store, batch_size, seq_length)          # where a torch DataLoader over the Dataset went
    batch = next(iter(loader))                                           # Batch: obs, act, rew, end, trunc, mask_padding, info, segment_ids

What is mirrored is the reference's DATA CONTRACT: `sample_ids` makes the numpy calls of `BatchSampler.sample`
(data/batch_sampler.py:38-70) in its order, so a shared numpy seed gives the same segment ids; `gather` gives the fields of
`collate_segments_to_batch` bit for bit and dtype for dtype; `traverse` gives the batches of `DatasetTraverser` (data/utils.py:44-82).

The store fills itself from the env loop: `record_window` writes a window of env steps -- the loop's stacked device tensors -- into
the arena in ONE `dmd_record_window` launch (the host handles B x T scalars, never a frame; diamond_amd/collector.py drives it
with the reference collector's protocol), keeps the `counts_rew` / `counts_end` of the reference's Dataset, and `load_episode`
gives an episode back with the fields of the reference's `Episode.load`: persistence is `dataset.add_episode(store.load_episode(i))`.
There is no CPU path: the arena lives where the kernels run.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import Counter
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import native as nv

_FLAG_DTYPES = (torch.uint8, torch.int64)
_SMALL = ("act", "rew", "end", "trunc", "mask_padding")


@dataclass
class SegmentId:
    episode_id: int
    start: int
    stop: int


@dataclass
class Batch:
    """The reference's batch (data/batch.py): tensors (B, T, ...) plus the per-sample `info` dicts and segment ids."""
    obs: Tensor
    act: Tensor
    rew: Tensor
    end: Tensor
    trunc: Tensor
    mask_padding: Tensor
    info: List[Dict[str, Any]]
    segment_ids: List[SegmentId]

    def _map(self, fn) -> "Batch":
        return Batch(**{k: (v if k in ("info", "segment_ids") else fn(v)) for k, v in self.__dict__.items()})

    def pin_memory(self) -> "Batch":
        return self._map(lambda v: v.pin_memory())

    def to(self, device) -> "Batch":
        return self._map(lambda v: v.to(device))


@dataclass
class Episode:
    """What `load_episode` returns: the fields and dtypes of the reference's Episode (data/episode.py), wherever the store lives."""
    obs: Tensor
    act: Tensor
    rew: Tensor
    end: Tensor
    trunc: Tensor
    info: Dict[str, Any]

    def __len__(self) -> int:
        return int(self.obs.shape[0])

    def to(self, device) -> "Episode":
        return Episode(**{k: (v.to(device) if k != "info" else {a: b.to(device) for a, b in v.items()}) for k, v in self.__dict__.items()})

    def compute_metrics(self) -> Dict[str, Any]:
        return {"length": len(self), "return": self.rew.sum().item()}

    def save(self, path) -> None:
        """The file the reference's Episode.load reads (data/episode.py:36-50): obs as uint8 levels, the rest as it is."""
        import os

        d = {k: (v.add(1).div(2).mul(255).round().byte() if k == "obs" else v) for k, v in self.to("cpu").__dict__.items()}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(d, str(path) + ".tmp")
        os.replace(str(path) + ".tmp", str(path))


@dataclass
class _OpenEpisode:
    """An episode `record_window` is still writing: its slot in the arena and what the host accumulates about it."""
    first: int = 0
    slot: int = 0      # arena rows reserved at `first`
    n: int = 0         # rows written
    eid: Optional[int] = None  # None until it is stored (at its death, or when a collect that keeps its open episodes ends)
    ret: float = 0.0   # sum of the rewards, fp64
    counts: np.ndarray = field(default_factory=lambda: np.zeros(5, np.int64))  # rewards < 0, == 0, > 0; end == 0, != 0
    final_row: int = -1


def _reward_end_counts(rew: np.ndarray, end: np.ndarray) -> np.ndarray:
    end = end != 0
    return np.array([(rew < 0).sum(), (rew == 0).sum(), (rew > 0).sum(), (~end).sum(), end.sum()], dtype=np.int64)


def _id_fields(i) -> Tuple[int, int, int]:
    if hasattr(i, "episode_id"):
        return int(i.episode_id), int(i.start), int(i.stop)
    e, a, b = i
    return int(e), int(a), int(b)


class DeviceReplay:
    def __init__(self, device, frame_shape: Optional[Sequence[int]] = None, capacity_frames: int = 0, name: Optional[str] = None,
                 strict_grid: bool = True) -> None:
        self.device = torch.device(device)
        # record_window stores the NEAREST level of every value.  Frames of a real env are on the grid and storing them loses
        # nothing: anything else is an error there (strict_grid).  Imagined frames (WorldModelEnv) leave the sampler's last Euler
        # step a few ulps off the level the denoiser quantised them to: a store that records them is built with strict_grid=False
        # and rounds them back, as saving them to disk would; `saw_off_grid` then says that it happened.
        self.strict_grid = bool(strict_grid)
        self.saw_off_grid = False
        self.name = name if name is not None else "dataset"  # the prefix of the collector's log keys
        self.frame_shape: Optional[Tuple[int, ...]] = None if frame_shape is None else tuple(int(s) for s in frame_shape)
        self.flag_dtype: Optional[torch.dtype] = None  # dtype of end / trunc, remembered from the first episode
        self.generation = 0     # arena reallocations (growth, reserve, compact): pointers recorded in a hipGraph are void after one
        self._capacity = 0
        self.frames = self.act = self.rew = self.end = self.trunc = self.finals = None
        self._off_grid: Optional[Tensor] = None        # the deferred flag of record_window's launches (assert_on_grid reads it)
        self._reset()
        self._want = int(capacity_frames)
        if self.frame_shape is not None and self._want > 0:
            self.reserve(self._want)

    def _reset(self) -> None:
        self.wasted_frames = 0  # arena rows of slots abandoned by replaced, moved or dropped episodes (compact() reclaims them)
        self.num_episodes = 0
        self.num_steps = 0
        self.lengths = np.array([], dtype=np.int64)    # per episode, as in the reference's Dataset
        self.start_idx = np.array([], dtype=np.int64)  # cumulative steps before each episode (the reference's bookkeeping)
        self.counter_rew: Counter = Counter()          # sign of the reward -> steps, end -> steps (data/dataset.py:108-112)
        self.counter_end: Counter = Counter()
        self._ep_counts = np.zeros((0, 5), dtype=np.int64)  # per episode: rewards < 0, == 0, > 0; end == 0, != 0
        self._first = np.array([], dtype=np.int64)     # arena row of each episode's step 0
        self._slot = np.array([], dtype=np.int64)      # arena rows the episode's slot holds (>= its length)
        self._final_row = np.array([], dtype=np.int64)  # row of `finals`, or -1
        self._used = 0        # arena rows handed out
        self._finals_used = 0
        self._open: Dict[int, _OpenEpisode] = {}       # env index -> the episode record_window is writing for it
        self._unchecked: List[_OpenEpisode] = []       # episodes written since assert_on_grid last read the flag

    def clear(self) -> None:
        """Forget every episode, open ones included (the reference's Dataset.clear); the arena keeps its allocation, so
        `generation` does not change."""
        if self._unchecked:
            self.assert_on_grid()
        self._reset()

    # -- bookkeeping -------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_episodes(cls, episodes: Iterable[Any], device=None, **kwargs: Any) -> "DeviceReplay":
        store = cls(device if device is not None else "cuda", **kwargs)
        for ep in episodes:
            store.add_episode(ep)
        return store

    @property
    def per_frame(self) -> int:
        return int(np.prod(self.frame_shape))

    @property
    def nbytes(self) -> int:
        """Bytes resident on the device."""
        ts = (self.frames, self.act, self.rew, self.end, self.trunc, self.finals)
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def __len__(self) -> int:
        return self.num_steps

    @property
    def counts_rew(self) -> List[int]:
        return [self.counter_rew[r] for r in (-1, 0, 1)]

    @property
    def counts_end(self) -> List[int]:
        return [self.counter_end[e] for e in (0, 1)]

    def _count(self, delta: np.ndarray) -> None:
        for key, v in zip((-1.0, 0.0, 1.0), delta[:3]):
            self.counter_rew[key] += int(v)
        for key, v in zip((0, 1), delta[3:]):
            self.counter_end[key] += int(v)

    def _alloc(self, rows: int) -> Dict[str, Tensor]:
        d = self.device
        return {"frames": torch.empty((rows, self.per_frame), dtype=torch.uint8, device=d),
                "act": torch.empty(rows, dtype=torch.int64, device=d), "rew": torch.empty(rows, dtype=torch.float32, device=d),
                "end": torch.empty(rows, dtype=torch.uint8, device=d), "trunc": torch.empty(rows, dtype=torch.uint8, device=d)}

    def reserve(self, n_frames: int, n_finals: int = 0) -> None:
        """Room for `n_frames` arena rows in all (at least double the present capacity when it grows: one device copy per
        array, amortised over the episodes) and for the final observations of `n_finals` episodes."""
        assert self.frame_shape is not None, "reserve: the frame shape is not known yet (pass frame_shape, or add an episode)"
        self._reserve_finals(int(n_finals))
        if n_frames <= self._capacity:
            return
        rows = max(int(n_frames), 2 * self._capacity)
        new = self._alloc(rows)
        for k, t in new.items():
            if self._used:
                t[: self._used].copy_(getattr(self, k)[: self._used])
            setattr(self, k, t)
        self._capacity = rows
        self.generation += 1

    def _reserve_finals(self, rows: int) -> None:
        have = 0 if self.finals is None else self.finals.shape[0]
        if rows <= have:
            return
        new = torch.empty((max(rows, 2 * have, 4), self.per_frame), dtype=torch.uint8, device=self.device)
        if self._finals_used:
            new[: self._finals_used].copy_(self.finals[: self._finals_used])
        self.finals = new
        self.generation += 1

    def _levels(self, x: Tensor, what: str) -> Tensor:
        """(n, per_frame) uint8 levels on the device of uint8 frames, or of fp32 frames in [-1, 1] ON the 256-level grid."""
        x = x.to(self.device)
        if x.dtype == torch.uint8:
            return x.reshape(-1, self.per_frame)
        if x.dtype != torch.float32:
            raise ValueError(f"{what}: frames are uint8 levels or float32 in [-1, 1], not {x.dtype}")
        x = x.contiguous()
        q = torch.empty(x.shape, dtype=torch.uint8, device=self.device)
        off_grid = torch.zeros(1, dtype=torch.int32, device=self.device)
        if x.numel():
            nv.check(nv.lib().dmd_quantize_u8(nv.fptr(x), nv.ptr(q), nv.ptr(off_grid), x.numel(), nv.stream()), "dmd_quantize_u8")
        if int(off_grid.item()) != 0:  # (the one read-back: adding an episode may synchronise, sampling and gathering never do)
            raise ValueError(f"{what}: fp32 frames are not on the uint8 grid ((level / 255) * 2 - 1): storing them as levels would "
                             "change them")
        return q.reshape(-1, self.per_frame)

    def add_episode(self, episode: Any, *, episode_id: Optional[int] = None) -> int:
        """Append an episode (anything with obs / act / rew / end / trunc / info), or -- with `episode_id`, as the reference's
        collector does for an episode that is still growing (data/dataset.py:90-120) -- replace one: in place when it is the
        arena's last episode or still fits its slot, else at the arena's end, the old slot counted in `wasted_frames`.
        `counter_rew` / `counter_end` follow as the reference's: a replaced episode's steps are taken out first."""
        eid = self.num_episodes if episode_id is None else int(episode_id)
        what = f"episode {eid}"
        assert episode_id is None or 0 <= eid < self.num_episodes, f"{what}: no such episode ({self.num_episodes} stored)"
        if episode_id is not None and any(r.eid == eid for r in self._open.values()):
            raise ValueError(f"{what}: record_window is still writing it (end_collect(keep_open=False) lets go of it)")
        obs = episode.obs
        n = int(obs.shape[0])
        if n < 1:
            raise ValueError(f"{what}: empty")
        if self.frame_shape is None:
            self.frame_shape = tuple(int(s) for s in obs.shape[1:])
        if tuple(obs.shape[1:]) != self.frame_shape:
            raise ValueError(f"{what}: frames of shape {tuple(obs.shape[1:])}, the store holds {self.frame_shape}")
        flag_dtype = episode.end.dtype
        if self.flag_dtype is None:
            if flag_dtype not in _FLAG_DTYPES or episode.trunc.dtype != flag_dtype:
                raise ValueError(f"{what}: end / trunc are {flag_dtype} / {episode.trunc.dtype}; uint8 or int64, both the same")
            self.flag_dtype = flag_dtype
        levels = self._levels(obs, what)
        info = getattr(episode, "info", None) or {}
        final = info.get("final_observation")
        if final is not None:
            if tuple(final.shape[-len(self.frame_shape):]) != self.frame_shape or final.numel() != self.per_frame:
                raise ValueError(f"{what}: final_observation of shape {tuple(final.shape)}, frames are {self.frame_shape}")
            final = self._levels(final, f"{what}: final_observation")
        if self._capacity == 0 and self._want > 0:
            self.reserve(self._want)
        counts = _reward_end_counts(episode.rew.detach().to("cpu", torch.float32).numpy(), episode.end.detach().cpu().numpy())

        if episode_id is None:
            self._ep_counts = np.concatenate((self._ep_counts, counts[None]))
            self._count(counts)
            first = self._used
            self.reserve(first + n)
            self._used = first + n
            self.start_idx = np.concatenate((self.start_idx, np.array([self.num_steps], dtype=np.int64)))
            self.lengths = np.concatenate((self.lengths, np.array([n], dtype=np.int64)))
            self._first = np.concatenate((self._first, np.array([first], dtype=np.int64)))
            self._slot = np.concatenate((self._slot, np.array([n], dtype=np.int64)))
            self._final_row = np.concatenate((self._final_row, np.array([-1], dtype=np.int64)))
            self.num_steps += n
            self.num_episodes += 1
        else:
            self._count(counts - self._ep_counts[eid])
            self._ep_counts[eid] = counts
            first, slot = int(self._first[eid]), int(self._slot[eid])
            if first + slot == self._used:  # the arena's last episode: its slot grows (or shrinks) where it is
                self.reserve(first + n)
                self._used = first + n
                self._slot[eid] = n
            elif n > slot:  # does not fit: to the arena's end, the old slot is a hole until compact()
                self.wasted_frames += slot
                first = self._used
                self.reserve(first + n)
                self._used = first + n
                self._first[eid], self._slot[eid] = first, n
            grown = n - int(self.lengths[eid])
            self.lengths[eid] = n
            self.start_idx[eid + 1:] += grown
            self.num_steps += grown

        self.frames[first:first + n].copy_(levels)
        self.act[first:first + n].copy_(episode.act.to(self.device).to(torch.int64))
        self.rew[first:first + n].copy_(episode.rew.to(self.device).to(torch.float32))
        self.end[first:first + n].copy_(episode.end.to(self.device).to(torch.uint8))
        self.trunc[first:first + n].copy_(episode.trunc.to(self.device).to(torch.uint8))
        if final is None:
            self._final_row[eid] = -1
        else:
            row = int(self._final_row[eid])
            if row < 0:
                row = self._finals_used
                self._reserve_finals(row + 1)
                self._finals_used = row + 1
                self._final_row[eid] = row
            self.finals[row].copy_(final[0])
        return eid

    def compact(self) -> None:
        """Rebuild the arena without holes: the episodes back to back in id order (one device gather per array)."""
        # (an episode record_window is still writing keeps every row written so far, stored or not; the ones without an id
        #  follow the stored episodes.  Slots shrink to what they hold: an open episode grows again at its next window.)
        writing = {r.eid: r for r in self._open.values() if r.eid is not None}
        spans = [(writing[e].first, writing[e].n) if e in writing else (int(self._first[e]), int(self.lengths[e])) for e in range(self.num_episodes)]
        unstored = [r for _, r in sorted(self._open.items()) if r.eid is None]
        spans += [(r.first, r.n) for r in unstored]
        if not spans:
            return
        rows = np.concatenate([np.arange(f, f + n, dtype=np.int64) for f, n in spans])
        idx = torch.from_numpy(rows).to(self.device)
        new = self._alloc(max(self._capacity, len(rows)))
        for k, t in new.items():
            torch.index_select(getattr(self, k), 0, idx, out=t[: len(rows)])
            setattr(self, k, t)
        self._capacity = new["act"].shape[0]
        held = np.array([n for _, n in spans], dtype=np.int64)
        at = np.concatenate(([0], np.cumsum(held)[:-1])).astype(np.int64)
        self._first = at[: self.num_episodes].copy()
        self._slot = held[: self.num_episodes].copy()
        for r, f in zip([writing.get(e) for e in range(self.num_episodes)] + unstored, at):
            if r is not None:
                r.first, r.slot = int(f), r.n
        self._used = len(rows)
        self.wasted_frames = 0
        keep = np.flatnonzero(self._final_row >= 0)
        if self.finals is not None and len(keep) != self._finals_used:  # final observations whose episode no longer has one
            if len(keep):
                self.finals = self.finals.index_select(0, torch.from_numpy(self._final_row[keep]).to(self.device))
            self._final_row[keep] = np.arange(len(keep), dtype=np.int64)
            self._finals_used = len(keep)
        self.generation += 1

    # -- collection: windows of env steps straight from the env loop -------------------------------------------------------------
    def _store(self, r: _OpenEpisode) -> int:
        """Give an episode that record_window wrote its id, or bring the stored one up to the rows written since."""
        if r.eid is None:
            r.eid = self.num_episodes
            self.start_idx = np.concatenate((self.start_idx, np.array([self.num_steps], dtype=np.int64)))
            self.lengths = np.concatenate((self.lengths, np.array([r.n], dtype=np.int64)))
            self._first = np.concatenate((self._first, np.array([r.first], dtype=np.int64)))
            self._slot = np.concatenate((self._slot, np.array([r.slot], dtype=np.int64)))
            self._final_row = np.concatenate((self._final_row, np.array([r.final_row], dtype=np.int64)))
            self._ep_counts = np.concatenate((self._ep_counts, r.counts[None]))
            self._count(r.counts)
            self.num_steps += r.n
            self.num_episodes += 1
        else:
            e = r.eid
            grown = r.n - int(self.lengths[e])
            self.lengths[e] = r.n
            self.start_idx[e + 1:] += grown
            self.num_steps += grown
            self._first[e], self._slot[e], self._final_row[e] = r.first, r.slot, r.final_row
            self._count(r.counts - self._ep_counts[e])
            self._ep_counts[e] = r.counts
        return r.eid

    def record_window(self, obs: Tensor, act: Tensor, rew: Tensor, end: Tensor, trunc: Tensor, final_observation=None, *,
                      store_open_if_episodes: Optional[int] = None) -> List[Dict[str, Any]]:
        """A window of env steps -- the env loop's stacked device tensors: obs (B, T, C, H, W) fp32 on the uint8 grid, act / rew /
        end / trunc (B, T) -- into the arena in ONE `dmd_record_window` launch.  Env b owns one open episode of the store across
        calls: its steps are cut at `end | trunc`, the open episode is extended, new ones are opened behind each death.
        final_observation: the step infos' (n_dead, C, H, W) tensors in order of death (steps first, ascending env index within a
        step), as one tensor or a sequence of them; None: the episodes that end here have no final observation.
        The host reads back rew / end / trunc once (B x T x 6 bytes) and never a frame; the call does not wait for its own launch:
        whether the frames were on the grid is `assert_on_grid()`'s to say, later.
        An open episode's slot holds twice what the episode needs when it grows: in place when it is the arena's last, else one
        device-side move of its rows to the arena's end in the same launch, the old slot counted in `wasted_frames`; `generation`
        changes only when the arena reallocates (add_episode's contract: reserve() first under a captured graph).
        An episode is STORED -- it gets its id, counts in num_steps / lengths / counts_rew / counts_end, can be sampled -- when it
        ends, or at `end_collect(keep_open=True)`, as the reference's collector adds an episode to its Dataset
        (coroutines/collector.py:68-77); ids go by death (steps first, then env index).  store_open_if_episodes = k: when at
        least k episodes end in this window (0: always) the collect ends with the window's last step, and the episodes still
        open are stored at that step in env order TOGETHER with its deaths -- the reference's order of ids at a collect's last step.
        Returns, per episode that ended in this window in that order, {"episode_id", "length", "return"}: the return is summed on
        the host in fp64 over the whole episode, which equals the reference's fp32 `rew.sum()` wherever that sum is exact
        (integer rewards, as the reference's sign-clipped ones, up to 2^24 in magnitude)."""
        nv.check_current_device(self.device)
        if obs.dim() < 3 or obs.dtype != torch.float32:
            raise ValueError(f"record_window: obs is {tuple(obs.shape)} {obs.dtype}; (B, T, ...) float32 frames in [-1, 1] on the uint8 grid")
        b, t = int(obs.shape[0]), int(obs.shape[1])
        if self.frame_shape is None:
            self.frame_shape = tuple(int(s) for s in obs.shape[2:])
        if tuple(obs.shape[2:]) != self.frame_shape:
            raise ValueError(f"record_window: frames of shape {tuple(obs.shape[2:])}, the store holds {self.frame_shape}")
        for k, v in (("act", act), ("rew", rew), ("end", end), ("trunc", trunc)):
            if tuple(v.shape) != (b, t):
                raise ValueError(f"record_window: {k} is {tuple(v.shape)}, obs has (B, T) = {(b, t)}")
        if end.dtype != trunc.dtype or end.element_size() not in (1, 8) or end.is_floating_point():
            raise ValueError(f"record_window: end / trunc are {end.dtype} / {trunc.dtype}; integers of 1 or 8 bytes, both the same")
        if self.flag_dtype is None:
            self.flag_dtype = torch.int64 if end.element_size() == 8 else torch.uint8
        if b == 0 or t == 0:
            return []
        obs, act, rew = obs.contiguous(), act.to(torch.int64).contiguous(), rew.to(torch.float32).contiguous()
        end, trunc = end.contiguous(), trunc.contiguous()
        final = final_observation
        if final is not None and not isinstance(final, Tensor):
            final = torch.cat([f.reshape((-1,) + self.frame_shape) for f in final]) if len(final) else None
        if final is not None:
            if final.dtype != torch.float32 or tuple(final.shape[1:]) != self.frame_shape:
                raise ValueError(f"record_window: final_observation is {tuple(final.shape)} {final.dtype}; (n_dead,) + {self.frame_shape} float32")
            final = final.contiguous()

        # the one read-back
        n = b * t
        host = torch.cat((rew.reshape(-1).view(torch.uint8), (end.reshape(-1) != 0).to(torch.uint8), (trunc.reshape(-1) != 0).to(torch.uint8))).cpu().numpy()
        rew_h = host[: 4 * n].view(np.float32).reshape(b, t)
        end_h = host[4 * n: 5 * n].reshape(b, t) != 0
        dead_h = end_h | (host[5 * n:].reshape(b, t) != 0)
        deaths = [(tt, bb) for tt in range(t) for bb in range(b) if dead_h[bb, tt]]
        if final is not None and final.shape[0] != len(deaths):
            raise ValueError(f"record_window: {final.shape[0]} final observations for the window's {len(deaths)} deaths")
        final_of = {d: j for j, d in enumerate(deaths)}
        if self._capacity == 0 and self._want > 0:
            self.reserve(self._want)

        # the plan: where every env's steps go (host integers only)
        runs: List[Tuple[int, int, int, int]] = []
        used, wasted = self._used, 0
        events: List[Tuple[int, int, bool, _OpenEpisode]] = []  # (step, env, ended, episode): who is stored, in the reference's order
        touched: List[_OpenEpisode] = []
        opened = dict(self._open)
        for bb in range(b):
            t0 = 0
            while t0 < t:
                ends = np.flatnonzero(dead_h[bb, t0:])
                died = len(ends) > 0
                t1 = t0 + int(ends[0]) + 1 if died else t
                r = opened.get(bb)
                if r is None:
                    r = opened[bb] = _OpenEpisode()
                need = r.n + (t1 - t0)
                if need > r.slot:
                    slot = need if died else 2 * need
                    if r.slot == 0:
                        r.first, used = used, used + slot
                    elif r.first + r.slot == used:  # the arena's last: grows where it is
                        used = r.first + slot
                    else:  # moves to the arena's end; the old slot is a hole until compact()
                        runs.append((2, r.first, r.n, used))
                        wasted += r.slot
                        r.first, used = used, used + slot
                    r.slot = slot
                runs.append((0, bb * t + t0, t1 - t0, r.first + r.n))
                r.n = need
                r.ret += float(rew_h[bb, t0:t1].astype(np.float64).sum())
                r.counts = r.counts + _reward_end_counts(rew_h[bb, t0:t1], end_h[bb, t0:t1])
                touched.append(r)
                if died:
                    if r.first + r.slot == used:  # (an episode that ends as the arena's last gives its spare rows back)
                        used, r.slot = r.first + r.n, r.n
                    if final is not None:
                        r.final_row = self._finals_used + final_of[(t1 - 1, bb)]
                        runs.append((1, final_of[(t1 - 1, bb)], 1, r.final_row))
                    events.append((t1 - 1, bb, True, r))
                    del opened[bb]
                t0 = t1
        n_finals = len(deaths) if final is not None else 0
        self.reserve(used, self._finals_used + n_finals)  # (copies the rows handed out so far, should the arena have to grow)
        self._used, self._finals_used, self._open = used, self._finals_used + n_finals, opened
        self.wasted_frames += wasted

        table = np.array(runs, dtype=np.int64).reshape(-1, 4)
        if self._off_grid is None:
            self._off_grid = torch.zeros(1, dtype=torch.int32, device=self.device)
        p = nv.RecordWindowParams()
        p.R, p.flag_size, p.per_frame, p.total = len(table), end.element_size(), self.per_frame, int(table[:, 2].sum())
        p.steps, p.K, p.F, p.E = n, n_finals, self._capacity, 0 if self.finals is None else self.finals.shape[0]
        p.obs, p.act, p.rew, p.end, p.trunc, p.final_obs = nv.fptr(obs), nv.ptr(act), nv.fptr(rew), nv.ptr(end), nv.ptr(trunc), nv.fptr(final)
        p.frames, p.arena_act, p.arena_rew, p.arena_end, p.arena_trunc = (nv.ptr(x) for x in (self.frames, self.act, self.rew, self.end, self.trunc))
        p.finals, p.off_grid = nv.ptr(self.finals), nv.ptr(self._off_grid)
        p.runs = nv.ptr(torch.from_numpy(table).to(self.device, non_blocking=True))
        nv.check(nv.lib().dmd_record_window(C.byref(p), nv.stream()), "dmd_record_window")
        self._unchecked.extend(touched)

        if store_open_if_episodes is not None and len(deaths) >= store_open_if_episodes:
            events += [(t - 1, bb, False, r) for bb, r in opened.items()]
        done = []
        for _, _, ended, r in sorted(events, key=lambda e: e[:2]):
            eid = self._store(r)
            if ended:
                done.append({"episode_id": eid, "length": r.n, "return": r.ret})
        return done

    def end_collect(self, keep_open: bool) -> None:
        """The end of a collect.  keep_open=True (the train collector): the episodes still open are stored as far as they go, in
        env order, and stay extendable by the next `record_window`.  keep_open=False (`reset_every_collect`): they are let go of
        -- one that was never stored gives its rows back (the arena's last ones at once, the others through `wasted_frames` and
        `compact()`), a stored one stays as it was last stored."""
        if keep_open:
            for _, r in sorted(self._open.items()):
                self._store(r)
            return
        for r in sorted(self._open.values(), key=lambda r: -r.first):
            if r.eid is not None:  # (its stored rows are the first `lengths[eid]` of wherever it was written last)
                self._first[r.eid], self._slot[r.eid] = r.first, r.slot
            elif r.first + r.slot == self._used:
                self._used = r.first
            else:
                self.wasted_frames += r.slot
        self._open = {}

    def assert_on_grid(self) -> None:
        """Read the flag that `record_window`'s launches leave on the device (this waits for them): ValueError, as add_episode's,
        if a frame written since the last check was not on the uint8 grid -- naming the episodes written since then.  A store
        built with strict_grid=False only notes it in `saw_off_grid`."""
        written, self._unchecked = self._unchecked, []
        if not written or self._off_grid is None or int(self._off_grid.item()) == 0:
            return
        self._off_grid.zero_()
        self.saw_off_grid = True
        if not self.strict_grid:
            return
        ids = sorted({r.eid for r in written if r.eid is not None})
        unstored = len({id(r) for r in written if r.eid is None})
        raise ValueError(f"episodes {ids}" + (f" (and {unstored} not stored)" if unstored else "") + ": fp32 frames are not on the uint8 "
                         "grid ((level / 255) * 2 - 1): storing them as levels would change them")

    def load_episode(self, episode_id: int) -> Episode:
        """The stored episode, on the device, with the fields and dtypes of the reference's `Episode.load` (data/episode.py:36-43):
        obs fp32 (n, C, H, W), act int64, rew fp32, end / trunc uint8, info with `final_observation` (C, H, W) if it has one --
        one `gather`.  Persistence is `dataset.add_episode(store.load_episode(i))`."""
        eid = int(episode_id)
        if not 0 <= eid < self.num_episodes:
            raise ValueError(f"load_episode: episode {eid} of {self.num_episodes}")
        n = int(self.lengths[eid])
        flags = {k: torch.empty((1, n), dtype=torch.uint8, device=self.device) for k in ("end", "trunc")}
        b = self.gather([(eid, 0, n)], out=flags)
        return Episode(b.obs[0], b.act[0], b.rew[0], b.end[0], b.trunc[0], b.info[0])

    # -- sampling (host integers only) -------------------------------------------------------------------------------------------
    def sample_ids(self, batch_size: int, seq_length: int, *, can_sample_beyond_end: bool = False,
                   sample_weights: Optional[Sequence[float]] = None, rank: int = 0, world_size: int = 1, rng=np.random) -> List[SegmentId]:
        """Segment ids drawn as the reference's BatchSampler.sample draws them (data/batch_sampler.py:38-70): one `choice` over
        this rank's episodes (weighted by length, or by `sample_weights` over equal groups of episodes, the last group taking
        the remainder), one `randint` for the anchor step, one for the offset -- the same calls in the same order, so the same
        numpy seed gives the same ids.  Without `can_sample_beyond_end` a segment is padded in front only."""
        n_ep = self.num_episodes
        if sample_weights is None or n_ep < len(sample_weights):
            weights = self.lengths / self.num_steps
        else:
            k = len(sample_weights)
            assert all(0 <= w <= 1 for w in sample_weights) and sum(sample_weights) == 1
            group = [n_ep // k + (n_ep % k) * (i == k - 1) for i in range(k)]
            weights = [w / g for w, g in zip(sample_weights, group) for _ in range(g)]
        mine = np.arange(rank, n_ep, world_size)
        weights = np.array(weights[rank::world_size])
        episode_ids = rng.choice(mine, size=batch_size, replace=True, p=weights / weights.sum())
        lengths = self.lengths[episode_ids]
        anchors = rng.randint(low=0, high=lengths)
        if can_sample_beyond_end:
            starts = anchors - rng.randint(0, seq_length, len(anchors))
            stops = starts + seq_length
        else:
            stops = np.minimum(lengths, anchors + 1 + rng.randint(0, seq_length, len(anchors)))
            starts = stops - seq_length
        return [SegmentId(int(e), int(a), int(b)) for e, a, b in zip(episode_ids, starts, stops)]

    def traverse(self, batch_num_samples: int, chunk_size: int, **gather_kwargs: Any) -> Iterator[Batch]:
        """One pass over the store in chunks of `chunk_size` steps, `batch_num_samples` chunks per batch, as the reference's
        DatasetTraverser (data/utils.py:44-82): an episode's trailing chunk with fewer than 2 valid steps is dropped, the last
        batch may be short."""
        pending: List[SegmentId] = []
        for eid in range(self.num_episodes):
            n = int(self.lengths[eid])
            chunks = [SegmentId(eid, i * chunk_size, (i + 1) * chunk_size) for i in range(math.ceil(n / chunk_size))]
            if n - chunks[-1].start < 2:  # (an episode has at least one step, so at least one chunk)
                chunks.pop()
            pending.extend(chunks)
            while len(pending) >= batch_num_samples:
                yield self.gather(pending[:batch_num_samples], **gather_kwargs)
                pending = pending[batch_num_samples:]
        if pending:
            yield self.gather(pending, **gather_kwargs)

    # -- batches -----------------------------------------------------------------------------------------------------------------
    def _descriptor(self, ids: Sequence[Any]) -> Tuple[np.ndarray, int, List[SegmentId]]:
        if len(ids) == 0:
            raise ValueError("gather: no segment ids")
        seg = np.empty((len(ids), 4), dtype=np.int64)
        clipped = []
        t = None
        for i, sid in enumerate(ids):
            eid, start, stop = _id_fields(sid)
            if not 0 <= eid < self.num_episodes:
                raise ValueError(f"gather: segment {i}: episode {eid} of {self.num_episodes}")
            n = int(self.lengths[eid])
            if not (start < n and stop > 0 and start < stop):  # data/utils.py:19
                raise ValueError(f"gather: segment {i} = (episode {eid}, start {start}, stop {stop}) lies outside the episode's "
                                 f"{n} steps or is empty")
            if t is None:
                t = stop - start
            elif stop - start != t:
                raise ValueError(f"gather: segment {i} has {stop - start} steps, the batch's first has {t}")
            seg[i] = (self._first[eid], start, n, self._final_row[eid])
            clipped.append(SegmentId(eid, max(0, start), min(n, stop)))
        return seg, int(t), clipped

    def _out_tensors(self, b: int, t: int, out: Optional[Dict[str, Tensor]], want_final: bool) -> Dict[str, Tensor]:
        d = self.device
        spec = {"obs": ((b, t) + self.frame_shape, (torch.float32,)), "act": ((b, t), (torch.int64,)), "rew": ((b, t), (torch.float32,)),
                "end": ((b, t), _FLAG_DTYPES), "trunc": ((b, t), _FLAG_DTYPES), "mask_padding": ((b, t), (torch.bool, torch.uint8)),
                "final_obs": ((b,) + self.frame_shape, (torch.float32,))}
        res: Dict[str, Tensor] = {}
        for k, (shape, dtypes) in spec.items():
            given = None if out is None else out.get(k)
            if given is None:
                if k == "final_obs" and not want_final:
                    continue
                dtype = self.flag_dtype if k in ("end", "trunc") else dtypes[0]
                if k in ("end", "trunc") and "end" in res and res["end"].dtype != dtype:
                    dtype = res["end"].dtype  # (the kernel writes both flags with one element size)
                given = torch.empty(shape, dtype=dtype, device=d)
            else:
                if tuple(given.shape) != tuple(shape) or given.dtype not in dtypes or not given.is_contiguous() or given.device.type != d.type:
                    raise ValueError(f"gather: out[{k!r}] is {tuple(given.shape)} {given.dtype} on {given.device} "
                                     f"(contiguous: {given.is_contiguous()}); needed {tuple(shape)} of {dtypes} on {d}")
            res[k] = given
        if res["end"].element_size() != res["trunc"].element_size():
            raise ValueError("gather: out['end'] and out['trunc'] differ in element size")
        return res

    def _launch(self, seg: Tensor, res: Dict[str, Tensor], b: int, t: int, put_back_final: bool) -> None:
        p = nv.SegmentGatherParams()
        p.B, p.T, p.per_frame = b, t, self.per_frame
        flags = [res[k] for k in ("end", "trunc") if res.get(k) is not None]
        p.flag_size = flags[0].element_size() if flags else 1
        p.put_back_final = int(bool(put_back_final))
        p.frames, p.act, p.rew, p.end, p.trunc = (nv.ptr(x) for x in (self.frames, self.act, self.rew, self.end, self.trunc))
        p.finals = nv.ptr(self.finals)
        p.seg = nv.ptr(seg)
        p.out_obs, p.out_act, p.out_rew = nv.ptr(res.get("obs")), nv.ptr(res.get("act")), nv.ptr(res.get("rew"))
        p.out_end, p.out_trunc = nv.ptr(res.get("end")), nv.ptr(res.get("trunc"))
        p.out_mask, p.out_final = nv.ptr(res.get("mask_padding")), nv.ptr(res.get("final_obs"))
        nv.check(nv.lib().dmd_segment_gather(C.byref(p), nv.stream()), "dmd_segment_gather")

    def gather(self, ids: Sequence[Any], *, out: Optional[Dict[str, Tensor]] = None, put_back_final: bool = False,
               info: bool = True) -> Batch:
        """The batch of the segments `ids` ((episode_id, start, stop), SegmentId-like or tuples) in one launch: what
        `collate_segments_to_batch([dataset[i] for i in ids])` gives, on the device.  The ids are validated on the host before
        anything is launched (ValueError); nothing is read back.
        out: preallocated tensors by field name (obs, act, rew, end, trunc, mask_padding, final_obs) -- e.g. a GraphedTrainStep's
        `.static`; the batch's fields ARE those tensors (fields `out` lacks are allocated), so the step's `copy_` of a field onto
        itself is skipped by torch and launches nothing.
        put_back_final: where an episode's end falls inside the segment, the frame after it is the episode's final observation
        instead of padding (what RewEndModel.forward / put_back_final_observations write there; the mask stays False).
        info: `batch.info[i]` is {"final_observation": a view of the batch's final_obs[i]} for samples whose episode has one and
        {} otherwise, as the reference's; False: empty dicts and no final_obs output."""
        nv.check_current_device(self.device)
        seg, t, clipped = self._descriptor(ids)
        b = len(clipped)
        res = self._out_tensors(b, t, out, bool(info))
        self._launch(torch.from_numpy(seg).to(self.device, non_blocking=True), res, b, t, put_back_final)
        infos: List[Dict[str, Any]] = [{} for _ in range(b)]
        if info:
            for i in np.flatnonzero(seg[:, 3] >= 0):
                infos[i]["final_observation"] = res["final_obs"][i]
        mask = res["mask_padding"]
        return Batch(res["obs"], res["act"], res["rew"], res["end"], res["trunc"], mask if mask.dtype == torch.bool else mask.view(torch.bool),
                     infos, clipped)

    def gather_static(self, seg_device: Tensor, out: Dict[str, Tensor], *, put_back_final: bool = False) -> None:
        """The same launch from a caller-owned (B, 4) int64 device descriptor (rows: arena row of the episode's step 0, the
        segment's first step, the episode's length, its row of final observations or -1 -- `descriptor(ids)` builds it on the
        host) into the tensors of `out` (any of obs, act, rew, end, trunc, mask_padding, final_obs; at least one (B, T, ...)
        field).  It does nothing else -- no validation of the descriptor's contents, no allocation, no upload -- so it can be
        recorded in a hipGraph and replayed after the descriptor's contents change.  The recorded launch holds the arena's
        pointers: under a captured graph the arena must not grow, i.e. `generation` must not change (reserve() the rows
        and the final observations first; add_episode within the reservation, and replacement that fits, leave `generation`
        alone; compact() does not)."""
        assert seg_device.dtype == torch.int64 and seg_device.dim() == 2 and seg_device.shape[1] == 4 and seg_device.is_contiguous()
        b = seg_device.shape[0]
        ts = [out[k].shape[1] for k in ("obs",) + _SMALL if out.get(k) is not None]
        assert ts and all(x == ts[0] for x in ts), "gather_static: `out` needs a (B, T, ...) field, all of one T"
        for k, v in out.items():
            assert v is None or (v.shape[0] == b and v.is_contiguous()), f"gather_static: out[{k!r}]"
        flags = [out[k].element_size() for k in ("end", "trunc") if out.get(k) is not None]
        assert len(set(flags)) <= 1, "gather_static: end and trunc differ in element size"
        self._launch(seg_device, out, b, ts[0], put_back_final)

    def descriptor(self, ids: Sequence[Any]) -> Tensor:
        """The validated (B, 4) int64 descriptor of `ids` as a HOST tensor (copy it into the device tensor a captured
        `gather_static` reads)."""
        return torch.from_numpy(self._descriptor(ids)[0])


class DeviceSegmentLoader:
    """Endless iterator of Batches drawn from a DeviceReplay: stands where the trainer's DataLoader over (Dataset, BatchSampler)
    stood -- as the `data_loader` of WorldModelEnv (it has `.batch_sampler.batch_size`) or the loader of a training loop.  Draws
    come from numpy only (`rng`, default the global numpy state like the reference's sampler): no torch generator is touched."""

    def __init__(self, store: DeviceReplay, batch_size: int, seq_length: int, *, put_back_final: bool = False, info: bool = True,
                 out: Optional[Dict[str, Tensor]] = None, **sampler_kwargs: Any) -> None:
        self.store = store
        self.batch_sampler = SimpleNamespace(batch_size=int(batch_size), seq_length=int(seq_length), **sampler_kwargs)
        self._sampler_kwargs = sampler_kwargs
        self._gather_kwargs = dict(put_back_final=put_back_final, info=info, out=out)

    def __iter__(self) -> "DeviceSegmentLoader":
        return self

    def __next__(self) -> Batch:
        bs = self.batch_sampler
        return self.store.gather(self.store.sample_ids(bs.batch_size, bs.seq_length, **self._sampler_kwargs), **self._gather_kwargs)
