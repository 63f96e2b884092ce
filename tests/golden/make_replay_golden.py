"""Generate tests/golden/replay_segments.pt by EXECUTING THE REFERENCE'S DATA PIPELINE (build container only).

    python tests/golden/make_replay_golden.py

Imports /root/reference/src (with the stubs of `_refimport.py`) and runs the reference's own Dataset, BatchSampler, make_segment,
collate_segments_to_batch and DatasetTraverser on six synthetic uint8 episodes under fixed numpy seeds.  The file holds data only:
the episodes (uint8 levels), the sampled segment ids and the collated batches.  tests/test_replay_simt.py holds
diamond_amd.replay against it.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refimport as R  # noqa: E402

R.install()

FRAME = (3, 8, 8)
LENGTHS = (1, 2, 7, 30, 12, 9)
LAST = ("end", "trunc", "end", "trunc", "none", "end")  # how each episode's last step is marked
B, T = 4, 5
CASES = [(beyond, weights, rank, world) for beyond in (False, True) for weights in (None, [0.25, 0.75])
         for rank, world in ((0, 1), (1, 2), (2, 4))]


def episodes_u8():
    g = torch.Generator().manual_seed(2024)
    eps = []
    for n, last in zip(LENGTHS, LAST):
        end = torch.zeros(n, dtype=torch.uint8)
        trunc = torch.zeros(n, dtype=torch.uint8)
        if last != "none":
            (end if last == "end" else trunc)[-1] = 1
        eps.append({"obs": torch.randint(0, 256, (n,) + FRAME, generator=g, dtype=torch.uint8),
                    "act": torch.randint(0, 4, (n,), generator=g, dtype=torch.long),
                    "rew": torch.randint(-2, 3, (n,), generator=g).float(),
                    "end": end, "trunc": trunc,
                    "final": None if last == "none" else torch.randint(0, 256, FRAME, generator=g, dtype=torch.uint8)})
    return eps


def dequant(u8):
    return u8.div(255).mul(2).sub(1)  # data/episode.py:40


def pack(batch):
    return {"obs": batch.obs, "act": batch.act, "rew": batch.rew, "end": batch.end, "trunc": batch.trunc,
            "mask_padding": batch.mask_padding, "segment_ids": [(int(s.episode_id), int(s.start), int(s.stop)) for s in batch.segment_ids],
            "final_observation": [i.get("final_observation") for i in batch.info]}


def main():
    from data import BatchSampler, Dataset, DatasetTraverser, Episode, collate_segments_to_batch

    eps = episodes_u8()
    with tempfile.TemporaryDirectory() as tmp:
        ds = Dataset(tmp, cache_in_ram=True, save_on_disk=False)
        for e in eps:
            info = {} if e["final"] is None else {"final_observation": dequant(e["final"])}
            ds.add_episode(Episode(dequant(e["obs"]), e["act"], e["rew"], e["end"], e["trunc"], info))
        samples = []
        for seed, (beyond, weights, rank, world) in enumerate(CASES):
            # (the installed torch's Sampler.__init__ no longer takes the data source the reference passes it: the fields are
            #  set as BatchSampler.__init__ sets them, `sample` is the reference's)
            sampler = BatchSampler.__new__(BatchSampler)
            sampler.__dict__.update(dataset=ds, rank=rank, world_size=world, batch_size=B, seq_length=T, sample_weights=weights,
                                    can_sample_beyond_end=beyond)
            np.random.seed(100 + seed)
            ids = sampler.sample()
            batch = collate_segments_to_batch([ds[i] for i in ids])
            samples.append({"seed": 100 + seed, "batch_size": B, "seq_length": T, "can_sample_beyond_end": beyond,
                            "sample_weights": weights, "rank": rank, "world_size": world,
                            "ids": [(int(i.episode_id), int(i.start), int(i.stop)) for i in ids], "batch": pack(batch)})
        traverser = {"batch_num_samples": 4, "chunk_size": 5, "batches": [pack(b) for b in DatasetTraverser(ds, 4, 5)]}
        assert len(traverser["batches"]) == len(DatasetTraverser(ds, 4, 5))
    path = os.path.join(HERE, "replay_segments.pt")
    torch.save({"episodes": eps, "samples": samples, "traverser": traverser}, path)
    print(f"wrote replay_segments.pt: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
