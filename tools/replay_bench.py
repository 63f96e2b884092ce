"""The device-resident replay store (diamond_amd/replay.py) at the reward / end model's training shape: batch 32, segments of 20
frames of 3 x 64 x 64, from an arena of `--frames` uint8 frames (default 100,000 = 1.2 GB: the Atari-100k buffer).

  kernel timing      `dmd_segment_gather` (DeviceReplay.gather_static from a device descriptor) against a plain fp32 device copy
                     of a tensor of the OUTPUT's size (torch `copy_`), HIP events around `--launches` launches per block -- each
                     arm's block captured once as a linear hipGraph and replayed, so that the device and not the python around a
                     launch is timed -- the two arms alternating over `--blocks` blocks in one process.  Both arms rotate over `--buffers` output tensors
                     (and the copy over as many sources) so that a block writes more than the 256 MB Infinity Cache holds; the
                     gather's descriptors are `--buffers` different random batches.  Bytes the algorithm needs: the gather reads
                     1 and writes 4 per value (1.25 x the output), the copy reads 4 and writes 4 (2 x).  THE BAR: the gather's
                     median is not above the copy's.
  batches per second (information only, no bar) DeviceSegmentLoader -- numpy draws of the ids, the (B, 4) descriptor's upload, one
                     launch -- against the numpy restatement of tests/replay_cases.py plus the upload of its fields, host clock
                     around `--batches` batches ending in a device synchronise.  One box, one process.

Prints one JSON line and writes it to profiles/device_replay.json.  Needs the GPU (there is no CPU path to time):

    timeout -k 10 600 python tools/replay_bench.py
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAME = (3, 64, 64)


def fill_store(store, frames, episode_len, dev, seed):
    """episodes of `episode_len` uint8 frames generated on the device; every second one ends (and has a final observation)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    k = 0
    while store.num_steps < frames:
        n = min(episode_len, frames - store.num_steps)
        end = torch.zeros(n, dtype=torch.int64)
        info = {}
        if k % 2:
            end[-1] = 1
            info["final_observation"] = torch.randint(0, 256, FRAME, generator=g, device=dev, dtype=torch.uint8)
        store.add_episode(SimpleNamespace(obs=torch.randint(0, 256, (n,) + FRAME, generator=g, device=dev, dtype=torch.uint8),
                                          act=torch.randint(0, 4, (n,), generator=g, device=dev), rew=torch.randn(n, generator=g, device=dev),
                                          end=end, trunc=torch.zeros(n, dtype=torch.int64), info=info))
        k += 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-length", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--episode-len", type=int, default=1000)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--launches", type=int, default=48, help="launches per timed block")
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--batches", type=int, default=200, help="batches of the batches-per-second legs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_replay.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_bench: no GPU visible -- NOT measured (a kernel time exists on the device only)")

    from diamond_amd.replay import DeviceReplay, DeviceSegmentLoader
    from tests import replay_cases as RC

    dev = torch.device("cuda:0")
    b, t, pf = args.batch, args.seq_length, int(np.prod(FRAME))
    store = DeviceReplay(dev, frame_shape=FRAME, capacity_frames=args.frames)
    fill_store(store, args.frames, args.episode_len, dev, 1)
    assert store.frames.shape[0] == args.frames and store.wasted_frames == 0  # the reservation held: no reallocation of the arena
    rng = np.random.RandomState(0)
    outs = [{"obs": torch.empty((b, t) + FRAME, device=dev), "act": torch.empty((b, t), dtype=torch.int64, device=dev),
             "rew": torch.empty((b, t), device=dev), "end": torch.empty((b, t), dtype=torch.int64, device=dev),
             "trunc": torch.empty((b, t), dtype=torch.int64, device=dev), "mask_padding": torch.empty((b, t), dtype=torch.bool, device=dev)}
            for _ in range(args.buffers)]
    segs = [store.descriptor(store.sample_ids(b, t, can_sample_beyond_end=True, rng=rng)).to(dev) for _ in range(args.buffers)]
    srcs = [torch.randn((b, t) + FRAME, device=dev) for _ in range(args.buffers)]
    dsts = [torch.empty((b, t) + FRAME, device=dev) for _ in range(args.buffers)]

    def gather(i):
        store.gather_static(segs[i % args.buffers], outs[i % args.buffers], put_back_final=True)

    def copy(i):
        dsts[i % args.buffers].copy_(srcs[i % args.buffers])

    # each arm's block of launches is captured once and REPLAYED (a linear graph): the python around a launch -- 14 pointers into
    # a ctypes struct for the gather -- takes longer than either kernel, and an eager loop would time the host's enqueue rate
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in (("gather", gather), ("copy", copy)):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(2 * args.buffers):
                fn(i)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for i in range(args.launches):
                fn(i)
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    us = {name: [] for name in graphs}
    for _ in range(args.blocks):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    med = {k: statistics.median(v) for k, v in us.items()}
    out_bytes = 4 * b * t * pf
    moved = {"gather": 1.25 * out_bytes, "copy": 2.0 * out_bytes}

    # batches per second: the loader (ids, descriptor, launch) against the CPU restatement + upload (information only)
    loader = DeviceSegmentLoader(store, b, t, can_sample_beyond_end=True, rng=np.random.RandomState(1), put_back_final=True, info=False)
    for _ in range(5):
        next(loader)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.batches):
        batch = next(loader)
    torch.cuda.synchronize()
    loader_bps = args.batches / (time.perf_counter() - t0)
    del batch
    arena = RC.make_arena(pf, seed=2)  # (a small host arena: the restatement's cost per batch does not depend on the arena's size)
    rows = RC.all_segments(arena, t)
    pick = np.random.RandomState(2)
    n_cpu = max(3, args.batches // 20)
    t0 = time.perf_counter()
    for _ in range(n_cpu):
        r = RC.restate(arena, rows[pick.randint(0, len(rows), b)], t, np.int64, True)
        up = [torch.from_numpy(r[k]).to(dev) for k in ("obs", "act", "rew", "end", "trunc", "mask_padding")]
    torch.cuda.synchronize()
    cpu_bps = n_cpu / (time.perf_counter() - t0)
    del up

    line = {"what": "dmd_segment_gather against a plain fp32 device copy of its output, us per launch (HIP events)",
            "device": torch.cuda.get_device_name(0), "library": os.path.basename(os.environ.get("DIAMOND_LIB", "libdiamond_hip.so")),
            "batch": b, "segment": t, "frame": list(FRAME), "arena_frames": store.num_steps, "arena_bytes": store.nbytes,
            "arena_bytes_per_100k_frames": round(store.nbytes * 100_000 / store.num_steps), "wasted_frames": store.wasted_frames,
            "buffers": args.buffers, "launches_per_block": args.launches, "blocks": args.blocks, "output_bytes": out_bytes,
            "median_us": {k: round(v, 3) for k, v in med.items()},
            "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
            "blocks_us": {k: [round(x, 3) for x in v] for k, v in us.items()},
            "algorithmic_bytes": moved, "achieved_TB_per_s": {k: round(moved[k] / (med[k] * 1e-6) / 1e12, 3) for k in med},
            "gather_over_copy": round(med["gather"] / med["copy"], 4), "bar_gather_not_above_copy": bool(med["gather"] <= med["copy"]),
            "batches_per_s_information_only": {"device_segment_loader": round(loader_bps, 1), "numpy_restatement_plus_upload": round(cpu_bps, 2),
                                               "batches_timed": [args.batches, n_cpu], "note": "one box, one process, host clock"}}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0 if line["bar_gather_not_above_copy"] else 1


if __name__ == "__main__":
    sys.exit(main())
