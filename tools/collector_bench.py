"""One collected window into the device replay store, against the path it replaces: B = 8 envs, T = 64 env steps of 3 x 64 x 64
frames, onto episodes that are already `--episode-len` (1,000) steps long.

  record_window   DeviceReplay.record_window of the env loop's stacked device tensors (one read-back of B x T x 6 bytes, one
                  dmd_record_window launch), end_collect(keep_open=True), assert_on_grid() -- which waits for the launch.
                  The open episodes' slots hold twice what they needed when they last grew, so the window is appended where the
                  episodes are (the amortised case; a move of the 1,000 rows is a device copy inside the same launch).
  host_episode    what the reference's collector does with the same window (coroutines/collector.py:53-106) in front of
                  `DeviceReplay.add_episode(..., episode_id=)`: `(end + trunc).item()` per env and step, the env's steps
                  concatenated into a CPU episode, the stored episode (CPU, fp32) concatenated with it, and the grown episode
                  uploaded and quantised whole again.

Host clock around one window, ending in a device synchronise; before each timed window the stores are put back to episodes of
`--episode-len` steps, untimed.  The two arms alternate over `--blocks` blocks of `--reps` windows in one process: medians of the
block means and the block-to-block spread.  Nobody has measured either arm before: the number is reported, there is no bar.

Prints one JSON line and writes it to profiles/device_collector.json.  Needs the GPU:

    timeout -k 10 600 python tools/collector_bench.py
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

import torch  # noqa: E402

FRAME = (3, 64, 64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--episode-len", type=int, default=1000)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3, help="windows per timed block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_collector.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("collector_bench: no GPU visible -- NOT measured (the store exists on the device only)")

    from diamond_amd.replay import DeviceReplay

    dev = torch.device("cuda:0")
    b, t, n0 = args.envs, args.window, args.episode_len
    g = torch.Generator().manual_seed(0)

    def steps(n):  # the env loop's stacked tensors for n steps, nobody dies; dequantised on the HOST: the device's division by a
        # scalar is a multiplication by its reciprocal, whose results are not all on the grid
        obs = torch.randint(0, 256, (b, n) + FRAME, generator=g, dtype=torch.uint8).div(255).mul(2).sub(1)
        return (obs, torch.randint(0, 4, (b, n), generator=g), torch.randint(-1, 2, (b, n), generator=g).float(),
                torch.zeros((b, n), dtype=torch.uint8), torch.zeros((b, n), dtype=torch.uint8))

    history_host, window_host = steps(n0), steps(t)
    history, window = tuple(x.to(dev) for x in history_host), tuple(x.to(dev) for x in window_host)
    rows = b * 2 * (n0 + t) + b * (n0 + t)

    # -- arm A: the window goes from the device tensors into the arena
    store_a = DeviceReplay(dev, frame_shape=FRAME, capacity_frames=rows, name="a")

    def setup_a():
        store_a.clear()
        store_a.record_window(*history)
        store_a.end_collect(keep_open=True)
        store_a.assert_on_grid()

    def run_a():
        store_a.record_window(*window)
        store_a.end_collect(keep_open=True)
        store_a.assert_on_grid()  # (reads the flag: waits for the launch)

    # -- arm B: the reference collector's host episodes in front of add_episode(..., episode_id=)
    store_b = DeviceReplay(dev, frame_shape=FRAME, capacity_frames=rows, name="b")
    host = [SimpleNamespace(**{k: v[i] for k, v in zip(("obs", "act", "rew", "end", "trunc"), history_host)}, info={}) for i in range(b)]
    for e in host:
        store_b.add_episode(e)

    def setup_b():
        for i, e in enumerate(host):
            store_b.add_episode(e, episode_id=i)
        torch.cuda.synchronize()

    def run_b():
        obs, act, rew, end, trunc = window
        dead = [[(end[i, s] + trunc[i, s]).clip(max=1).item() for i in range(b)] for s in range(t)]  # collector.py:60-62
        assert not any(map(any, dead))
        for i in range(b):
            new = [torch.cat([x[i, s:s + 1] for s in range(t)]).to("cpu") for x in (obs, act, rew, end, trunc)]  # :74
            old = host[i]                                                                                       # :76 (cache_in_ram)
            ep = SimpleNamespace(**{k: torch.cat((getattr(old, k), v)) for k, v in zip(("obs", "act", "rew", "end", "trunc"), new)}, info={})
            store_b.add_episode(ep, episode_id=i)                                                               # :77
        torch.cuda.synchronize()

    arms = {"record_window": (setup_a, run_a), "host_episode": (setup_b, run_b)}
    for setup, run in arms.values():  # warm-up: allocations, first-use costs, the slots' first growth
        for _ in range(2):
            setup()
            run()
    assert store_a.lengths.tolist() == [n0 + t] * b and store_b.lengths.tolist() == [n0 + t] * b
    ids = [(i, n0 - 2, n0 + t) for i in range(b)]
    assert all(torch.equal(getattr(store_a.gather(ids), k), getattr(store_b.gather(ids), k)) for k in ("obs", "act", "rew", "end", "trunc"))
    ms = {name: [] for name in arms}
    for _ in range(args.blocks):
        for name, (setup, run) in arms.items():
            total = 0.0
            for _ in range(args.reps):
                setup()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                total += time.perf_counter() - t0
            ms[name].append(1e3 * total / args.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"what": "one collected window into the device replay store, ms per window (host clock, ends in a device synchronise)",
            "device": torch.cuda.get_device_name(0), "envs": b, "window_steps": t, "frame": list(FRAME), "episode_steps_before": n0,
            "blocks": args.blocks, "windows_per_block": args.reps,
            "median_ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": {k: round(max(v) - min(v), 4) for k, v in ms.items()},
            "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "host_episode_over_record_window": round(med["host_episode"] / med["record_window"], 2),
            "window_bytes_fp32": 4 * b * t * FRAME[0] * FRAME[1] * FRAME[2], "note": "reported, not gated; one box, one process"}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
