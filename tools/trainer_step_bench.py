"""What the device-resident LR costs the replayed denoiser training step (batch 32, 4 conditioning + 1 predicted frame, 64 x 64, the
default agent: bench.py's `--config train` shapes), two arms in ONE process on one box:

  plain           GraphedTrainStep(den, opt, 1.0, batch): the LR a launch constant of the captured AdamW
  lr_scheduler    the same with lr_scheduler=LambdaLR(warm-up over 100 steps): the LR a 0-dim device tensor the captured AdamW reads,
                  one `fill_` of it and the host's closed form per call

ms per step from HIP events around blocks of `--steps` replays, the arms alternating over `--rounds` blocks each (200 replays per arm
by default).  Reported: each arm's median block, every block, and each arm's block-to-block spread (max - min); the expectation is
only that the two medians differ by less than the plain arm's spread.  Prints one JSON line and writes it to
profiles/trainer_step_ab.json.  Needs the GPU; run it as one process under a time limit:

    timeout -k 10 600 python tools/trainer_step_bench.py
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20, help="replays per block")
    ap.add_argument("--rounds", type=int, default=10, help="blocks per arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_step_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trainer_step_bench: no GPU visible -- NOT measured (a step time exists on the device only)")

    import diamond_amd as D
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames
    from diamond_amd.train_graph import GraphedTrainStep

    dev = torch.device("cuda:0")
    b, t = args.batch, 5

    def arm(with_scheduler):
        agent = D.Agent(D.default_agent_config())
        fill_module_(agent, 0)
        den = agent.denoiser.to(dev).train()
        den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
        g = torch.Generator().manual_seed(0)
        batch = SimpleNamespace(obs=synthetic_frames(g, b, t, 3, 64, 64).to(dev), act=synthetic_actions(g, 4, b, t).to(dev),
                                mask_padding=torch.ones(b, t, dtype=torch.bool, device=dev))
        opt = torch.optim.AdamW(den.parameters(), lr=1e-4, capturable=True, fused=True)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1 if s >= 100 else s / 100) if with_scheduler else None
        return GraphedTrainStep(den, opt, 1.0, batch, warmup_steps=args.warmup, lr_scheduler=sched), batch

    arms = [("plain", *arm(False)), ("lr_scheduler", *arm(True))]
    for _, step, batch in arms:
        for _ in range(args.warmup):
            step(batch)
    torch.cuda.synchronize()
    rounds = {name: [] for name, _, _ in arms}
    for _ in range(args.rounds):
        for name, step, batch in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(batch)
            e1.record()
            torch.cuda.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / args.steps)
    med = {name: statistics.median(v) for name, v in rounds.items()}
    spread = {name: max(v) - min(v) for name, v in rounds.items()}
    line = {"what": "replayed denoiser training step with and without lr_scheduler=, ms per step (HIP events)",
            "device": torch.cuda.get_device_name(0), "batch": b, "segment": t, "size": 64, "steps_per_block": args.steps,
            "blocks_per_arm": args.rounds, "replays_per_arm": args.steps * args.rounds, "optimizer": "AdamW capturable fused",
            "ms_per_step": {k: round(v, 4) for k, v in med.items()},
            "block_spread_ms": {k: round(v, 4) for k, v in spread.items()},
            "blocks_ms_per_step": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            "lr_scheduler_minus_plain_ms": round(med["lr_scheduler"] - med["plain"], 4),
            "within_plain_spread": abs(med["lr_scheduler"] - med["plain"]) <= spread["plain"]}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
