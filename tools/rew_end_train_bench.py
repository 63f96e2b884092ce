"""One training step of the reward / end model at the trainer's shapes (batch 32, a segment of 19 steps plus one, 64 x 64, the
default agent; reference trainer.py:349-388: model(batch), backward, clip, AdamW), three arms in ONE process on one box:

  eager_forward   the eager loop on RewEndModel.forward (host round trip for the ends, boolean gathers, torch.bincount, one
                  autograd node per LSTM step)
  eager_static    the eager loop on put_back_final_observations + forward_static
  graph           train_graph.graphed_rew_end_step: the static step as one replayed hipGraph

ms per step from HIP events around `--steps` steps after `--warmup` steps, the arms alternating over `--rounds` rounds (the
median round is reported, all rounds are kept).  Prints one JSON line and writes it to profiles/rew_end_train_graph.json.  Needs
the GPU (there is no CPU path to time); run it as one process under a time limit:

    timeout -k 10 600 python tools/rew_end_train_bench.py
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


def make_batch(seed, b, t, dev):
    """a (b, t) segment: rewards in {-2 ... 2}, every eighth sample ends inside the segment (its steps behind the end are padding,
    its `info` carries the final observation), every fifth has a padded tail"""
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    g = torch.Generator().manual_seed(seed)
    obs = synthetic_frames(g, b, t, 3, 64, 64)
    act = synthetic_actions(g, 4, b, t)
    rew = torch.randint(-2, 3, (b, t), generator=g).float()
    end = torch.zeros(b, t, dtype=torch.long)
    mask = torch.ones(b, t, dtype=torch.bool)
    info = [{} for _ in range(b)]
    for i in range(b):
        if i % 8 == 1:
            when = 3 + i % (t - 4)
            end[i, when] = 1
            mask[i, when + 1:] = False
            info[i]["final_observation"] = synthetic_frames(g, 1, 3, 64, 64)[0].to(dev)
        elif i % 5 == 2:
            mask[i, t - 1 - i % 4:] = False
    return SimpleNamespace(obs=obs.to(dev), act=act.to(dev), rew=rew.to(dev), end=end.to(dev), trunc=torch.zeros(b, t, dtype=torch.long).to(dev),
                           mask_padding=mask.to(dev), info=info, segment_ids=None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-length", type=int, default=19, help="the trainer's seq_length; the segment holds one more frame")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-grad-norm", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rew_end_train_graph.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rew_end_train_bench: no GPU visible -- NOT measured (a step time exists on the device only)")

    import diamond_amd as D
    from diamond_amd.testing import fill_module_
    from diamond_amd.train_graph import graphed_rew_end_step

    dev = torch.device("cuda:0")
    b, t = args.batch, args.seq_length + 1

    def arm():
        agent = D.Agent(D.default_agent_config())
        fill_module_(agent, 7)
        m = agent.to(dev).rew_end_model.train()
        return m, torch.optim.AdamW(m.parameters(), lr=1e-4, capturable=True, fused=True), make_batch(3, b, t, dev)

    def eager(m, opt, fn):
        def step(batch):
            loss, _ = fn(batch)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), args.max_grad_norm)
            opt.step()
            opt.zero_grad(set_to_none=True)
        return step

    mg, og, bg = arm()
    gstep = graphed_rew_end_step(mg, og, args.max_grad_norm, bg, warmup_steps=args.warmup)
    mf, of, bf = arm()
    ms_, os_, bs = arm()

    def static(batch):
        ms_.put_back_final_observations(batch)
        return ms_.forward_static(batch)

    arms = [("eager_forward", eager(mf, of, mf), bf), ("eager_static", eager(ms_, os_, static), bs), ("graph", gstep, bg)]
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
    line = {"what": "reward/end model training step, ms per step (HIP events)", "device": torch.cuda.get_device_name(0),
            "batch": b, "segment": t, "size": 64, "steps": args.steps, "warmup": args.warmup, "optimizer": "AdamW capturable fused",
            "ms_per_step": {k: round(v, 4) for k, v in med.items()},
            "rounds_ms_per_step": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
            "graph_over_eager_forward": round(med["graph"] / med["eager_forward"], 4),
            "eager_static_over_eager_forward": round(med["eager_static"] / med["eager_forward"], 4)}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
