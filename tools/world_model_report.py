"""How good is this world model on this dataset?  Loads a checkpoint and a directory of recorded episodes (the files Episode.save
writes, which are the reference's: obs as uint8 levels, act, rew, end, trunc, info), puts every episode into a DeviceReplay with
`add_episode`, and runs `evaluate_store` over every window of the store twice -- free running (the model's own frames go back
into its context) and teacher forced (one-step errors at every horizon).  Prints one JSON object with both summaries: per step
mse / psnr / pixels_off / ssim, the skill over copying the previous recorded frame and over freezing the context, recall and
precision of the changed values, the error on changed and on static values, the reward / end confusion matrices.

    python tools/world_model_report.py checkpoints/agent_versions/agent_epoch_01000.pt dataset/test --horizon 15

Needs the GPU.  The host waits for the device once per summary."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def episode_files(directory):
    """Every *.pt file under `directory` but the dataset's own info.pt, in path order (the reference nests them by id)."""
    found = []
    for base, _, names in os.walk(directory):
        found += [os.path.join(base, n) for n in names if n.endswith(".pt") and n != "info.pt"]
    return sorted(found)


def load_store(directory, device):
    from diamond_amd.replay import DeviceReplay

    files = episode_files(directory)
    if not files:
        sys.exit(f"world_model_report: no episode file (*.pt) under {directory}")
    store = DeviceReplay(device)
    for path in files:
        d = torch.load(path, map_location="cpu", weights_only=False)
        store.add_episode(SimpleNamespace(obs=d["obs"], act=d["act"], rew=d["rew"], end=d["end"], trunc=d["trunc"], info=d.get("info", {})))
    return store, len(files)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="an agent checkpoint (Agent.load)")
    ap.add_argument("dataset", help="a directory of episode files")
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--stride", type=int, default=None, help="steps between window starts (default: the horizon)")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-windows", type=int, default=None)
    ap.add_argument("--denoising-steps", type=int, default=3)
    ap.add_argument("--num-actions", type=int, default=None, help="default: from the checkpoint's action embedding")
    ap.add_argument("--no-ssim", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("world_model_report: no GPU visible (there is no CPU path)")

    import diamond_amd as D
    from diamond_amd.openloop import evaluate_store

    dev = torch.device("cuda:0")
    store, n_files = load_store(args.dataset, dev)
    num_actions = args.num_actions if args.num_actions is not None else int(store.act[:store._used].max().item()) + 1
    agent = D.Agent(D.default_agent_config(num_actions=num_actions, img_size=int(store.frame_shape[-1]))).to(dev).eval()
    agent.load(args.checkpoint, load_actor_critic=False)
    sampler = D.DiffusionSampler(agent.denoiser, D.DiffusionSamplerConfig(num_steps_denoising=args.denoising_steps))
    out = {"checkpoint": args.checkpoint, "dataset": args.dataset, "episodes": n_files, "steps": len(store), "horizon": args.horizon,
           "denoising_steps": args.denoising_steps}
    for name, forced in (("free_running", False), ("teacher_forced", True)):
        totals = evaluate_store(sampler, agent.rew_end_model, store, args.horizon, batch_size=args.batch_size, stride=args.stride,
                                teacher_forced=forced, ssim=not args.no_ssim and len(store.frame_shape) == 3 and min(store.frame_shape[1:]) >= 11,
                                motion=True, max_windows=args.max_windows)
        out[name] = totals.summary()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
