"""What closing the open-loop evaluation's step on the device is worth (diamond_amd/openloop.py, dmd_openloop_step): batch 32,
horizon 15, frames of 3 x 64 x 64, a 3-step sampler, the default agent with re-randomised weights.

  arm A  `open_loop_eval`: per step the sampler, the reward / end model and ONE dmd_openloop_step launch
  arm B  the same loop written with the entry points that existed before it (tests/openloop_cases.py `reference_loop`: an fp32
         `gather` of the whole segment, dmd_quantize_u8 of prediction and target, torch integer ops, masks, explicit ring writes)

Both arms in one process, alternating over `--blocks` blocks of `--evals` evaluations each, HIP events around a block (which ends in
a device synchronise).  The sampler dominates both arms: the number to read is the DIFFERENCE of the medians and whether it
exceeds the block-to-block spread.  Launches per evaluated step are counted in a pass of their own: the C-ABI launches through
native.PROFILER's hook, every device kernel (torch's included) from a torch.profiler trace of one evaluation per arm.

Prints one JSON line and writes it to profiles/openloop_eval.json.  Needs the GPU (there is no CPU path to time):

    timeout -k 10 900 python tools/openloop_bench.py

`--ssim`: what `open_loop_eval(..., ssim=True)` costs instead -- arm `ssim_off` (exactly the launches above) against arm `ssim_on`
(one dmd_frame_ssim call per step more) in the same alternating blocks, the entry point's own time from a replayed graph of
`--ssim-graph-calls` arena-mode calls, and its largest difference from the 121-tap numpy restatement (tests/ssim_cases.py) over
the GPU tests' production shapes.  Writes profiles/openloop_ssim.json.

`--motion`: the same for `open_loop_eval(..., motion=True)` -- arm `motion_off` against arm `motion_on` (one dmd_openloop_motion
launch per step more) in the same alternating blocks, and the entry point's own time from a replayed graph of `--ssim-graph-calls`
calls.  Writes profiles/openloop_motion.json.
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAME = (3, 64, 64)


class LaunchCounter:
    """native.PROFILER stand-in that only counts the C-ABI launches."""

    def __init__(self):
        self.n = 0

    def annotate(self, key, flops, nbytes):
        pass

    def call(self, name, fn, args):
        self.n += 1
        return fn(*args)


def device_kernels(fn):
    """Device kernels one call of `fn` launches (a torch.profiler trace); None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001
        print(f"openloop_bench: no kernel trace ({e!r})", file=sys.stderr)
        return None


def blocks_ms(arms, blocks, evals):
    """ms per evaluation of every arm over alternating blocks (HIP events around a block, which ends in a synchronise)."""
    ms = {name: [] for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(evals):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / evals)
    return ms


def ssim_arms(args, sampler, agent, store, ids, t):
    import ctypes

    from diamond_amd import native as nv
    from diamond_amd.metrics import frame_ssim, set_operand, ssim_params, ssim_workspace
    from diamond_amd.openloop import open_loop_eval
    from tests import ssim_cases as SC

    dev, b, horizon, tf = store.device, args.batch, args.horizon, args.teacher_forced
    arms = {"ssim_off": lambda: open_loop_eval(sampler, agent.rew_end_model, store, ids, horizon, teacher_forced=tf),
            "ssim_on": lambda: open_loop_eval(sampler, agent.rew_end_model, store, ids, horizon, teacher_forced=tf, ssim=True)}
    noise = torch.randn(horizon, b, *FRAME, device=dev)
    reports = {}
    for name, fn in arms.items():  # the same injected draws: ssim changes no other field
        left = list(noise)
        sampler.noise_fn = lambda shape, d: left.pop()
        reports[name] = fn()
    sampler.noise_fn = None
    same = all(torch.equal(getattr(reports["ssim_on"], k), getattr(reports["ssim_off"], k)) for k in
               ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "ctx_obs"))
    sm = reports["ssim_on"].summary()
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = blocks_ms(arms, args.blocks, args.evals)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}

    # the entry point alone: a graph of arena-mode calls on a prediction-shaped operand, replayed
    seg = torch.from_numpy(store._descriptor(ids)[0]).to(dev)
    pred = torch.rand((b,) + FRAME, device=dev) * 2 - 1
    p = ssim_params(b, *FRAME)
    set_operand(p, "a", pred)
    work, out = ssim_workspace(p, dev), torch.empty((b, 2), dtype=torch.float64, device=dev)
    p.frames, p.finals, p.end, p.seg = (nv.ptr(x) for x in (store.frames, store.finals, store.end, seg))
    p.T, p.step, p.workspace, p.out = t, 0, nv.ptr(work), nv.ptr(out)
    call = lambda: nv.check(nv.lib().dmd_frame_ssim(ctypes.byref(p), nv.stream()), "dmd_frame_ssim")
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.ssim_graph_calls):
            call()
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / args.ssim_graph_calls)

    worst = {}
    for shape in ((11, 3, 64, 64), (2, 3, 256, 256), (2, 3, 68, 76)):
        x, y = SC.pair("plus minus 2", shape, seed=1)
        got = frame_ssim(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
        worst["x".join(map(str, shape))] = float(np.abs(got - SC.restate(x, y)).max())

    diff = med["ssim_on"] - med["ssim_off"]
    line = {"what": "open_loop_eval(ssim=True) against ssim=False of the same tree, ms per evaluation (HIP events around alternating blocks)",
            "device": torch.cuda.get_device_name(0), "batch": b, "horizon": horizon, "context": t, "frame": list(FRAME),
            "denoising_steps": args.denoising_steps, "teacher_forced": tf, "evals_per_block": args.evals, "blocks_per_arm": args.blocks,
            "other_fields_agree_bitwise": bool(same), "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_ms": {k: round(v, 4) for k, v in spread.items()}, "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "ssim_on_minus_off_ms": round(diff, 4), "increase_exceeds_larger_spread": bool(diff > max(spread.values())),
            "frame_ssim_call_us_graph_replay": {"calls_per_graph": args.ssim_graph_calls, "median": round(statistics.median(us), 3),
                                                "blocks": [round(x, 3) for x in us]},
            "frame_ssim_calls_per_evaluation": horizon, "summary_ssim": sm["ssim"], "summary_ssim_cs": sm["ssim_cs"],
            "max_abs_diff_from_restatement": {"tolerance": SC.TOL, "device": worst, "interpreter": args.interpreter_max_diff}}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


def motion_arms(args, sampler, agent, store, ids, t):
    import ctypes

    from diamond_amd import native as nv
    from diamond_amd.openloop import MOTION_FIELDS, open_loop_eval

    dev, b, horizon, tf = store.device, args.batch, args.horizon, args.teacher_forced
    arms = {"motion_off": lambda: open_loop_eval(sampler, agent.rew_end_model, store, ids, horizon, teacher_forced=tf),
            "motion_on": lambda: open_loop_eval(sampler, agent.rew_end_model, store, ids, horizon, teacher_forced=tf, motion=True)}
    noise = torch.randn(horizon, b, *FRAME, device=dev)
    reports = {}
    for name, fn in arms.items():  # the same injected draws: motion changes no other field
        left = list(noise)
        sampler.noise_fn = lambda shape, d: left.pop()
        reports[name] = fn()
    sampler.noise_fn = None
    same = all(torch.equal(getattr(reports["motion_on"], k), getattr(reports["motion_off"], k)) for k in
               ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid", "logits_rew", "logits_end", "ctx_obs"))
    sm = reports["motion_on"].summary()
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = blocks_ms(arms, args.blocks, args.evals)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}

    # the entry point alone: a graph of calls on a prediction-shaped operand and a ring, replayed
    seg = torch.from_numpy(store._descriptor(ids)[0]).to(dev)
    pred = torch.rand((b,) + FRAME, device=dev) * 2 - 1
    ring = torch.rand((b, t) + FRAME, device=dev) * 2 - 1
    out, valid = torch.empty((b, 8), dtype=torch.int64, device=dev), torch.empty((b, 3), dtype=torch.uint8, device=dev)
    p = nv.MotionParams()
    p.B, p.T, p.per_frame, p.step, p.head = b, t, store.per_frame, 0, 0
    p.frames, p.end, p.finals, p.seg = (nv.ptr(x) for x in (store.frames, store.end, store.finals, seg))
    p.pred, p.ctx_obs, p.out, p.out_valid = nv.fptr(pred), nv.fptr(ring), nv.ptr(out), nv.ptr(valid)
    call = lambda: nv.check(nv.lib().dmd_openloop_motion(ctypes.byref(p), nv.stream()), "dmd_openloop_motion")
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.ssim_graph_calls):
            call()
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000.0 / args.ssim_graph_calls)
    nbytes = int(valid[:, 0].sum()) * store.per_frame * 9 + int(valid[:, 1].sum()) * store.per_frame + int(valid[:, 2].sum()) * store.per_frame

    diff = med["motion_on"] - med["motion_off"]
    line = {"what": "open_loop_eval(motion=True) against motion=False of the same tree, ms per evaluation (HIP events around alternating blocks)",
            "device": torch.cuda.get_device_name(0), "batch": b, "horizon": horizon, "context": t, "frame": list(FRAME),
            "denoising_steps": args.denoising_steps, "teacher_forced": tf, "evals_per_block": args.evals, "blocks_per_arm": args.blocks,
            "other_fields_agree_bitwise": bool(same), "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_ms": {k: round(v, 4) for k, v in spread.items()}, "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "motion_on_minus_off_ms": round(diff, 4), "increase_exceeds_larger_spread": bool(diff > max(spread.values())),
            "openloop_motion_call_us_graph_replay": {"calls_per_graph": args.ssim_graph_calls, "median": round(statistics.median(us), 3),
                                                     "blocks": [round(x, 3) for x in us], "bytes_read_per_call": nbytes,
                                                     "note": "the same buffers every call: they stay in the caches, not an HBM figure"},
            "openloop_motion_calls_per_evaluation": horizon,
            "summary": {k: sm[k] for k in ("skill_prev", "skill_anchor", "change_recall", "change_precision", "share_changed")},
            "report_fields": list(MOTION_FIELDS)}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--denoising-steps", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--episode-len", type=int, default=40)
    ap.add_argument("--evals", type=int, default=20, help="evaluations per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="blocks per arm")
    ap.add_argument("--teacher-forced", action="store_true")
    ap.add_argument("--no-kernel-trace", action="store_true", help="count the C-ABI launches only (no torch.profiler pass)")
    ap.add_argument("--ssim", action="store_true", help="time open_loop_eval(ssim=True) against ssim=False instead")
    ap.add_argument("--motion", action="store_true", help="time open_loop_eval(motion=True) against motion=False instead")
    ap.add_argument("--ssim-graph-calls", type=int, default=200, help="dmd_frame_ssim / dmd_openloop_motion calls in the replayed graph")
    ap.add_argument("--interpreter-max-diff", type=float, default=None,
                    help="recorded as given: the largest difference tests/test_ssim_simt.py printed (pytest -s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "openloop_ssim.json" if args.ssim else "openloop_motion.json" if args.motion else "openloop_eval.json")
    if not torch.cuda.is_available():
        sys.exit("openloop_bench: no GPU visible -- NOT measured (a time exists on the device only)")

    import diamond_amd as D
    from diamond_amd import native as nv
    from diamond_amd.openloop import open_loop_eval
    from diamond_amd.replay import DeviceReplay
    from diamond_amd.testing import fill_module_
    from tests.openloop_cases import reference_loop

    dev = torch.device("cuda:0")
    agent = D.Agent(D.default_agent_config())
    fill_module_(agent, 7)
    agent = agent.to(dev).eval()
    t = agent.denoiser.cfg.inner_model.num_steps_conditioning
    b, horizon, tf = args.batch, args.horizon, args.teacher_forced

    store = DeviceReplay(dev, frame_shape=FRAME, capacity_frames=args.episodes * args.episode_len)
    g = torch.Generator(device=dev).manual_seed(1)
    for k in range(args.episodes):  # every second episode ends and has a final observation
        n = args.episode_len
        end = torch.zeros(n, dtype=torch.int64)
        info = {}
        if k % 2:
            end[-1] = 1
            info["final_observation"] = torch.randint(0, 256, FRAME, generator=g, device=dev, dtype=torch.uint8)
        store.add_episode(SimpleNamespace(obs=torch.randint(0, 256, (n,) + FRAME, generator=g, device=dev, dtype=torch.uint8),
                                          act=torch.randint(0, 4, (n,), generator=g, device=dev), rew=torch.randint(-1, 2, (n,), generator=g, device=dev).float(),
                                          end=end, trunc=torch.zeros(n, dtype=torch.int64), info=info))
    rng = np.random.RandomState(0)
    drawn = store.sample_ids(b, t + horizon, can_sample_beyond_end=True, rng=rng)
    starts = [(int(i.episode_id), max(int(i.start), 1 - t)) for i in drawn]  # (at least one context frame: the same starts serve horizon 1 below)
    ids = [(e, s, s + t + horizon) for e, s in starts]
    sampler = D.DiffusionSampler(agent.denoiser, D.DiffusionSamplerConfig(num_steps_denoising=args.denoising_steps))

    def make_arms(h):
        ids_h = [(e, s, s + t + h) for e, s in starts]
        return {"open_loop_eval": lambda: open_loop_eval(sampler, agent.rew_end_model, store, ids_h, h, teacher_forced=tf),
                "reference_loop": lambda: reference_loop(sampler, agent.rew_end_model, store, ids_h, t, h, tf)}

    if args.ssim:
        return ssim_arms(args, sampler, agent, store, ids, t)
    if args.motion:
        return motion_arms(args, sampler, agent, store, ids, t)

    arms = make_arms(horizon)

    # the two arms agree (same injected draws) before anything is timed
    noise = torch.randn(horizon, b, *FRAME, device=dev)
    results = {}
    for name, fn in arms.items():
        left = list(noise)
        sampler.noise_fn = lambda shape, d: left.pop()
        results[name] = fn()
    sampler.noise_fn = None
    rep, (want, ctx_obs, _, _) = results["open_loop_eval"], results["reference_loop"]
    same = all(torch.equal(getattr(rep, k), want[k]) for k in ("sq_err", "abs_err", "max_err", "pixels_off", "frame_valid", "transition_valid",
                                                                "logits_rew", "logits_end")) and torch.equal(rep.ctx_obs, ctx_obs)

    for fn in arms.values():  # warm-up (the first calls above packed the weights)
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(args.blocks):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.evals):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.evals)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}

    # launches, in a pass of their own: per evaluation, and per evaluated step = (horizon H - horizon 1) / (H - 1), which leaves
    # the context set-up and the burn-in out
    def count(fn):
        counter = LaunchCounter()
        nv.PROFILER = counter
        try:
            fn()
        finally:
            nv.PROFILER = None
        return counter.n, None if args.no_kernel_trace else device_kernels(fn)

    one = make_arms(1)
    abi, kernels, abi_step, kernels_step = {}, {}, {}, {}
    for name in arms:
        (abi[name], kernels[name]), (a1, k1) = count(arms[name]), count(one[name])
        abi_step[name] = round((abi[name] - a1) / max(1, horizon - 1), 2)
        kernels_step[name] = None if None in (kernels[name], k1) else round((kernels[name] - k1) / max(1, horizon - 1), 2)
    diff = med["reference_loop"] - med["open_loop_eval"]
    line = {"what": "open_loop_eval against the same loop on the earlier entry points, ms per evaluation (HIP events around blocks)",
            "device": torch.cuda.get_device_name(0), "batch": b, "horizon": horizon, "context": t, "frame": list(FRAME),
            "denoising_steps": args.denoising_steps, "teacher_forced": tf, "evals_per_block": args.evals, "blocks_per_arm": args.blocks,
            "arms_agree_bitwise": bool(same), "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_ms": {k: round(v, 4) for k, v in spread.items()}, "blocks_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "reference_minus_open_loop_ms": round(diff, 4), "difference_exceeds_spread": bool(abs(diff) > max(spread.values())),
            "abi_launches_per_evaluation": abi, "device_kernels_per_evaluation": kernels,
            "abi_launches_per_step": abi_step, "device_kernels_per_step": kernels_step}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
