"""dmd_conv2d_dgrad_input on the device (development aid, GPU): the precision table behind tests/test_dgrad_input.py's K_DGRAD and
the launch's time at the training shape -- a sibling of tools/wgrad_bench.py.

    python tools/dgrad_input_bench.py [precision|time|all] [reps]

precision: for every case of tests/test_dgrad_input.py (the same inputs) the kernel's error and float32 CPU conv_transpose2d's,
both relative to max |float64 result|, and their ratio; K_DGRAD is twice the largest ratio.  time: microseconds per launch (HIP
events around `reps` launches) at N = 32, 64x64, Cout = 64 with the denoiser's 15, the policy's 3 and the reward / end model's 6
input channels; a recorded measurement, no threshold.  The output is what profiles/dgrad_input_precision.txt keeps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from torch import nn

from diamond_amd import engine as E, grad_ops as G

what = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
props = torch.cuda.get_device_properties(0)
print(f"dmd_conv2d_dgrad_input, {props.name} ({props.gcnArchName.split(':')[0]}, {props.multi_processor_count} CUs)")

if what in ("precision", "all"):
    from tests import test_dgrad_input as T

    print(f"N = {T.N}; error against float64 conv_transpose2d relative to max |want|: the kernel's, float32 CPU conv_transpose2d's, ratio\n")
    print(f"{'buffer':>8s} {'valid':>8s} {'Cout':>5s} {'cin/split':>9s} | {'kernel':>10s} {'float32':>10s} {'ratio':>6s}")
    worst = (0.0, None)
    for h, w, valid in T.BUFFERS:
        for cout in T.COUTS:
            for ch in T.CHANNELS:
                e, e32 = T.measure(T.GPU, h, w, valid, cout, *ch)
                tag = (f"{h}x{w}", "all" if valid is None else f"{valid[0]}x{valid[1]}", cout, f"{ch[0]}/{ch[1]}")
                print(f"{tag[0]:>8s} {tag[1]:>8s} {tag[2]:5d} {tag[3]:>9s} | {e:10.3e} {e32:10.3e} {e / e32:6.2f}")
                worst = max(worst, (e / e32, tag))
    print(f"\nlargest ratio {worst[0]:.2f} at {worst[1]}: K_DGRAD = 2 x {worst[0]:.2f} = {2 * worst[0]:.2f}\n")

if what in ("time", "all"):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    n, h, cout = 32, 64, 64
    dy = E.Act(torch.randn(n, h, h, cout, device=dev, generator=g))
    c_in = torch.rand(n, device=dev, generator=g) + 0.5
    post = torch.tensor([2.0 ** -9], device=dev)
    print(f"time per launch, N = {n}, {h}x{h}, Cout = {cout}, {reps} launches between two HIP events")
    for name, cin, split, kw in (("denoiser 15 (12 | 3)", 15, 12, dict(scale_a=c_in, scale_b=2.0, post=post, swap_scales=True)),
                                 ("policy 3", 3, 3, dict(want_b=False, post=post)), ("rew/end 6 (3 | 3)", 6, 3, dict(post=post))):
        conv = nn.Conv2d(cin, cout, 3, padding=1).to(dev)
        fn = lambda: G.dgrad_input(dy, conv, split, **kw)
        fn(); fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        flop = 2.0 * 9 * cin * cout * n * h * h
        mma = 2.0 * 9 * 16 * cout * n * h * h  # (a group of 16 channels is computed whatever cin is)
        dx = torch.cat([t for t in out if t is not None], dim=1)
        print(f"  {name:22s} {us:8.1f} us  {flop / us / 1e6:6.2f} TFLOP/s algorithmic ({mma / us / 1e6:6.2f} issued)   sum {float(dx.double().sum()):+.9e}", flush=True)
