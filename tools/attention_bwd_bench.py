#!/usr/bin/env python
"""The attention backward's two routes side by side, in one process: the one-thread-per-token pair (dmd_attention_bwd) and the tiled
fp32-MFMA kernels (dmd_attention_bwd_mfma, full grid: H = 1, W = T).

Timing (default): us per call from HIP events around blocks of `--calls` launches, the two routes alternating over `--rounds` blocks
each; reported per shape: each route's median block, its block-to-block spread (max - min), the speed-up of the medians, whether
the new route is faster by more than the larger spread, and the new kernels' algorithmic TFLOP/s (112 FLOP per (query, key) pair and
head) as a fraction of the 157.3 TFLOP/s fp32 matrix peak.  Shapes (C = 64): N = 32, T = 256 (the default training step's);
N = 8, T = 1024; N = 8, T = 4096.  Prints one JSON line and writes it to --out (profiles/attention_bwd_mfma.json).

--precision: the error table of tests/test_attention_bwd_mfma.py's harder families (both routes on the same inputs, against float64
autograd, as a ratio to float32 CPU autograd's error, per third dq | dk | dv) -> --out (profiles/attention_bwd_mfma_precision.txt).
Run from the repository root."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 256), (8, 1024), (8, 4096)]
C = 64
PEAK_TFLOPS = 157.3


def box():
    p = torch.cuda.get_device_properties(0)
    return f"{p.name} ({p.gcnArchName.split(':')[0]}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


def timing(args):
    from diamond_amd import native as nv
    from diamond_amd import unet_train as UT

    L = nv.lib()
    out = {"what": "attention backward, us per call (both kernels of a route), C = 64, head_dim 8",
           "device": box(), "calls_per_block": args.calls, "blocks_per_route": args.rounds, "shapes": []}
    for n, t in SHAPES:
        g = torch.Generator().manual_seed(t)
        qkv = (torch.randn(n, t, 3 * C, generator=g) * 1.5).cuda()
        dy = torch.randn(n, t, C, generator=g).cuda()
        y = torch.empty(n, t, C, device="cuda")
        nv.check(L.dmd_attention(nv.fptr(qkv), nv.fptr(y), n, t, C, 8, nv.stream()), "dmd_attention")
        ws = torch.empty(int(L.dmd_attention_bwd_workspace_floats(n, t, C)), device="cuda")
        dq = {r: torch.empty_like(qkv) for r in ("scalar", "mfma")}
        a = [nv.fptr(x) for x in (qkv, y, dy)]
        launch = {"scalar": lambda: L.dmd_attention_bwd(*a, nv.fptr(dq["scalar"]), nv.fptr(ws), n, t, C, 8, nv.stream()),
                  "mfma": lambda: L.dmd_attention_bwd_mfma(*a, nv.fptr(dq["mfma"]), nv.fptr(ws), n, 1, t, 1, t, C, 8, nv.stream())}
        calls = max(2, args.calls // (16 if t >= 4096 else 1))
        blocks = {r: [] for r in launch}
        for r in launch:  # warm-up
            nv.check(launch[r](), r)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for r in launch:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    launch[r]()
                e1.record()
                torch.cuda.synchronize()
                blocks[r].append(e0.elapsed_time(e1) * 1e3 / calls)
        med = {r: statistics.median(v) for r, v in blocks.items()}
        spread = {r: max(v) - min(v) for r, v in blocks.items()}
        agree = float((dq["mfma"] - dq["scalar"]).abs().max() / dq["scalar"].abs().max())
        tflops = 112.0 * n * (C // 8) * t * t / (med["mfma"] * 1e-6) / 1e12
        out["shapes"].append({
            "N": n, "T": t, "calls_per_block": calls, "median_us": {r: round(v, 2) for r, v in med.items()},
            "block_spread_us": {r: round(v, 2) for r, v in spread.items()},
            "blocks_us": {r: [round(x, 2) for x in v] for r, v in blocks.items()},
            "speedup_of_medians": round(med["scalar"] / med["mfma"], 3),
            "mfma_faster_by_more_than_the_spread": med["scalar"] - med["mfma"] > max(spread.values()),
            "mfma_algorithmic_tflops": round(tflops, 2), "fraction_of_fp32_matrix_peak": round(tflops / PEAK_TFLOPS, 4),
            "routes_agree_to": agree})
    wins = [s["T"] for s in out["shapes"] if s["mfma_faster_by_more_than_the_spread"]]
    out["default_threshold"] = UT.ATTN_BWD_MFMA_MIN_T
    out["threshold_note"] = (f"the new route wins at T = {wins}; unet_train.ATTN_BWD_MFMA_MIN_T = {UT.ATTN_BWD_MFMA_MIN_T}: "
                             + ("256 .. 1023 valid tokens stay on the scalar pair although it is slower there, because the default 64x64 "
                                "training step's launch sequence (tests/golden/launch_sequences.json) and the 68x76 step's launch counts "
                                "(tests/test_offgrid_train.py, 17 x 19 = 323 valid tokens) are pinned to it; DIAMOND_ATTN_BWD_MIN_T=256 takes "
                                "the new route there" if 256 in wins and UT.ATTN_BWD_MFMA_MIN_T > 256 else "as measured"))
    return json.dumps(out)


def precision(args):
    from tests import test_attention_bwd_mfma as M
    from tests import attention_cases as A
    from tests import test_attention_precision as P

    lines = [f"dmd_attention_bwd_mfma against dmd_attention_bwd on the same inputs, {box()}",
             "N = 2, C = 24; error per (image, head) and third against float64 autograd, as a ratio to float32 CPU autograd's error;",
             "largest ratio over the (image, head) pairs, per third dq | dk | dv; y = forward: dmd_attention's output, truth: float32(float64)",
             "",
             f"{'family':>7} {'a':>4} {'T':>5} {'y':>8} | {'mfma dq':>8} {'dk':>7} {'dv':>7} | {'scalar dq':>9} {'dk':>7} {'dv':>7} | mfma > scalar"]
    worst = (0.0, "")
    for t in (64, 256, 1024):
        for family, a in A.BWD_CASES:
            for y_from in ("forward", "truth"):
                e, e32 = M.measure(M.GPU, t, family, a, y_from)
                s, _ = M.measure(M.GPU, t, family, a, y_from, run=P.GPU.attention_bwd)
                rm, rs = (e / e32).amax(dim=(0, 2)), (s / e32).amax(dim=(0, 2))
                over = [n for n, x, z in zip(("dq", "dk", "dv"), rm, rs) if float(x) > float(z)]
                lines.append(f"{family:>7} {a:>4} {t:>5} {y_from:>8} | {float(rm[0]):8.2f} {float(rm[1]):7.2f} {float(rm[2]):7.2f} | "
                             f"{float(rs[0]):9.2f} {float(rs[1]):7.2f} {float(rs[2]):7.2f} | {' '.join(over)}")
                if (family, a) != (1, 1.5) and float(rm.max()) > worst[0]:
                    worst = (float(rm.max()), f"family {family}, a = {a}, T = {t}, y = {y_from}")
    lines += ["", f"largest mfma ratio over the harder families (a = 4, 8, offset): {worst[0]:.2f} ({worst[1]})"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=32, help="launches per block (a sixteenth of it at T = 4096)")
    ap.add_argument("--rounds", type=int, default=10, help="blocks per route")
    ap.add_argument("--precision", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    text = precision(args) if args.precision else timing(args)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
