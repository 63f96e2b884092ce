#!/usr/bin/env python
"""The exact attention forward's two routes side by side, in one process: attention_kernel (dmd_attention_valid, the online-softmax
kernel written for the 64-token level: the comparator) and attention_f32_tiled_kernel (dmd_attention_f32), with the split-fp16
two-pass kernel (dmd_attention, T % 256 == 0) for context.

Timing (default): us per call from HIP events around blocks of `--calls` launches, the routes alternating over `--rounds` blocks
each; reported per shape: each route's median block, its block-to-block spread (max - min), the speed-up of the medians, whether
the tiled kernel is faster than attention_kernel by more than the larger spread, and the tiled kernel's algorithmic TFLOP/s
(32 FLOP per (query, key) pair and head) as a fraction of the 157.3 TFLOP/s fp32 matrix peak.  Shapes (C = 64): N = 32, T = 256;
N = 8, T = 256; N = 8, T = 1024; N = 8, T = 4096; and two valid extents at N = 8: 18 x 20 (360 tokens) of a 32 x 32 grid and
36 x 36 (1296 tokens) of a 64 x 64 grid.  "derived_threshold" is the smallest measured token count from which the tiled kernel is
faster by more than the spread at every measured shape (null: at none); engine.ATTN_F32_TILED_MIN_T ("default_threshold") has to be
that number, and tests/test_attention_f32_tiled.py holds it to the file.  Prints one JSON line and writes it to --out
(profiles/attention_f32_tiled.json).

--qg LABEL=LIB,...: development builds of the library as further arms of the same alternating loop, recorded under
"query_groups_per_wave".  LABEL is <QG>u<U>: AT_QG = QG 16-query groups per wave, AT_UNROLL = U 16-key blocks of a whole tile per
loop iteration (U = 1: the rolled loop); each is built by
    touch diamond_amd/csrc/dmd_attention.hip && EXTRA_HIPCC_FLAGS="-DAT_QG=4 -DAT_UNROLL=2" bash diamond_amd/csrc/build.sh
and diamond_amd/libdiamond_hip.so copied aside (then once more without the flags for the shipped library, which is 2u4).

--precision: the error table of tests/test_attention_f32_tiled.py's finite-input families (dmd_attention_f32 and attention_kernel
on the same inputs against float64, as a ratio to the float32 CPU evaluation's error) -> --out
(profiles/attention_f32_tiled_precision.txt).
Run from the repository root."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, H, W, valid_h, valid_w): the full grid of T tokens is H = 1, W = T
SHAPES = [(32, 1, 256, 1, 256), (8, 1, 256, 1, 256), (8, 1, 1024, 1, 1024), (8, 1, 4096, 1, 4096), (8, 32, 32, 18, 20), (8, 64, 64, 36, 36)]
C = 64
PEAK_TFLOPS = 157.3
BWD_FRACTION = 0.37  # profiles/attention_bwd_mfma.json, T = 4096


def box():
    p = torch.cuda.get_device_properties(0)
    return f"{p.name} ({p.gcnArchName.split(':')[0]}, {p.multi_processor_count} CUs, {p.total_memory >> 30} GiB)"


def derived_threshold(shapes):
    """the smallest measured token count from which the tiled kernel wins by more than the spread at every measured shape"""
    counts = sorted({s["valid_tokens"] for s in shapes})
    ok = [t for t in counts if all(s["faster_by_more_than_the_spread"] for s in shapes if s["valid_tokens"] >= t)]
    return ok[0] if ok else None


def k_tiled(worst):
    """twice the largest measured ratio, rounded UP to two decimals"""
    import math

    return math.ceil(2.0 * worst * 100.0 - 1e-9) / 100.0


def timing(args):
    from diamond_amd import engine as E
    from diamond_amd import native as nv

    L = nv.lib()
    variants = {}
    for item in filter(None, (args.qg or "").split(",")):
        qg, path = item.split("=")
        lib = ctypes.CDLL(path)
        nv.declare_signatures(lib)
        variants[f"f32_tiled_qg{qg}"] = lib
    out = {"what": "attention forward, us per call, C = 64, head_dim 8", "device": box(), "calls_per_block": args.calls,
           "blocks_per_route": args.rounds, "shapes": []}
    for n, h, w, vh, vw in SHAPES:
        t, tv, full = h * w, vh * vw, (h == 1)
        g = torch.Generator().manual_seed(t + tv)
        qkv = (torch.randn(n, t, 3 * C, generator=g) * 1.5).cuda()
        routes = ["f32_tiled", "attention_kernel"] + (["split_f16x2"] if full and t % 256 == 0 else []) + (sorted(variants) if full else [])
        y = {r: torch.zeros(n, t, C, device="cuda") for r in routes}
        # attention_kernel walks the padded grid and masks: its full-grid extent is a (T / 16, 16) grid, all of it valid
        eh, ew, evh, evw = (t // 16, 16, t // 16, 16) if full else (h, w, vh, vw)
        launch = {"f32_tiled": lambda: L.dmd_attention_f32(nv.fptr(qkv), nv.fptr(y["f32_tiled"]), n, h, w, vh, vw, C, 8, nv.stream()),
                  "attention_kernel": lambda: L.dmd_attention_valid(nv.fptr(qkv), nv.fptr(y["attention_kernel"]), n, eh, ew, evh, evw, C, 8,
                                                                    nv.stream()),
                  "split_f16x2": lambda: L.dmd_attention(nv.fptr(qkv), nv.fptr(y["split_f16x2"]), n, t, C, 8, nv.stream())}
        for name, lib in variants.items():
            launch[name] = (lambda lib, name: lambda: lib.dmd_attention_f32(nv.fptr(qkv), nv.fptr(y[name]), n, h, w, vh, vw, C, 8,
                                                                          nv.stream()))(lib, name)
        calls = max(2, args.calls // (16 if tv >= 4096 else 1))
        blocks = {r: [] for r in routes}
        for r in routes:  # warm-up
            nv.check(launch[r](), r)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for r in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    launch[r]()
                e1.record()
                torch.cuda.synchronize()
                blocks[r].append(e0.elapsed_time(e1) * 1e3 / calls)
        med = {r: statistics.median(v) for r, v in blocks.items()}
        spread = {r: max(v) - min(v) for r, v in blocks.items()}
        grid = lambda x: x.reshape(n, h, w, C)[:, :vh, :vw]
        agree = float((grid(y["f32_tiled"]) - grid(y["attention_kernel"])).abs().max() / grid(y["attention_kernel"]).abs().max())
        tflops = 32.0 * n * (C // 8) * tv * tv / (med["f32_tiled"] * 1e-6) / 1e12
        # (two shapes may share a token count: every field that selects by it has to look at all of them)
        rec = {"N": n, "H": h, "W": w, "valid": [vh, vw], "valid_tokens": tv, "calls_per_block": calls,
               "median_us": {r: round(v, 2) for r, v in med.items()}, "block_spread_us": {r: round(v, 2) for r, v in spread.items()},
               "blocks_us": {r: [round(x, 2) for x in v] for r, v in blocks.items()},
               "speedup_over_attention_kernel": round(med["attention_kernel"] / med["f32_tiled"], 3),
               "faster_by_more_than_the_spread": med["attention_kernel"] - med["f32_tiled"] > max(spread["attention_kernel"],
                                                                                                 spread["f32_tiled"]),
               "f32_tiled_algorithmic_tflops": round(tflops, 2), "fraction_of_fp32_matrix_peak": round(tflops / PEAK_TFLOPS, 4),
               "routes_agree_to": agree}
        if variants and full:
            rec["query_groups_per_wave"] = {r[len("f32_tiled_qg"):]: round(med[r], 2) for r in sorted(variants)}
        out["shapes"].append(rec)
    out["derived_threshold"] = derived_threshold(out["shapes"])
    out["default_threshold"] = E.ATTN_F32_TILED_MIN_T
    wins = sorted({s["valid_tokens"] for s in out["shapes"] if s["faster_by_more_than_the_spread"]})
    loses = sorted({s["valid_tokens"] for s in out["shapes"] if not s["faster_by_more_than_the_spread"]})
    out["threshold_note"] = (f"the tiled kernel beats attention_kernel by more than the block spread at {wins} valid tokens and not at {loses}: "
                             f"the table gives {out['derived_threshold']}; engine.ATTN_F32_TILED_MIN_T = {E.ATTN_F32_TILED_MIN_T}"
                             + ("" if out["derived_threshold"] == E.ATTN_F32_TILED_MIN_T else " -- THE CONSTANT DOES NOT FOLLOW FROM THIS TABLE"))
    last = [s for s in out["shapes"] if s["valid_tokens"] == 4096 and s["H"] == 1][0]
    out["fraction_of_fp32_matrix_peak_at_4096"] = {"forward": last["fraction_of_fp32_matrix_peak"], "backward": BWD_FRACTION}
    return json.dumps(out)


def precision(args):
    from tests import test_attention_f32_tiled as F
    from tests import test_attention_precision as P

    lines = [f"dmd_attention_f32 (attention_f32_tiled_kernel) beside attention_kernel on the same inputs, {box()}",
             f"N = {F.N}; error per (image, head) against float64 as a ratio to max(float32 CPU evaluation's error, 2^-24); largest ratio over",
             "the (image, head) pairs.  attention_kernel (dmd_attention_valid over the whole grid) needs T % 64 == 0.",
             "", f"{'family':>20} {'T':>5} {'C':>3} | {'tiled err':>10} {'fp32 err':>10} {'ratio':>6} | {'attention_kernel ratio':>22}"]
    worst = (0.0, "")
    for t, c in [(t, F.GPU.c) for t in F.TS] + [(1280, 64)]:
        for label, ref in list(F.precision_cases(t, c)) + ([("6a k, v = 1e5", F.beyond_fp16_case(t, c)[0])] if t == 256 else []):
            e, r = F.ratios(ref, F.GPU.attention(ref.qkv, c))
            i = int(r.argmax())
            other = f"{float(F.ratios(ref, P.Gpu.attention(ref.qkv, c, exact=True))[1].max()):22.2f}" if t % 64 == 0 else f"{'-':>22}"
            lines.append(f"{label:>20} {t:>5} {c:>3} | {float(e.flatten()[i]):10.3e} {float(ref.e32.flatten()[i]):10.3e} {float(r.max()):6.2f} | {other}")
            if float(r.max()) > worst[0]:
                worst = (float(r.max()), f"family {label}, T = {t}, C = {c}")
    for h, w, vh, vw in F.V.CASES:
        qkv, ref, _ = F.extent_inputs(h, w, vh, vw)
        e, r = F.ratios(ref, F.GPU.run(qkv, h, w, vh, vw, F.V.C)[:, :vh, :vw].reshape(F.V.N, vh * vw, F.V.C))
        i = int(r.argmax())
        lines.append(f"{f'extent {h}x{w}/{vh}x{vw}':>20} {vh * vw:>5} {F.V.C:>3} | {float(e.flatten()[i]):10.3e} {float(ref.e32.flatten()[i]):10.3e} "
                     f"{float(r.max()):6.2f} | {'-':>22}")
        if float(r.max()) > worst[0]:
            worst = (float(r.max()), f"extent {h}x{w}/{vh}x{vw}")
    lines += ["", f"largest tiled ratio: {worst[0]:.4f} ({worst[1]}); K_TILED = twice that, rounded up to two decimals: "
                  f"{k_tiled(worst[0]):.2f} (tests/test_attention_f32_tiled.py has {F.K_TILED}); K_EXACT = {P.K_EXACT}"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=32, help="launches per block (a sixteenth of it at 4096 tokens)")
    ap.add_argument("--rounds", type=int, default=10, help="blocks per route")
    ap.add_argument("--qg", default=None, help="<QG>u<U>=LIB,...: development builds with -DAT_QG=QG -DAT_UNROLL=U as further arms (see above)")
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
