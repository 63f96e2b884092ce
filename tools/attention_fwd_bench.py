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

--f16x2-extent: the DEFAULT precision's routes off the tile grid, the same alternating-block timing: attention_kernel (what a valid
extent or a whole grid with T % 256 != 0 ran before dmd_attention_f16x2 existed: dmd_attention_valid over the padded grid /
dmd_attention; the comparator), dmd_attention_f16x2 (attention_f16x2_kernel over the valid tokens) and, for context, the f32 tiled
kernel; at T % 256 == 0 also dmd_attention, to which the new entry called as the whole-grid extent (1, T, 1, T) has to stay within
the block spread.  Shapes: the ones above plus 17 x 19 of 32 x 32 and the whole grids 320 and 576.  "derived_threshold" by the rule
above; engine.ATTN_F16X2_EXTENT_MIN_T ("default_threshold") has to be that number (tests/test_attention_f16x2_extent.py) -> --out
(profiles/attention_f16x2_extent.json).
--f16x2-precision: the error table of tests/test_attention_f16x2_extent.py's finite-input cases -> --out
(profiles/attention_f16x2_extent_precision.txt).
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


F16X2_SHAPES = SHAPES + [(8, 32, 32, 17, 19), (8, 1, 320, 1, 320), (8, 1, 576, 1, 576)]


# valid tokens of the 68 x 76 training step's upper attention level (18 x 20 of its 72 x 80 padded image), whose launches
# tests/test_offgrid_train.py pins to dmd_attention_valid on the interpreter: the default threshold stays above it
# (engine.ATTN_F16X2_EXTENT_MIN_T)
F16X2_PINNED_OLD_ROUTE_TOKENS = 360


def f16x2_default_threshold(shapes):
    """the smallest measured token count that is at least the derived threshold and above the pinned count; 0: none"""
    derived = derived_threshold(shapes)
    ok = [] if derived is None else sorted({s["valid_tokens"] for s in shapes if s["valid_tokens"] >= derived and s["valid_tokens"] > F16X2_PINNED_OLD_ROUTE_TOKENS})
    return ok[0] if ok else 0


def f16x2_threshold_fields(out, constant):
    """derived_threshold / default_threshold / threshold_note of a table, from its shapes"""
    shapes = out["shapes"]
    out["derived_threshold"] = derived_threshold(shapes)
    out["pinned_old_route_tokens"] = F16X2_PINNED_OLD_ROUTE_TOKENS
    out["default_threshold"] = constant
    wins = sorted({s["valid_tokens"] for s in shapes if s["faster_by_more_than_the_spread"]})
    loses = sorted({s["valid_tokens"] for s in shapes if not s["faster_by_more_than_the_spread"]})
    out["threshold_note"] = (f"dmd_attention_f16x2 beats attention_kernel by more than the block spread at {wins} valid tokens and not at {loses}: "
                             f"the table gives {out['derived_threshold']}; {F16X2_PINNED_OLD_ROUTE_TOKENS} tokens (the 68 x 76 training step, whose launches "
                             f"tests/test_offgrid_train.py pins) stay on the old route, so the default is the next measured count, "
                             f"{f16x2_default_threshold(shapes)}; engine.ATTN_F16X2_EXTENT_MIN_T = {constant}"
                             + ("" if f16x2_default_threshold(shapes) == constant else " -- THE CONSTANT DOES NOT FOLLOW FROM THIS TABLE"))
    return out


def timing_f16x2(args):
    from diamond_amd import engine as E
    from diamond_amd import native as nv

    L = nv.lib()
    out = {"what": "attention forward in default precision off the tile grid, us per call, C = 64, head_dim 8", "device": box(),
           "calls_per_block": args.calls, "blocks_per_route": args.rounds, "shapes": []}
    for n, h, w, vh, vw in F16X2_SHAPES:
        t, tv, full = h * w, vh * vw, (h == 1)
        g = torch.Generator().manual_seed(t + tv)
        qkv = (torch.randn(n, t, 3 * C, generator=g) * 1.5).cuda()
        on_grid = full and t % 256 == 0
        routes = ["f16x2_extent", "attention_kernel", "f32_tiled"] + (["split_f16x2"] if on_grid else [])
        y = {r: torch.zeros(n, t, C, device="cuda") for r in routes}
        # attention_kernel as the parent's default route reaches it: a valid extent through dmd_attention_valid over the padded grid,
        # a whole grid with T % 256 != 0 through dmd_attention; at T % 256 == 0 (never routed there) as a (T / 16, 16) grid, all valid
        if not full:
            comparator = lambda: L.dmd_attention_valid(nv.fptr(qkv), nv.fptr(y["attention_kernel"]), n, h, w, vh, vw, C, 8, nv.stream())
        elif on_grid:
            comparator = lambda: L.dmd_attention_valid(nv.fptr(qkv), nv.fptr(y["attention_kernel"]), n, t // 16, 16, t // 16, 16, C, 8, nv.stream())
        else:
            comparator = lambda: L.dmd_attention(nv.fptr(qkv), nv.fptr(y["attention_kernel"]), n, t, C, 8, nv.stream())
        launch = {"f16x2_extent": lambda: L.dmd_attention_f16x2(nv.fptr(qkv), nv.fptr(y["f16x2_extent"]), n, h, w, vh, vw, C, 8, nv.stream()),
                  "attention_kernel": comparator,
                  "f32_tiled": lambda: L.dmd_attention_f32(nv.fptr(qkv), nv.fptr(y["f32_tiled"]), n, h, w, vh, vw, C, 8, nv.stream()),
                  "split_f16x2": lambda: L.dmd_attention(nv.fptr(qkv), nv.fptr(y["split_f16x2"]), n, t, C, 8, nv.stream())}
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
        agree = float((grid(y["f16x2_extent"]) - grid(y["attention_kernel"])).abs().max() / grid(y["attention_kernel"]).abs().max())
        rec = {"N": n, "H": h, "W": w, "valid": [vh, vw], "valid_tokens": tv, "calls_per_block": calls,
               "median_us": {r: round(v, 2) for r, v in med.items()}, "block_spread_us": {r: round(v, 2) for r, v in spread.items()},
               "blocks_us": {r: [round(x, 2) for x in v] for r, v in blocks.items()},
               "speedup_over_attention_kernel": round(med["attention_kernel"] / med["f16x2_extent"], 3),
               "routes_agree_to": agree}
        # (the decision is taken on the rounded figures the record holds, so that the record can be checked against itself)
        m, sp = rec["median_us"], rec["block_spread_us"]
        rec["faster_by_more_than_the_spread"] = m["attention_kernel"] - m["f16x2_extent"] > max(sp["attention_kernel"], sp["f16x2_extent"])
        if on_grid:
            rec["bitwise_dmd_attention"] = bool(torch.equal(y["f16x2_extent"], y["split_f16x2"]))
            rec["on_grid_within_the_spread_of_dmd_attention"] = abs(m["f16x2_extent"] - m["split_f16x2"]) <= max(sp["f16x2_extent"], sp["split_f16x2"])
        out["shapes"].append(rec)
    f16x2_threshold_fields(out, E.ATTN_F16X2_EXTENT_MIN_T)
    return json.dumps(out)


F16X2_ONE_TOKEN_NOTE = """1x1x1x1 (above the on-grid kernel's 4.92): with ONE key every weight is 1 and the output is v itself, so a float32 evaluation makes
no error at all and the yardstick is its floor, 2^-24 of the head's max |v|.  The kernel's floor is ABSOLUTE: the fp16 pieces of v
stop at 2^-25 (the contract's "v far below 2^-3 is not rebalanced").  The worst head is the one whose V scale is 0.03: max |v| =
0.0336, error 1.96e-8 = 0.66 x 2^-25, which is 9.8 floors of that head (2^-25 itself would be 14.9).  It is the on-grid kernel's
family-7 floor seen without the averaging over keys that hides it at every T the on-grid kernel can run; nothing of the extent
handling enters (one key, one query; on the interpreter at C = 16, whose smallest max |v| is larger, the same case has 1.56)."""


def precision_f16x2(args):
    from tests import test_attention_f16x2_extent as X
    from tests import attention_cases as P

    arm = X.GPU
    lines = [f"dmd_attention_f16x2 (attention_f16x2_kernel over a valid extent), {box()}",
             f"N = {X.N}, C = {arm.c}; error per (image, head) against float64 of the cropped tensors as a ratio to max(float32 CPU evaluation's",
             f"error, 2^-24); largest ratio over the (image, head) pairs.  Margins NaN / +-Inf.  Bound: K_SPLIT = {P.K_SPLIT} (the on-grid kernel's,",
             "whose largest recorded ratio is 4.92: profiles/attention_precision.txt).",
             "", f"{'case':>24} {'extent':>14} {'tv':>5} | {'err':>10} {'fp32 err':>10} {'ratio':>6}"]
    worst = (0.0, "")
    cases = [("extent, 1 a=1.5", P.family_scale(X.N, arm.c, X.tokens(e), 1.5), e) for e in X.EXTENTS + X.GPU_ONLY_EXTENTS]
    cases += [(label, ref, X.PARTIAL) for label, ref in X.family_cases(X.tokens(X.PARTIAL), arm.c)]
    cases += [("5b mixed workgroups", P.family_mixed_workgroups(X.N, arm.c, X.tokens(X.ODD)), X.ODD),
              ("5 kv", P.family_range(X.N, arm.c, X.tokens(X.ODD), "kv"), X.ODD)]
    for label, ref, extent in cases:
        e, r = X.ratios(ref, X.on_extent(arm, ref.qkv, extent, arm.c))
        i = int(r.argmax())
        name = "x".join(map(str, extent))
        lines.append(f"{label:>24} {name:>14} {X.tokens(extent):>5} | {float(e.flatten()[i]):10.3e} {float(ref.e32.flatten()[i]):10.3e} {float(r.max()):6.2f}")
        if float(r.max()) > worst[0]:
            worst = (float(r.max()), f"{label}, {name}")
    lines += ["", f"largest ratio: {worst[0]:.4f} ({worst[1]}); the on-grid kernel's recorded largest: 4.92; K_SPLIT = {P.K_SPLIT}",
              "", F16X2_ONE_TOKEN_NOTE]
    return "\n".join(lines)


def precision(args):
    from tests import test_attention_f32_tiled as F
    from tests import attention_cases as P

    lines = [f"dmd_attention_f32 (attention_f32_tiled_kernel) beside attention_kernel on the same inputs, {box()}",
             f"N = {F.N}; error per (image, head) against float64 as a ratio to max(float32 CPU evaluation's error, 2^-24); largest ratio over",
             "the (image, head) pairs.  attention_kernel (dmd_attention_valid over the whole grid) needs T % 64 == 0.",
             "", f"{'family':>20} {'T':>5} {'C':>3} | {'tiled err':>10} {'fp32 err':>10} {'ratio':>6} | {'attention_kernel ratio':>22}"]
    worst = (0.0, "")
    for t, c in [(t, F.GPU.c) for t in F.TS] + [(1280, 64)]:
        for label, ref in list(F.precision_cases(t, c)) + ([("6a k, v = 1e5", F.beyond_fp16_case(t, c)[0])] if t == 256 else []):
            e, r = F.ratios(ref, F.GPU.attention(ref.qkv, c))
            i = int(r.argmax())
            other = f"{float(F.ratios(ref, F.GPU.other(ref.qkv, c, exact=True))[1].max()):22.2f}" if t % 64 == 0 else f"{'-':>22}"
            lines.append(f"{label:>20} {t:>5} {c:>3} | {float(e.flatten()[i]):10.3e} {float(ref.e32.flatten()[i]):10.3e} {float(r.max()):6.2f} | {other}")
            if float(r.max()) > worst[0]:
                worst = (float(r.max()), f"family {label}, T = {t}, C = {c}")
    for h, w, vh, vw in P.EXTENT_CASES:
        qkv, ref, _ = F.extent_inputs(h, w, vh, vw)
        e, r = F.ratios(ref, F.GPU.run(qkv, h, w, vh, vw, P.EXTENT_C)[:, :vh, :vw].reshape(P.EXTENT_N, vh * vw, P.EXTENT_C))
        i = int(r.argmax())
        lines.append(f"{f'extent {h}x{w}/{vh}x{vw}':>20} {vh * vw:>5} {P.EXTENT_C:>3} | {float(e.flatten()[i]):10.3e} {float(ref.e32.flatten()[i]):10.3e} "
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
    ap.add_argument("--f16x2-extent", action="store_true", help="dmd_attention_f16x2 against attention_kernel: timing table and threshold")
    ap.add_argument("--f16x2-precision", action="store_true", help="dmd_attention_f16x2: the error table")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    mode = precision if args.precision else timing_f16x2 if args.f16x2_extent else precision_f16x2 if args.f16x2_precision else timing
    text = mode(args)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
