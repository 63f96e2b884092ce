"""The GroupNorm sites' numerics away from benign N(0.3, 1.5^2) inputs: every place the native code evaluates GroupNorm (groups of
C / max(1, C / 32) channels, eps 1e-5, optional FiLM and SiLU) -- the statistics kernels, conv_mfma_kernel's prologue and
residual_norm (norm_entry / norm_entry_gs / dmd_finalize_stats), conv_f16ws_kernel's producer tables and epilogue statistics,
the wgrad prologues, dmd_gn_silu_bwd, the 8x8 chains' own sums and finish_stats -- on the SIMT interpreter and on the device
(-m gpu), through the same C ABI, the same inputs and the same assertions.  Outputs start as NaN.

Inputs (tests/groupnorm_cases.py): an arm is one launch of N = 3 images of three different families, one of them benign; the
groups of an image carry different parameters, so a statistic from the wrong image or group is a wrong result.  Families: 1 small
spread (sigma 1e-1 .. 1e-4: variance above, at and below eps), 2 constant groups (0, 0.7, -3.25; a zero image), 3 offset (mean =
10, 30 sigma at sigma = 1 and 0.01), 4 one outlier of 1e4, 5 channel scales 1e-3 .. 1e3 inside a group, 6 FiLM edges (1 + mul = 0,
add = +-20, add = -100 under SiLU), 7 one NaN.  Truth is the operation in float64 over the float32 inputs; the measuring stick is
the same code in float32 on the CPU (F.group_norm on contiguous NCHW -- the channels-last kernel forms E[x^2] - mean^2 in float32
and is itself off by 6e-5 at mean = 30 sigma --, F.silu, F.conv2d, autograd).

Error: max |got - truth| / max |truth| per (image, 32-channel output block) for convolutions and chains, per (image, group) for
dx, per channel for dmul / dadd, per 32-channel group of the source for dw.
Bound: err <= K max(err_fp32, FLOOR) per block; K is a margin over the float32 reference, the project's precedent of
test_attention_precision.py, not lowered to the table's and never raised:

    kernels                                  K    FLOOR   largest measured ratio (MI355X = interpreter unless said)
    exact-fp32 forward (conv_mfma_kernel)    16   2^-24   4.04 (3x3, family 1); typical 0.3 .. 3
    split-fp16 forward (conv_f16ws_kernel,   10   2^-20   7.3 (two convolutions, r = 30, 16x16 geometry); prologue families
      conv_mfma SPLIT, the 8x8 chains)                    other than constant groups 0.2 .. 1.3 on the MI355X (interpreter 0.5 .. 3.2)
    backward (dmd_gn_silu_bwd, wgrad)        30   2^-24   15.6 (dmul, zero image + outlier, 15x20 valid 13x17); dx <= 2.5; wgrad <= 1.5

The statistics kernels are compared as (mean, rstd) formed in float64 from their sums: 1e-9 (mean in units of 1 / rstd), which
test_fp64_sums_give_mean_and_rstd_to_1e_9 first establishes for float64 sums in numpy on every family.
Every arm with sigma <= 1e-2 must SEE eps (check_sees_eps): the truth at eps 0, 1e-6 and 1e-4 differs from the truth by more than
100 x the bound on those rows.  With DMD_GN_EPS = 1e-6 70 of the 152 interpreter cases fail, with 1e-4 110 -- every site of every
test that has an eps; with norm_entry reading the neighbouring image's statistics, 80.

FINDINGS (profiles/groupnorm_precision.txt has the table; no kernel was changed, both are now stated in conv_f16ws_kernel's
header and include/diamond_hip.h and pinned here at the contract's edge):
  * conv_f16ws_kernel's producers evaluate fma(x, a, b), b = add - mean a rounded to float32.  A group CONSTANT at v != 0 has
    variance 0, rstd = 316, so b is rounded at 316 |v mul'|: test_conv_prologues[ws-*-small-const] measured 8.2e-6 .. 1.6e-5 of
    the output's scale where float32 has 1e-7 (ratio 8.0 .. 16.9 over FLOOR; the 64-channel 8x8 chain, same form: 4.2 on the
    MI355X, the 32-channel one 5.6), while every (x - mean) a path gives silu(add) to the last bit
    (test_constant_groups_are_silu_of_add_to_the_last_bit).  Contract: half an ulp of b, delta = 2^-24 (|mean| rstd |mul'| +
    |add|), on every normalised value of a channel; inside the plain bound up to |mean| rstd = 32 (family 3's mean = 30 sigma
    included: ratio <= 1.3); beyond it xab_allowance adds 2 x the root-sum-square of delta through the weights, sized from the
    table: the measured errors are 0.2 .. 1.37 of that root-sum-square, the limit of an affected row 2.3 .. 4.7 x its error.
    The producer is left as it is: (x - mean) a + add needs the mean in a fourth table row (LDS, four more registers per staging
    thread in geometries at the register cap) and changes the bits of every normalised convolution of the world model.  One more
    VALU instruction per element by itself (a build that subtracts a run-time zero) measured 13,357 against 13,375 frames/s
    over three alternating benchmark runs each, inside their +-0.3 % spread.
  * conv_f16ws_kernel's out_stats come from float32 sums of a lane's 16 (16x16 geometries) or 32 .. 64 outputs (8x8, fused
    projection: StatAcc = float, at the register cap).  The next prologue's rstd is off by 0.27 x 2^-24 (1 + r^2), r = |mean| /
    sigma: 1.66e-5 at r = 30 in WsGeom<true, 2, 9>, 1.2e-5 in the 16x16 geometries, 5e-6 with the fused projection, against 0
    from conv_mfma_kernel's float64 sums.  test_epilogue_statistics_feed_the_next_prologue: ratio 10.9 (MI355X) / 11.5
    (interpreter) in WsGeom<true, 2, 9> at r = 30, <= 7.3 everywhere else.  Contract: rstd to 2^-24 (1 + r^2), asserted of every
    geometry; the second convolution is held to the plain bound at every r except on the 8x8 geometries beyond r = 15, where
    the exact first-order effect of that rstd error (d out / d log rstd, computed in float64) is added.
Two facts of the dispatch shape the site list: dmd_conv1x1_stream_eligible rejects any prologue, so conv1x1_stream_kernel never
normalises (a 1x1 with a prologue is conv_mfma_kernel's, exact and SPLIT, or conv_f16ws_kernel<WsGeom<false, 2, 1>>: all three
are here); and dmd_conv2d_wgrad has no 3x3 instance with 32 output and 64 input channels, so the wgrad case is 64 -> 64 (two
groups per image; 32 -> 64 would have one).

What the interpreter cannot reproduce: expf / exp2f are the host libm's, v_rcp_f32 is an IEEE division there, and the order of
the sums inside an MFMA is its own -- the split-fp16 prologue rows differ by up to 3x between the runners for that reason.  The
epilogue's float32 partial sums and every float64 sum are the same bits on both: the two findings read the same on either."""
import functools
import math

import numpy as np
import pytest
import torch

from diamond_amd import native as nv  # struct layouts only
from tests import groupnorm_cases as GC
from tests.abi import RUNNERS, act_norm, check, kernel_sums, launch_conv, launch_gn_silu_bwd, launch_lowres_chain, nan_like, norm_struct
from tests.groupnorm_cases import FLOOR_EXACT, FLOOR_SPLIT, K_BWD, K_EXACT, K_SPLIT, rows_errors

STATS_TOL = 1e-9


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def image_blocks(x, block=32):
    """(N, ..., C) -> (N * C / block, M): one row per (image, `block`-channel block)"""
    n, c = x.shape[0], x.shape[-1]
    return x.reshape(n, -1, c // block, block).permute(0, 2, 1, 3).reshape(n * (c // block), -1)


def check_bound(run, site, arm, got, truth, stick, k, floor, rows=image_blocks, families=None, what="", allowance=None):
    """print the figures of the worst row of every family of the launch, then assert finiteness where the truth is finite and the
    bound on every row.  got / truth / stick: tensors of one layout; rows: that layout -> (B, M) with B a multiple of the images."""
    got, truth, stick = (torch.as_tensor(x) for x in (got, truth, stick))
    e, e32 = rows_errors(rows(got), rows(truth)), rows_errors(rows(stick), rows(truth))
    ratio = e / torch.clamp(e32, min=floor)
    limit = k * torch.clamp(e32, min=floor)
    if allowance is not None:  # a documented contract's term, relative to the row's scale like e
        limit = limit + allowance
    used = e / limit
    fams = families if families is not None else GC.FAMILY_OF[arm]
    per = used.reshape(len(fams), -1)
    for i in range(per.shape[0]):
        j = int(per[i].argmax()) + i * per.shape[1]
        print(f"GNPREC {run.name} {site}{what} arm={arm} family={fams[i]}: err {float(e[j]):.3e} fp32 {float(e32[j]):.3e} ratio {float(ratio[j]):.2f} "
              f"limit {float(limit[j]):.3e}")
    same = torch.isfinite(got) == torch.isfinite(truth)
    assert bool(same.all()), f"{int((~same).sum())} outputs are finite where the float64 restatement is not, or the reverse"
    assert float(used.max()) <= 1.0, (float(used.max()), ratio, limit)
    return limit


def sensitive_images(arm, c, shift):
    """images of the arm with a group of sigma <= 1e-2: every output of such an image sees eps"""
    return sorted({i for i, _ in GC.sees_eps(arm, c, shift)})


def check_sees_eps(truth_at, truth, bound, rows, row_ids):
    """the condition of this file: on the rows `row_ids` (sigma <= 1e-2) the truth recomputed with another eps differs from the
    truth by more than 100 x the bound -- an arm that could not tell eps = 1e-5 from 0, 1e-6 or 1e-4 would have to be replaced"""
    for eps in GC.OTHER_EPS:
        other = torch.as_tensor(truth_at(eps))
        d = rows(other.double() - torch.as_tensor(truth).double())
        d = torch.where(torch.isfinite(d), d.abs(), torch.full_like(d, math.inf)).amax(dim=1)
        s = torch.where(torch.isfinite(rows(truth)), rows(truth).abs(), torch.zeros_like(rows(truth))).amax(dim=1)
        for r in row_ids:
            assert float(d[r] / s[r]) > 100.0 * float(bound[r]), (eps, r, float(d[r] / s[r]), float(bound[r]))


# ---- statistics entry points -----------------------------------------------------------------------------------------------------------
STATS_SHAPES = [((8, 8, 64), None), ((8, 8, 48), None), ((16, 16, 64), (9, 13))]  # gn_stats_kernel, gn_stats_any_kernel, the valid extent


def stats_close(sums, a):
    m, r = GC.mean_rstd(sums, a.count())
    tm, tr = GC.true_mean_rstd(a.x, a.hv, a.wv)
    assert np.array_equal(np.isnan(m), np.isnan(tm)) and np.array_equal(np.isnan(r), np.isnan(tr))
    ok = ~np.isnan(tm)
    return float(np.max(np.abs(m - tm)[ok] * tr[ok])), float(np.max(np.abs(r / tr - 1.0)[ok]))


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("shape,valid", STATS_SHAPES, ids=["8x8x64", "8x8x48", "16x16x64-valid9x13"])
def test_fp64_sums_give_mean_and_rstd_to_1e_9(shape, valid, arm):
    """on the CPU, before anything is asserted of a kernel: sum and sum of squares in float64 (numpy) hold mean (in units of the
    group's 1 / rstd) and rstd to 1e-9 on every family, r = 30 included"""
    for shift in (0, 1):
        a = GC.act(arm, *shape, valid=valid, shift=shift)
        dm, dr = stats_close(a.sums(), a)
        assert dm <= STATS_TOL and dr <= STATS_TOL, (dm, dr)


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("shape,valid", STATS_SHAPES, ids=["8x8x64", "8x8x48", "16x16x64-valid9x13"])
@pytest.mark.parametrize("run", RUNNERS)
def test_statistics_kernels(run, shape, valid, arm):
    """gn_stats_kernel, gn_stats_any_kernel (48 channels: one group) and dmd_gn_stats_valid: (mean, rstd) formed in float64 from
    the kernel's sums against the two-pass float64 statistics, NaN exactly in the group that holds one"""
    for shift in (0, 1):
        a = GC.act(arm, *shape, valid=valid, shift=shift)
        dm, dr = stats_close(kernel_sums(run, a.x, *(valid or ())), a)
        print(f"GNPREC {run.name} gn_stats {shape} valid={valid} arm={arm} shift={shift}: mean off by {dm:.2e} / rstd, rstd by {dr:.2e}")
        assert dm <= STATS_TOL and dr <= STATS_TOL, (dm, dr)


# ---- forward convolutions ----------------------------------------------------------------------------------------------------------------
MFMA, WS = "conv_mfma_kernel<", "conv_f16ws_kernel<"
CONV_SITES = {
    # exact fp32, NORM_SILU + FiLM (plus_one); the 48-channel one is the general-group instance
    "mfma-3x3-c64": dict(h=8, w=16, cins=[64], cout=64, k=3, prologue=1, expect=MFMA + "ConvGeom<4, false, 9, 1, false>>"),
    "mfma-3x3-c48": dict(h=8, w=16, cins=[48], cout=48, k=3, prologue=1, expect=MFMA + "ConvGeomGN<1, false, 9, 1, false>>"),
    # residual_norm and a NORM prologue (the attention block's x_normed + out_proj(y))
    "mfma-1x1-resnorm": dict(h=8, w=16, cins=[64], cout=64, k=1, prologue=2, residual="norm", expect=MFMA + "ConvGeom<4, false, 1, 1, false>>"),
    # a normalised 1x1 (conv1x1_stream_kernel itself takes raw sources only: with a prologue the launch is conv_mfma_kernel's)
    "mfma-1x1-exact": dict(h=16, w=16, cins=[64], cout=64, k=1, prologue=2, expect=MFMA + "ConvGeom<4, false, 1, 1, false>>"),
    "mfma-1x1-split": dict(h=16, w=16, cins=[64], cout=64, k=1, prologue=2, precision=1, expect=MFMA + "ConvGeom<4, false, 1, 1, true>>"),
    "ws-false-2-9": dict(h=16, w=16, cins=[64], cout=64, k=3, prologue=1, precision=1, w16=True, stats=True, residual="raw",
                         expect=WS + "WsGeom<false, 2, 9>>"),
    "ws-true-2-9": dict(h=8, w=8, cins=[64], cout=64, k=3, prologue=1, precision=1, w16=True, stats=True, expect=WS + "WsGeom<true, 2, 9>>"),
    "ws-false-1-9": dict(h=16, w=16, cins=[32], cout=32, k=3, prologue=1, precision=1, w16=True, stats=True, residual="raw",
                         expect=WS + "WsGeom<false, 1, 9>>"),
    "ws-true-1-9": dict(h=8, w=8, cins=[32, 32], cout=32, k=3, prologue=1, precision=1, w16=True, stats=True, expect=WS + "WsGeom<true, 1, 9>>"),
    "ws-false-2-1": dict(h=16, w=16, cins=[64], cout=64, k=1, prologue=2, precision=1, w16=True, residual="raw", expect=WS + "WsGeom<false, 2, 1>>"),
    "ws-proj": dict(h=16, w=32, cins=[64], cout=64, k=3, prologue=1, precision=1, w16=True, stats=True, proj=True, expect=WS + "WsGeomProj>"),
}


def bounds_of(site):
    return (K_SPLIT, FLOOR_SPLIT) if site.get("precision") else (K_EXACT, FLOOR_EXACT)


def shifts_of(c):
    return (0,) if GC.groups_of(c) > 1 else (0, 1)


@functools.lru_cache(maxsize=None)
def conv_case(name, arm, shift):
    """inputs, float64 truth at any eps and float32 stick of one launch (computed once, shared by the runners, never written to)"""
    s = CONV_SITES[name]
    rng = np.random.default_rng([sum(map(ord, name)), shift])
    h, w, cins, cout, k, pro = s["h"], s["w"], s["cins"], s["cout"], s["k"], s["prologue"]
    acts = [GC.act(arm, h, w, c, plus_one=pro == 1, shift=shift, seed=i) for i, c in enumerate(cins)]
    n = acts[0].n
    case = dict(acts=acts, w=GC.conv_weight(rng, cout, sum(cins), k), bias=rng.standard_normal(cout).astype(np.float32), res=None, rn=None, proj=None)
    if s.get("residual") == "raw":
        case["res"] = rng.standard_normal((n, h, w, cout)).astype(np.float32)
    if s.get("residual") == "norm":
        case["rn"] = GC.act(arm, h, w, cout, plus_one=False, shift=shift, seed=7)
    if s.get("proj"):
        case["proj"] = (rng.standard_normal((n, h, w, 64)).astype(np.float32), rng.standard_normal((n, h, w, 64)).astype(np.float32),
                        GC.conv_weight(rng, cout, 128, 1), rng.standard_normal(cout).astype(np.float32))

    def formula(dtype, eps=GC.EPS):
        y = GC.conv([a.normalised(dtype, pro == 1, eps) for a in acts], case["w"], case["bias"], dtype)
        if case["res"] is not None:
            y = y + GC.tt(case["res"], dtype).permute(0, 3, 1, 2)
        if case["rn"] is not None:
            y = y + case["rn"].normalised(dtype, False, eps)
        if case["proj"] is not None:
            j0, j1, wp, bp = case["proj"]
            y = y + GC.conv([GC.tt(j, dtype).permute(0, 3, 1, 2) for j in (j0, j1)], wp, bp, dtype)
        return GC.nhwc(y)

    case["formula"], case["truth"], case["stick"] = formula, formula(torch.float64), formula(torch.float32)
    return case


XAB_EDGE = 32.0  # |mean| rstd up to which conv_f16ws_kernel's x * a + b producer is held to the plain bound (its header's contract)
XAB_SIGMAS = 2.0  # x the root-sum-square below; the largest measured is 1.37 (WsGeom<false, 2, 1>), 0.2 .. 0.9 on the 3x3 geometries


def xab_allowance(case, truth, rows):
    """The contract of the split-fp16 producer (dmd_conv_f16ws.hip's header, include/diamond_hip.h), as an error per row relative
    to the row's scale.  It evaluates the normalisation as fma(x, a, b) with b = add - mean a rounded to float32: half an ulp of b,
    at most delta = 2^-24 (|mean a| + |add|), on every normalised value of a channel.  Counted only for groups with |mean| rstd >
    XAB_EDGE (constant groups away from zero: rstd = 316); up to the edge -- mean = 30 sigma included -- the plain bound holds.
    In a constant group the error e_c of channel c is the same at every pixel, uniform in +-delta_c, and independent between
    channels; an output gets sum_c e_c sum_taps w (|SiLU'| <= 1.1 left out: it is below 1 where it matters), and a sum over
    the taps of a 3x3 is of the size of their root-sum-square.  So the term is XAB_SIGMAS x sqrt(sum_c delta_c^2 sum_taps w^2):
    with the standard deviation delta / sqrt(3) of a uniform error that is 3.5 sigma of the output's error, what the largest of
    the few thousand outputs of a block reaches.  Measured on the MI355X: 0.2 .. 0.9 of the root-sum-square on the 3x3
    geometries, 0.8 .. 1.37 on the 1x1 (profiles/groupnorm_precision.txt), so the limit of an affected row is 2.3 .. 4.7 x
    its measured error -- not the worst case sum |w| delta, which would be 20 .. 90 x."""
    w2 = (case["w"].astype(np.float64) ** 2).sum(axis=(2, 3))  # (Cout, Cin)
    delta = []
    for a in case["acts"]:
        m, r = GC.true_mean_rstd(a.x, a.hv, a.wv)
        gs = a.c // GC.groups_of(a.c)
        mr = np.repeat(np.nan_to_num(np.abs(m) * r), gs, axis=1)  # (N, C)
        f = np.abs(1.0 + a.mul.astype(np.float64)) if a.plus_one else np.abs(a.mul.astype(np.float64))
        delta.append(np.where(mr > XAB_EDGE, 2.0 ** -24 * (mr * f + np.abs(a.add.astype(np.float64))), 0.0))
    out = XAB_SIGMAS * np.sqrt((np.concatenate(delta, axis=1) ** 2) @ w2.T)  # (N, Cout)
    scale = torch.where(torch.isfinite(rows(truth)), rows(truth).abs(), torch.zeros_like(rows(truth))).amax(dim=1)
    rss = rows(torch.tensor(out)[:, None, :]).amax(dim=1)
    return torch.where(scale > 0, rss / scale.clamp_min(1e-300), torch.zeros_like(scale))


def run_conv_case(run, name, case, expect=True):
    s = CONV_SITES[name]
    srcs = [(a.x, s["prologue"], functools.partial(lambda r, keep, a: act_norm(r, keep, a), a=a)) for a in case["acts"]]
    return launch_conv(run, srcs, case["w"], case["bias"], precision=s.get("precision", 0), w16=s.get("w16", False), residual=case["res"],
                       residual_norm=case["rn"], want_stats=s.get("stats", False), proj=case["proj"], expect=s["expect"] if expect else None)


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("name", CONV_SITES)
@pytest.mark.parametrize("run", RUNNERS)
def test_conv_prologues(run, name, arm):
    """every family through every forward site that normalises: per (image, 32-channel output block) within K x the float32 error;
    non-finite exactly where the float64 restatement is; the arms with sigma <= 1e-2 see eps"""
    s = CONV_SITES[name]
    k, floor = bounds_of(s)
    for shift in shifts_of(s["cins"][0]):
        case = conv_case(name, arm, shift)
        got, stats = run_conv_case(run, name, case)
        block = 32 if s["cout"] % 32 == 0 else s["cout"]
        rows = functools.partial(image_blocks, block=block)
        allowance = xab_allowance(case, case["truth"], rows) if name.startswith("ws-") else None
        bound = check_bound(run, name, arm, got, case["truth"], case["stick"], k, floor, rows=rows, what=f" shift={shift}" if shift else "",
                            allowance=allowance)
        nb = s["cout"] // block
        ids = [i * nb + b for i in sensitive_images(arm, s["cins"][0], shift) for b in range(nb)]
        check_sees_eps(lambda eps: case["formula"](torch.float64, eps), case["truth"], bound, rows, ids)
        if stats is not None and arm != "nan":  # the epilogue's sums describe the output the kernel wrote
            m, r = GC.mean_rstd(stats, float(s["h"] * s["w"] * 32))
            tm, tr = GC.true_mean_rstd(got, s["h"], s["w"])
            ratio = np.abs(tm) * GC.true_mean_rstd(got, s["h"], s["w"], eps=0.0)[1]  # |mean| / sigma of the output groups
            dr, dm = np.abs(r / tr - 1.0), np.abs(m - tm) * tr
            print(f"GNPREC {run.name} {name} arm={arm}: epilogue rstd off by {float(dr.max()):.2e} = "
                  f"{float((dr / epilogue_rstd_contract(ratio)).max()):.2f} x 2^-24 (1 + r^2), mean by {float(dm.max()):.2e} / rstd")
            assert bool((dr <= epilogue_rstd_contract(ratio)).all()) and bool((dm <= 2.0 ** -24 * (1.0 + ratio)).all()), (dr, dm, ratio)


@pytest.mark.parametrize("run", RUNNERS)
def test_constant_groups_are_silu_of_add_to_the_last_bit(run):
    """Family 2 on a path that forms (x - mean) * a: conv_mfma_kernel (exact fp32) with the identity as its 1x1 weight.  Groups
    constant at 0.7 and -3.25 give bit for bit what a zero image gives under the same FiLM rows -- silu(add) as the kernel
    evaluates it, since (x - mean) is exactly 0 -- and that is silu(add) to float32 rounding."""
    rng = np.random.default_rng(5)
    n, h, w, c = 3, 8, 16, 64
    x = (rng.standard_normal((n, h, w, c)) * 1.5 + 0.3).astype(np.float32)
    x[0, ..., :32], x[0, ..., 32:], x[1] = 0.7, -3.25, 0.0
    mul, add = (rng.standard_normal((n, c)) * 0.3).astype(np.float32), (rng.standard_normal((n, c)) * 0.3).astype(np.float32)
    mul[1], add[1] = mul[0], add[0]
    eye = np.eye(c, dtype=np.float32).reshape(c, c, 1, 1)
    norm = lambda r, keep: norm_struct(r, keep, kernel_sums(r, x), mul, add, True)
    got, _ = launch_conv(run, [(x, 1, norm)], eye, np.zeros(c, dtype=np.float32), expect=MFMA + "ConvGeom<4, false, 1, 1, false>>")
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    want = add[0].astype(np.float64) / (1.0 + np.exp(-add[0].astype(np.float64)))
    assert np.all(np.abs(got[1] - want) <= 4 * 2.0 ** -24 * np.maximum(np.abs(want), np.abs(add[0]))), np.abs(got[1] - want).max()
    assert np.isfinite(got).all()


# ---- epilogue statistics -> next prologue ------------------------------------------------------------------------------------------------
CHAIN_SITES = ["mfma-3x3-c64", "ws-false-2-9", "ws-true-2-9", "ws-false-1-9", "ws-true-1-9", "ws-false-2-1", "ws-proj"]


STATS_EDGE = 15.0  # |mean| / sigma up to which statistics from the 8x8 geometries' float32 partial sums are held to the plain bound


def epilogue_rstd_contract(r):
    """conv_f16ws_kernel's out_stats (dmd_conv_f16ws.hip's header, include/diamond_hip.h): a lane's 16 .. 64 outputs are summed in
    float32 before the float64 sums, so rstd is that of a mean square rounded once to float32: off by up to 2^-24 (1 + r^2),
    r = |mean| / sigma of the output group"""
    return 2.0 ** -24 * (1.0 + np.asarray(r, dtype=np.float64) ** 2)


@functools.lru_cache(maxsize=None)
def chain_case(name, shift):
    s = CONV_SITES[name]
    rng = np.random.default_rng([sum(map(ord, name)), shift, 99])
    h, w, cins, cout, k, pro = s["h"], s["w"], s["cins"], s["cout"], s["k"], s["prologue"]
    n = len(GC.IMAGE_SCALE)
    xs = [GC.dyadic_input(rng, (n, h, w, c)) for c in cins]
    w1, b1, kinds, claims = GC.chain_first_conv(rng, cout, sum(cins), k, shift)
    proj = None
    if s.get("proj"):  # the projection lands in the same accumulators: the same kind of weights per group
        proj = (GC.dyadic_input(rng, (n, h, w, 64)), GC.dyadic_input(rng, (n, h, w, 64)), GC.sparse_dyadic_weight(rng, cout, 128, 1, kinds),
                np.zeros(cout, dtype=np.float32))
    w2, b2 = GC.conv_weight(rng, cout, cout, k), rng.standard_normal(cout).astype(np.float32)
    m = (rng.standard_normal((n, cout)) * 0.3).astype(np.float32)
    mul, add = (m if pro == 1 else (1.0 + m).astype(np.float32)), (rng.standard_normal((n, cout)) * 0.3).astype(np.float32)

    def first(dtype):
        t = lambda a: GC.tt(a, dtype).permute(0, 3, 1, 2)
        y1 = GC.conv([t(x) for x in xs], w1, b1, dtype)
        return y1 if proj is None else y1 + GC.conv([t(j) for j in proj[:2]], proj[2], proj[3], dtype)

    def formula(dtype, eps=GC.EPS):
        return GC.nhwc(GC.conv([GC.norm_act(first(dtype), GC.tt(mul, dtype), GC.tt(add, dtype), pro == 1, pro == 1, eps)], w2, b2, dtype))

    mid = GC.nhwc(first(torch.float64))
    assert bool((mid == GC.nhwc(first(torch.float32)).double()).all())  # exact in float32: nothing of the first convolution's is measured
    # the family is what it claims: statistics of the float64 intermediate, per (image, group)
    tm, tr = GC.true_mean_rstd(mid.numpy(), h, w, eps=0.0)
    sens = []
    for i, si in enumerate(GC.IMAGE_SCALE):
        for j, (sig, mean) in enumerate(claims):
            sd = 1.0 / tr[i, j]
            assert 0.5 <= sd / (sig * si * (math.sqrt(2.0) if proj is not None else 1.0)) <= 2.0, (i, j, sd)
            assert abs(tm[i, j] - mean) <= 0.3 * sd, (i, j, tm[i, j], sd)
            if mean == 0.0 and sd <= 1e-2:
                sens.append(i)
    truth = formula(torch.float64)
    # d out / d log rstd of every (image, group), exactly: what a relative error of the epilogue's rstd does to the second output
    y1 = first(torch.float64)
    xn = torch.nn.functional.group_norm(y1, GC.groups_of(cout), eps=GC.EPS)
    mm = (1.0 + GC.tt(mul, torch.float64)) if pro == 1 else GC.tt(mul, torch.float64)
    d = xn * mm[:, :, None, None]
    if pro == 1:
        t = d + GC.tt(add, torch.float64)[:, :, None, None]
        sg = torch.sigmoid(t)
        d = d * sg * (1.0 + t * (1.0 - sg))
    r = np.abs(tm) * tr  # (N, G): |mean| / sigma
    scale = image_blocks(truth).abs().amax(dim=1)
    stats_allowance = torch.zeros_like(scale)
    for j in range(GC.groups_of(cout)):
        dj = torch.zeros_like(d)
        dj[:, 32 * j:32 * j + 32] = d[:, 32 * j:32 * j + 32]
        x_of = torch.tensor(np.where(r[:, j] > STATS_EDGE, epilogue_rstd_contract(r[:, j]), 0.0))
        stats_allowance += image_blocks(GC.nhwc(GC.conv([dj], w2, None, torch.float64)).abs() * x_of[:, None, None, None]).amax(dim=1) / scale
    return dict(xs=xs, w1=w1, b1=b1, proj=proj, w2=w2, b2=b2, mul=mul, add=add, formula=formula, mid=mid.numpy(), truth=truth,
                stick=formula(torch.float32), sens=sorted(set(sens)), r=r, stats_allowance=stats_allowance)


@pytest.mark.parametrize("name", CHAIN_SITES)
@pytest.mark.parametrize("run", RUNNERS)
def test_epilogue_statistics_feed_the_next_prologue(run, name):
    """two convolutions in a row: the first with out_stats, its output -- exact by construction, see groupnorm_cases -- in families
    1 (mean 0, sigma = 0.0039 .. 0.0156) and 3 (mean 15, r = 7.5, 15, 30); the second normalises with exactly those statistics"""
    s = CONV_SITES[name]
    k, floor = bounds_of(s)
    for shift in (0, 1):
        c = chain_case(name, shift)
        kw = dict(precision=s.get("precision", 0), w16=s.get("w16", False))
        mid, st = launch_conv(run, [(x, 0, None) for x in c["xs"]], c["w1"], c["b1"], want_stats=True, proj=c["proj"],
                              expect=s["expect"].replace("ConvGeomGN", "ConvGeom"), **kw)
        assert np.array_equal(mid.astype(np.float64), c["mid"]), "the first convolution is not exact"
        m, r = GC.mean_rstd(st, float(s["h"] * s["w"] * 32))
        tm, tr = GC.true_mean_rstd(mid, s["h"], s["w"])
        dr, dm = np.abs(r / tr - 1.0), np.abs(m - tm) * tr
        print(f"GNPREC {run.name} chain-{name} shift={shift}: epilogue rstd off by {float(dr.max()):.2e} = {float((dr / epilogue_rstd_contract(c['r'])).max()):.2f}"
              f" x 2^-24 (1 + r^2), mean by {float(dm.max()):.2e} / rstd")
        # the statistics describe the output the kernel wrote: float64 sums (conv_mfma_kernel) / the epilogue's contract (conv_f16ws_kernel)
        assert bool((dr <= (epilogue_rstd_contract(c["r"]) if name.startswith("ws-") else STATS_TOL)).all()) and float(dm.max()) <= 1e-6, (dr, dm)
        norm = lambda rr, keep: norm_struct(rr, keep, st, c["mul"], c["add"], s["prologue"] == 1)
        got, _ = launch_conv(run, [(mid, s["prologue"], norm)], c["w2"], c["b2"], **kw)
        fams = tuple("1+3" for _ in GC.IMAGE_SCALE)
        # beyond STATS_EDGE the 8x8 geometries (float32 partial sums up to the wave reduction: at the register cap) are held to the
        # plain bound plus what their contract's rstd error does to this output; every other site to the plain bound at every r
        allowance = c["stats_allowance"] if name.startswith("ws-true") else None
        bound = check_bound(run, "chain-" + name, f"shift{shift}", got, c["truth"], c["stick"], k, floor, families=fams, allowance=allowance)
        nb = s["cout"] // 32
        check_sees_eps(lambda eps: c["formula"](torch.float64, eps), c["truth"], bound, image_blocks, [i * nb + b for i in c["sens"] for b in range(nb)])


# ---- wgrad with a normalised source ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_case(arm):
    rng = np.random.default_rng(17)
    a = GC.act(arm, 8, 16, 64, plus_one=True)
    dy = rng.standard_normal((a.n, 8, 16, 64)).astype(np.float32)

    def formula(dtype, eps=GC.EPS):
        w = torch.zeros(64, 64, 3, 3, dtype=dtype, requires_grad=True)
        y = torch.nn.functional.conv2d(a.normalised(dtype, True, eps), w, padding=1)
        y.backward(GC.tt(dy, dtype).permute(0, 3, 1, 2))
        return w.grad

    return a, dy, formula, formula(torch.float64), formula(torch.float32)


def cin_groups(dw):
    """(Cout, Cin, k, k) -> (Cin / 32, M): one row per normalised group of the source"""
    co, ci, k, _ = dw.shape
    return dw.reshape(co, ci // 32, 32 * k * k).permute(1, 0, 2).reshape(ci // 32, -1)


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("precision", [0, 1], ids=["exact", "split"])
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_with_a_normalised_source(run, precision, arm):
    """dmd_conv2d_wgrad, 8x16, 64 -> 64, 3x3 (two groups per image),
    source under NORM_SILU + FiLM: dw per 32-channel group of the source (the three
    images are summed: a statistic from the wrong image still is a wrong sum) against float64 autograd"""
    a, dy, formula, truth, stick = wgrad_case(arm)
    L, keep = run.lib(), []
    p = nv.WgradParams()
    p.N, p.H, p.W, p.Cout, p.taps, p.cin_real, p.precision = a.n, a.h, a.w, 64, 9, 64, precision
    hs = [run.put(a.x), run.put(dy), run.put(nan_like((64, 64, 3, 3))), run.put(nan_like(64))]
    p.src.x, p.src.C, p.src.prologue, p.src.norm = run.ptr(hs[0]), 64, 1, act_norm(run, keep, a)
    p.dy, p.dw, p.dbias = run.ptr(hs[1]), run.ptr(hs[2]), run.ptr(hs[3])
    ws = run.put(nan_like(int(L.dmd_wgrad_workspace_floats(p))))
    p.workspace = run.ptr(ws)
    check(run, L.dmd_conv2d_wgrad(p, run.stream()), "dmd_conv2d_wgrad")
    got = torch.from_numpy(run.get(hs[2]))
    k, floor = K_BWD, (FLOOR_SPLIT if precision else FLOOR_EXACT)
    fams = ("+".join(str(f) for f in GC.FAMILY_OF[arm]),)
    bound = check_bound(run, "wgrad-" + ("split" if precision else "exact"), arm, got, truth, stick, k, floor, rows=cin_groups, families=fams)
    check_sees_eps(lambda eps: formula(torch.float64, eps), truth, bound, cin_groups, sorted({j for _, j in GC.sees_eps(arm, 64)}))


# ---- dmd_gn_silu_bwd ---------------------------------------------------------------------------------------------------------------------
BWD_SITES = {"c64-8x8-skip": dict(h=8, w=8, c=64, skip=True), "c32-15x20-valid13x17": dict(h=15, w=20, c=32, valid=(13, 17)), "c48-8x8": dict(h=8, w=8, c=48)}


@functools.lru_cache(maxsize=None)
def bwd_case(name, arm, shift):
    s = BWD_SITES[name]
    rng = np.random.default_rng([sum(map(ord, name)), shift, 3])
    a = GC.act(arm, s["h"], s["w"], s["c"], plus_one=True, valid=s.get("valid"), shift=shift)
    da = rng.standard_normal(a.x.shape).astype(np.float32)
    dskip = rng.standard_normal(a.x.shape).astype(np.float32) if s.get("skip") else None

    def formula(dtype, eps=GC.EPS):
        x, mul, add = (GC.tt(t, dtype).requires_grad_(True) for t in (a.x, a.mul, a.add))
        y = GC.norm_act(x[:, :a.hv, :a.wv].permute(0, 3, 1, 2), mul, add, True, True, eps)
        y.backward(GC.tt(da[:, :a.hv, :a.wv], dtype).permute(0, 3, 1, 2))
        dx = x.grad[:, :a.hv, :a.wv]
        if dskip is not None:
            dx = dx + GC.tt(dskip[:, :a.hv, :a.wv], dtype)
        return dx.contiguous(), mul.grad, add.grad

    return a, da, dskip, formula, formula(torch.float64), formula(torch.float32)


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("name", BWD_SITES)
@pytest.mark.parametrize("run", RUNNERS)
def test_gn_silu_bwd(run, name, arm):
    """dx per (image, group), dmul / dadd per channel, against float64 autograd of silu(group_norm(x) * (1 + mul) + add); a zero
    image gives finite gradients; nothing is written outside the valid extent"""
    s = BWD_SITES[name]
    for shift in shifts_of(s["c"]):
        a, da, dskip, formula, truth, stick = bwd_case(name, arm, shift)
        c = a.c
        dx, dmul, dadd = launch_gn_silu_bwd(run, a, da, dskip, valid=bool(s.get("valid")))
        if s.get("valid"):
            assert not dx[:, a.hv:].any() and not dx[:, :, a.wv:].any()
        dx = torch.from_numpy(np.ascontiguousarray(dx[:, :a.hv, :a.wv]))
        gs = c // GC.groups_of(c)
        tag = f" shift={shift}" if shift else ""
        bound = check_bound(run, "bwd-" + name, arm, dx, truth[0], stick[0], K_BWD, FLOOR_EXACT, rows=functools.partial(image_blocks, block=gs),
                            what=" dx" + tag)
        channels = lambda t: t.t()  # (N, C) -> one row per channel
        fams = ("+".join(str(f) for f in GC.FAMILY_OF[arm]),)
        check_bound(run, "bwd-" + name, arm, torch.from_numpy(dmul), truth[1], stick[1], K_BWD, FLOOR_EXACT, rows=channels, families=fams, what=" dmul" + tag)
        check_bound(run, "bwd-" + name, arm, torch.from_numpy(dadd), truth[2], stick[2], K_BWD, FLOOR_EXACT, rows=channels, families=fams, what=" dadd" + tag)
        g = GC.groups_of(c)
        ids = [i * g + j for i, j in GC.sees_eps(arm, c, shift)]
        check_sees_eps(lambda eps: formula(torch.float64, eps)[0], truth[0], bound, functools.partial(image_blocks, block=gs), ids)


# ---- the 8x8 chains ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lowres_case(c, arm, shift):
    rng = np.random.default_rng([41, c, shift])
    a = GC.act(arm, 8, 8, c, plus_one=True, shift=shift)
    n = a.n
    specs = [dict(cat=False, attn=False, save=1 if c == 64 else -1), dict(cat=False, attn=True, save=-1)]
    if c == 64:
        specs.append(dict(cat=True, attn=True, save=-1))
    film = lambda ch: ((rng.standard_normal((n, ch)) * 0.3).astype(np.float32), (rng.standard_normal((n, ch)) * 0.3).astype(np.float32))
    vec = lambda m, s=1.0: (rng.standard_normal(m) * s).astype(np.float32)
    blocks = []
    for i, sp in enumerate(specs):
        cin = 2 * c if sp["cat"] else c
        b = dict(sp, w1=GC.conv_weight(rng, c, cin, 3), w2=GC.conv_weight(rng, c, c, 3), b1=vec(c), b2=vec(c), f1=film(cin), f2=film(c))
        if i == 0:
            b["f1"] = (a.mul, a.add)  # the chain input's own normalisation carries the arm's FiLM rows (family 6)
        if sp["cat"]:
            b["wp"], b["bp"] = GC.conv_weight(rng, c, cin, 1), vec(c)
        if sp["attn"]:
            b.update(wqkv=GC.conv_weight(rng, 3 * c, c, 1), bqkv=vec(3 * c, 0.2), wo=GC.conv_weight(rng, c, c, 1), bo=vec(c),
                     gam=(1 + 0.2 * rng.standard_normal(c)).astype(np.float32), bet=vec(c, 0.2))
        blocks.append(b)
    formula = lambda dtype, eps=GC.EPS: GC.lowres_chain(a.x, blocks, dtype, eps)
    return a, blocks, formula, formula(torch.float64), formula(torch.float32)


@pytest.mark.parametrize("arm", GC.ARMS)
@pytest.mark.parametrize("c", [64, 32], ids=["chain64", "chain32"])
@pytest.mark.parametrize("run", RUNNERS)
def test_lowres_chains(run, c, arm):
    """dmd_lowres_chain (three blocks: plain, attention, cat + projection + attention) and dmd_lowres_chain32 (two blocks) with the
    families at the chain input: the chains' own sums and their two private finish_stats"""
    for shift in shifts_of(c):
        a, blocks, formula, truth, stick = lowres_case(c, arm, shift)
        got = launch_lowres_chain(run, a.x, blocks)
        bound = check_bound(run, f"chain{c}", arm, got, truth, stick, K_SPLIT, FLOOR_SPLIT, what=f" shift={shift}" if shift else "")
        nb = c // 32
        ids = [i * nb + j for i in sensitive_images(arm, c, shift) for j in range(nb)]
        check_sees_eps(lambda eps: formula(torch.float64, eps), truth, bound, image_blocks, ids)
