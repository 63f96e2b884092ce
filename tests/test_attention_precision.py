"""The attention kernels' numerics away from benign N(0, 1.5^2) inputs: dmd_attention (attention_kernel, exact fp32, for T % 256 != 0;
attention_f16x2_kernel, split-fp16 operands in two passes over the keys, for T % 256 == 0), dmd_attention_bwd on the forward it
gets in training, on the SIMT interpreter (small shapes) and on the device (-m gpu).

Truth is softmax(q k^T / sqrt(8)) v per head in float64 over the float32 inputs; the measuring stick is the same formula in float32
on the CPU.  The error is taken per (image, head): max over queries and dims of |got - truth| / max|v| of that (image, head), and
every (image, head) has its own V scale (0.03 .. 30, shuffled), so a result in the wrong head or image, or an error that only
shows in a small-scale head, fails.  `out` starts as NaN.

Bound of families 1-5:  err_kernel <= K * max(err_fp32, 2^-24) per (image, head), K = twice the largest ratio measured on the
MI355X over every family, T and C of this file (profiles/attention_precision.txt has the table):

    kernel                    largest measured ratio                                              K
    attention_kernel          7.65 (family 1, a = 16, T = 64, C = 64; typical 1.0 .. 2.5)         K_EXACT = 15.3
    attention_f16x2_kernel    4.92 (family 1, a = 16, T = 512, C = 64; typical 0.6 .. 3)          K_SPLIT = 9.84
    dmd_attention_bwd         14.98 (family 2, T = 256, dq, y from the forward; family 1: <= 9.1)  K_BWD = 30
                              (against float32 CPU autograd, no floor)

The ratio is one of two maxima over a head, so it scatters: attention_kernel's 7.65 is a head whose float32 CPU error happened to
be 8.6e-8 while the kernel's was 6.6e-7, at scores of +-700 where either evaluation is off by 2^-24 |s| in the exponent of a
near-tie; the largest error of any head in that case is 1.65e-5 for the kernel and of the same size for float32.  The two kernels
sit at the same distance from float64 at every T they share.  dmd_attention_bwd's 12 .. 15 are family 2's dq only (1.6e-4 of
max |dq| against float32 autograd's 1.1e-5): the kernel takes D = dy . y from the forward's y but recomputes the weights from
scores of +-204, which carry their own 1e-5 rounding, so sum_j dS_ij is not zero to rounding and is multiplied by the keys' common
component 24 U; with y from the float64 truth it is 8 .. 9.5: the forward's own error in y adds about a third.

TWO FINDINGS of these tests, both fixed in attention_f16x2_kernel (figures of the kernel before the fix):
  * test_operands_up_to_the_end_of_fp16[*-kv]: ratio 838 / 1019 / 523 / 696 at T = 256 / 512 / 768 / 1280 on the MI355X, 1340 /
    1005 on the interpreter (errors of 3.6e-4 .. 6.9e-4 of max|v| where float32 has 5e-7).  Scores of N(0, 4^2) with k at 1e4 ..
    65504 need q ~ 2e-4, and q' = q log2(e) / sqrt(8) ~ 1e-4 lies below 2^-3, where the split's absolute floor of 2^-25 per
    operand holds: the score was off by 2^-25 sum_i |k_i| ~ 2e-3.  The kernel now rebalances q' against its copy of the keys by
    a power of two when every q' of a workgroup is below 2^-3 (factor 1, and every bit as before, otherwise).
  * test_non_finite_operands_behave_as_in_float32[*-k]: a +-Inf in k made EVERY output of its (image, head) NaN (k_h = +-Inf,
    k_l = NaN, and both the q_l k_h slot and the unused slot group's k_h * 0 are NaN), while float32 keeps the rows finite whose
    score against that key is -Inf (1008 .. 5352 outputs differed per case).  An infinite key is now held as h = 0, l = +-Inf.

What the interpreter cannot reproduce: expf / exp2f are the host libm's, and the order of the sums inside an MFMA is its own; the
fp16 conversions (round to nearest even, overflow to infinity, subnormals kept) are the host compiler's IEEE ones, which is what
the device does too, so no assertion here had to be kept off the interpreter arm."""
import math
from types import SimpleNamespace

import pytest
import torch

from tests import abi
from tests import attention_cases as A
from tests.attention_cases import (BWD_CASES, K_BWD, K_EXACT, K_SPLIT, Ref, bwd_case, check_confined, family_floor, family_mixed_workgroups,
                                   family_moving_max, family_offset, family_onehot_uniform, family_range, family_scale, k_of, kernel_of,
                                   plant, sites, third_errors)

EXACT_T = (64, 192, 320)         # attention_kernel: one full tile of 64 .. 256 keys, a partial tile, a full + a partial tile
SPLIT_T = (256, 512, 768, 1280)  # attention_f16x2_kernel: 1, 2, 3 and 5 key tiles (both parities of the double buffer)


# ---- the two arms: tests/abi.py's runners with this file's shapes ------------------------------------------------------------------
def _arm(run, shapes, bwd_c):
    """`attention` is dmd_attention (exact=True: attention_kernel through dmd_attention_valid) on (N, T, 3C), `attention_bwd`
    dmd_attention_bwd, as tensors"""
    return SimpleNamespace(name=run.name, shapes=shapes, bwd_c=bwd_c,
                           attention=lambda qkv, c, exact=False: torch.from_numpy(abi.attention_default(run, qkv, c, exact)),
                           attention_bwd=lambda qkv, y, dy, c: torch.from_numpy(abi.attention_bwd(run, qkv, y, dy, c)))


SIMT = _arm(abi.Simt, ((2, 16),), 16)  # shapes: (N, C)
GPU = _arm(abi.Gpu, ((3, 8), (3, 24), (3, 64)), 24)  # one head, three heads, eight heads


def runners_by(ts, *more):
    """(run, t, *extra) cases: the interpreter arm gets T <= 512 only, the device arm every T"""
    return abi.arms_by_token_count(SIMT, GPU, ts, *more)


def check_bound(family, run, ref, got, exact=False, what=""):
    """print the figures of the worst (image, head), then assert the bound on every (image, head)"""
    n, t, _ = ref.qkv.shape
    A.check_bound(f"ATTPREC {run.name} family={family}{what} T={t} N={n} C={ref.c} {kernel_of(t, exact)}", ref, got, k_of(t, exact))


# ---- families 1-5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,t,a", runners_by(EXACT_T + SPLIT_T, 1.5, 4.0, 8.0, 16.0))
def test_score_magnitude(run, t, a):
    """Family 1; at the two-pass kernel's T the exact-fp32 kernel (dmd_attention_valid over the whole grid) is measured on the same
    inputs and held to its own bound, and the two kernels agree to within the sum of their bounds."""
    for n, c in run.shapes:
        ref = family_scale(n, c, t, a)
        got = run.attention(ref.qkv, c)
        check_bound(1, run, ref, got, what=f" a={a}")
        if t % 256 == 0:
            exact = run.attention(ref.qkv, c, exact=True)
            check_bound(1, run, ref, exact, exact=True, what=f" a={a}")
            both = ref.per_element(ref.limit(K_SPLIT) + ref.limit(K_EXACT))
            assert bool(((got.double() - exact.double()).abs() <= both).all()), "the two kernels disagree by more than their bounds"


@pytest.mark.parametrize("run,t", runners_by(EXACT_T + SPLIT_T))
def test_common_offset(run, t):
    """Family 2: the subtraction of the row maximum (negm in pass 2, m_run in the online kernel) under scores of +-204 +- O(5)"""
    for n, c in run.shapes:
        ref = family_offset(n, c, t)
        check_bound(2, run, ref, run.attention(ref.qkv, c))
        if t % 256 == 0:
            check_bound(2, run, ref, run.attention(ref.qkv, c, exact=True), exact=True)


@pytest.mark.parametrize("run,t", runners_by(EXACT_T + SPLIT_T))
def test_maximum_moving_with_the_key_index(run, t):
    """Family 3: the row maximum rises at every 16-key block and 256-key tile for half of the rows (alpha rescale of the online
    kernel; pass 1's running maximum across tiles), falls for the other half; winners exactly at keys 0, 255, 256, T - 1"""
    for n, c in run.shapes:
        ref = family_moving_max(n, c, t)
        check_bound(3, run, ref, run.attention(ref.qkv, c))
        if t % 256 == 0:
            check_bound(3, run, ref, run.attention(ref.qkv, c, exact=True), exact=True)


@pytest.mark.parametrize("run,t", runners_by(EXACT_T + SPLIT_T))
def test_onehot_and_uniform_rows(run, t):
    """Family 4: a one-hot row returns its key's v row, a q = 0 row the mean of V, side by side in every 16-query group"""
    for n, c in run.shapes:
        ref = family_onehot_uniform(n, c, t)
        got = run.attention(ref.qkv, c)
        check_bound(4, run, ref, got)
        v = ref.qkv[..., 2 * c:].double()
        lim = ref.per_element(ref.limit(k_of(t)))
        assert bool(((got[:, ref.hot].double() - v[:, ref.tgt]).abs() <= lim[:, ref.hot]).all()), "a one-hot row is not its key's v"
        mean = v.mean(dim=1, keepdim=True)
        assert bool(((got[:, ref.hot + 1].double() - mean).abs() <= lim[:, ref.hot + 1]).all()), "a q = 0 row is not the mean of V"


@pytest.mark.parametrize("run,t,which", runners_by(EXACT_T + SPLIT_T, "v", "kv"))
def test_operands_up_to_the_end_of_fp16(run, t, which):
    """Family 5: finite and within the bound with v ("v") and with k and v ("kv") reaching +-65504"""
    for n, c in run.shapes:
        ref = family_range(n, c, t, which)
        check_bound(5, run, ref, run.attention(ref.qkv, c), what=f" {which}")


@pytest.mark.parametrize("run,t", runners_by((512, 1280)))
def test_rebalanced_and_plain_workgroups_over_the_same_keys(run, t):
    """Family 5b: the power-of-two rebalancing of q' against the keys is each workgroup's own"""
    for n, c in run.shapes:
        ref = family_mixed_workgroups(n, c, t)
        check_bound("5b", run, ref, run.attention(ref.qkv, c))



@pytest.mark.parametrize("run,t", runners_by(EXACT_T + SPLIT_T))
def test_a_finite_value_beyond_fp16_is_loud_and_confined(run, t):
    """Family 6a: 1.0e5 in one v, one k and one q element of three different (image, head) pairs.  Nothing is clamped: every
    output of those heads (for q: of that query row) is non-finite or within the bound of the float64 truth, never finite and
    wrong, and everything else is bitwise unchanged.  (q * log2(e) / sqrt(8) = 5.1e4 is still an fp16 number: the two-pass kernel
    has to get that row right.)"""
    for n, c in run.shapes:
        where = sites(n, c, t)
        qkv = family_scale(n, c, t, 1.5).qkv
        for operand, site in where.items():
            qkv = plant(qkv, c, site, operand, 1.0e5)
        ref = Ref(qkv, c)
        got = run.attention(qkv, c)
        touched = check_confined(run, t, n, c, got, where)
        lim = ref.per_element(ref.limit(k_of(t)))
        err = (got.double() - ref.truth).abs()
        wrong = torch.isfinite(got) & ~(err <= lim)
        print(f"ATTPREC {run.name} family=6a T={t} N={n} C={c} {kernel_of(t)}: {int((~torch.isfinite(got)).sum())} non-finite of "
              f"{int(touched.sum())} touched outputs, largest finite err / bound {float((err / lim)[torch.isfinite(got)].max()):.2f}")
        assert not bool(wrong.any()), f"{int(wrong.sum())} outputs are finite and wrong"
        assert bool(torch.isfinite(got[~touched]).all())


@pytest.mark.parametrize("run,t,operand", runners_by(EXACT_T + SPLIT_T, "q", "k", "v"))
def test_non_finite_operands_behave_as_in_float32(run, t, operand):
    """Family 6b: NaN, +Inf, -Inf in one element of q, k or v: the output is finite exactly where the float32 CPU evaluation is
    finite, the finite part is within the bound, and everything outside the planted head / row / dim is bitwise unchanged."""
    failures = []
    for n, c in run.shapes:
        site = sites(n, c, t)[operand]
        for value in (math.nan, math.inf, -math.inf):
            ref = Ref(plant(family_scale(n, c, t, 1.5).qkv, c, site, operand, value), c)
            got = run.attention(ref.qkv, c)
            check_confined(run, t, n, c, got, {operand: site})
            fin, fin32 = torch.isfinite(got), torch.isfinite(ref.y32)
            both = fin & fin32 & torch.isfinite(ref.truth)
            err = torch.where(both, (got.double() - ref.truth).abs(), torch.zeros_like(ref.truth))
            over = err > ref.per_element(ref.limit(k_of(t)))
            print(f"ATTPREC {run.name} family=6b {operand}={value} T={t} N={n} C={c} {kernel_of(t)}: finite {int(fin.sum())} "
                  f"(float32: {int(fin32.sum())}), {int((fin != fin32).sum())} differ, {int(over.sum())} finite outputs over the bound")
            if bool((fin != fin32).any()):
                failures.append(f"C={c} {operand}={value}: {int((fin & ~fin32).sum())} finite where float32 is not, "
                                f"{int((~fin & fin32).sum())} non-finite where float32 is finite")
            if bool(over.any()):
                failures.append(f"C={c} {operand}={value}: {int(over.sum())} finite outputs over the bound")
    assert not failures, failures


# ---- family 7: the absolute floor --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,t", runners_by(EXACT_T + SPLIT_T))
def test_absolute_floor(run, t):
    """Family 7: v * 1e-7.  The two-pass kernel's fp16 pieces stop at 2^-25: the output is a convex combination of operands each off
    by at most that, plus the fp32 rounding: |got - truth| <= 2^-24 + 1e-5 |truth|; the same tensor times 2^23 is within the
    ordinary bound again.  attention_kernel holds the ordinary bound without pre-scaling."""
    for n, c in run.shapes:
        ref = family_floor(n, c, t, 1.0)
        got = run.attention(ref.qkv, c)
        if t % 256:
            check_bound(7, run, ref, got, what=" v*1e-7")
            continue
        err = (got.double() - ref.truth).abs()
        print(f"ATTPREC {run.name} family=7 v*1e-7 T={t} N={n} C={c} {kernel_of(t)}: largest |got - truth| {float(err.max()):.3e} "
              f"= {float(err.max()) * 2.0 ** 25:.2f} x 2^-25 (max |truth| {float(ref.truth.abs().max()):.3e})")
        assert bool(torch.isfinite(got).all())
        assert bool((err <= 2.0 ** -24 + 1.0e-5 * ref.truth.abs()).all()), float(err.max())
        up = family_floor(n, c, t, 2.0 ** 23)
        check_bound(7, run, up, run.attention(up.qkv, c), what=" v*1e-7*2^23")



@pytest.mark.parametrize("y_from", ["forward", "truth"])
@pytest.mark.parametrize("run,t,family,a", runners_by((64, 256, 1024), *BWD_CASES))
def test_backward_on_the_forward_it_gets(run, t, family, a, y_from):
    """dmd_attention_bwd over the full grid with y = dmd_attention's output (the split-fp16 kernel for T >= 256: what the training
    step feeds it) and with y = float32(float64 truth), against float64 autograd, per (image, head) and per third of dqkv:
    within K_BWD x the error of float32 CPU autograd, and within test_attention_bwd_valid.py's 2e-5 at a = 1.5."""
    n, c = 2, run.bwd_c
    ref, b = bwd_case(n, c, t, family, a)
    y = run.attention(ref.qkv, c) if y_from == "forward" else b.y64.float()
    got = run.attention_bwd(ref.qkv, y, b.dy, c)
    assert bool(torch.isfinite(got).all())
    e, e32 = third_errors(got, b.want, c), third_errors(b.g32, b.want, c)
    ratio = e / e32
    print(f"ATTPREC {run.name} bwd family={family} a={a} T={t} N={n} C={c} y={y_from}: err dq|dk|dv "
          f"{[f'{float(x):.2e}' for x in e.amax(dim=(0, 2))]} float32 autograd {[f'{float(x):.2e}' for x in e32.amax(dim=(0, 2))]} "
          f"ratio {float(ratio.max()):.2f}")
    assert float(ratio.max()) <= K_BWD, ratio
    if family == 1 and a == 1.5:
        assert float(e.max()) <= 2e-5, float(e.max())

