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
import functools
import math

import numpy as np
import pytest
import torch

K_EXACT = 15.3  # 2 x 7.65
K_SPLIT = 9.84  # 2 x 4.92
K_BWD = 30.0    # 2 x 14.98
FLOOR = 2.0 ** -24

EXACT_T = (64, 192, 320)         # attention_kernel: one full tile of 64 .. 256 keys, a partial tile, a full + a partial tile
SPLIT_T = (256, 512, 768, 1280)  # attention_f16x2_kernel: 1, 2, 3 and 5 key tiles (both parities of the double buffer)
U = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype=torch.float64) / math.sqrt(8.0)  # the fixed direction


# ---- the two runners ---------------------------------------------------------------------------------------------------------------
class Simt:
    """the kernels' own source on the interpreter, arrays fenced"""
    name = "simt"
    shapes = ((2, 16),)  # (N, C)
    bwd_c = 16

    @staticmethod
    def attention(qkv, c, exact=False):
        from tests.simt import loader as S
        from tests.simt.fence import fenced as G

        n, t, _ = qkv.shape
        a, out = G(qkv.numpy()), G(np.full((n, t, c), np.nan, dtype=np.float32))
        if exact:
            S.check(S.lib().dmd_attention_valid(S.ptr(a), S.ptr(out), n, t // 16, 16, t // 16, 16, c, 8, None), "dmd_attention_valid")
        else:
            S.check(S.lib().dmd_attention(S.ptr(a), S.ptr(out), n, t, c, 8, None), "dmd_attention")
        return torch.from_numpy(np.array(out))

    @staticmethod
    def attention_bwd(qkv, y, dy, c):
        from tests.simt import loader as S
        from tests.simt.fence import fenced as G

        n, t, _ = qkv.shape
        L = S.lib()
        a = [G(x.numpy()) for x in (qkv, y, dy)]
        ws = G(np.full(L.dmd_attention_bwd_workspace_floats(n, t, c), np.nan, dtype=np.float32))
        dqkv = G(np.full((n, t, 3 * c), np.nan, dtype=np.float32))
        S.check(L.dmd_attention_bwd(*(S.ptr(x) for x in a), S.ptr(dqkv), S.ptr(ws), n, t, c, 8, None), "dmd_attention_bwd")
        return torch.from_numpy(np.array(dqkv))


class Gpu:
    name = "gpu"
    shapes = ((3, 8), (3, 24), (3, 64))  # one head, three heads, eight heads
    bwd_c = 24

    @staticmethod
    def attention(qkv, c, exact=False):
        from diamond_amd import native as nv

        n, t, _ = qkv.shape
        a, out = qkv.cuda().contiguous(), torch.full((n, t, c), float("nan"), device="cuda")
        if exact:
            nv.check(nv.lib().dmd_attention_valid(nv.fptr(a), nv.fptr(out), n, t // 16, 16, t // 16, 16, c, 8, nv.stream()),
                     "dmd_attention_valid")
        else:
            nv.check(nv.lib().dmd_attention(nv.fptr(a), nv.fptr(out), n, t, c, 8, nv.stream()), "dmd_attention")
        return out.cpu()

    @staticmethod
    def attention_bwd(qkv, y, dy, c):
        from diamond_amd import native as nv

        n, t, _ = qkv.shape
        a = [x.cuda().contiguous() for x in (qkv, y, dy)]
        ws = torch.full((int(nv.lib().dmd_attention_bwd_workspace_floats(n, t, c)),), float("nan"), device="cuda")
        dqkv = torch.full((n, t, 3 * c), float("nan"), device="cuda")
        nv.check(nv.lib().dmd_attention_bwd(*(nv.fptr(x) for x in a), nv.fptr(dqkv), nv.fptr(ws), n, t, c, 8, nv.stream()),
                 "dmd_attention_bwd")
        return dqkv.cpu()


def runners_by(ts, *more, simt_max_t=512):
    """(run, t, *extra) cases: the interpreter arm gets T <= 512 only, the device arm every T"""
    extras = [()] if not more else [e if isinstance(e, tuple) else (e,) for e in more]
    out = []
    for t in ts:
        for e in extras:
            tag = "-".join([str(t)] + [str(x) for x in e])
            if t <= simt_max_t:
                out.append(pytest.param(Simt, t, *e, id=f"simt-{tag}"))
            out.append(pytest.param(Gpu, t, *e, marks=pytest.mark.gpu, id=f"gpu-{tag}"))
    return out


# ---- reference and metric ----------------------------------------------------------------------------------------------------------
def heads(x, c):
    """(N, T, c) -> (N, c / 8, T, 8)"""
    n, t, _ = x.shape
    return x.reshape(n, t, c // 8, 8).transpose(1, 2)


def formula(qkv, c, dtype):
    """softmax(q k^T / sqrt(8)) v per head in `dtype` on the CPU, image by image"""
    outs = []
    for x in qkv:
        q, k, v = (heads(x[None, :, i * c:(i + 1) * c].to(dtype), c) for i in range(3))
        p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(8.0), dim=-1)
        outs.append((p @ v).transpose(1, 2).reshape(1, -1, c))
    return torch.cat(outs)


def assemble(q, k, v):
    """three (N, heads, T, 8) float64 tensors -> float32 qkv (N, T, 3C)"""
    n, nh, t, _ = q.shape
    return torch.cat([x.transpose(1, 2).reshape(n, t, nh * 8) for x in (q, k, v)], dim=-1).float().contiguous()


def v_scales(n, nh, g):
    """one V scale per (image, head): 0.03 .. 30, log-spaced, in no particular order"""
    m = n * nh
    f = 0.03 * 1000.0 ** (torch.arange(m, dtype=torch.float64) / max(m - 1, 1))
    return f[torch.randperm(m, generator=g)].reshape(n, nh, 1, 1)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def orth(x):
    """x without its component along U"""
    return x - (x @ U)[..., None] * U


def head_max(x, c):
    """(N, T, c) -> (N, heads): max |x| of every (image, head), non-finite entries left out"""
    return heads(torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)), c).amax(dim=(2, 3)).double()


def head_errors(y, truth, vmax, c):
    """max over queries and dims of |y - truth| / max|v| per (image, head); entries where either is non-finite are left out"""
    d = (y.double() - truth).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    return heads(d, c).amax(dim=(2, 3)) / vmax


class Ref:
    """inputs with their float64 truth and float32 stick (computed once per case, shared by the tests, never written to)"""

    def __init__(self, qkv, c):
        self.qkv, self.c = qkv, c
        self.truth = formula(qkv, c, torch.float64)
        self.y32 = formula(qkv, c, torch.float32)
        self.vmax = head_max(qkv[..., 2 * c:], c)
        self.e32 = head_errors(self.y32, self.truth, self.vmax, c)

    def limit(self, k):
        """the bound as an absolute error per (image, head)"""
        return k * torch.maximum(self.e32, torch.full_like(self.e32, FLOOR)) * self.vmax

    def per_element(self, lim):
        """(N, heads) -> (N, T, C)"""
        return lim.repeat_interleave(8, dim=1)[:, None, :].expand_as(self.truth)


def kernel_of(t, exact=False):
    return "attention_kernel" if exact or t % 256 else "attention_f16x2_kernel"


def k_of(t, exact=False):
    return K_EXACT if exact or t % 256 else K_SPLIT


def check_bound(family, run, ref, got, exact=False, what=""):
    """print the figures of the worst (image, head), then assert the bound on every (image, head)"""
    n, t, _ = ref.qkv.shape
    e = head_errors(got, ref.truth, ref.vmax, ref.c)
    ratio = e / torch.maximum(ref.e32, torch.full_like(ref.e32, FLOOR))
    i = int(ratio.argmax())
    print(f"ATTPREC {run.name} family={family}{what} T={t} N={n} C={ref.c} {kernel_of(t, exact)}: err {float(e.flatten()[i]):.3e} "
          f"fp32 {float(ref.e32.flatten()[i]):.3e} ratio {float(ratio.max()):.2f} (largest err {float(e.max()):.3e})")
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert float(ratio.max()) <= k_of(t, exact), (float(ratio.max()), ratio)
    return e


# ---- input families ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_scale(n, c, t, a):
    """1: q, k ~ a N(0, 1), v at its per-head scale"""
    g = torch.Generator().manual_seed(1000 + t + c)
    nh = c // 8
    return Ref(assemble(randn(g, n, nh, t, 8) * a, randn(g, n, nh, t, 8) * a, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)


@functools.lru_cache(maxsize=None)
def family_offset(n, c, t):
    """2: every key carries 24 U, every query +-24 U (alternating): each row's scores share the offset +-24 * 24 / sqrt(8) = +-204,
    the parts orthogonal to U give differences of O(5)"""
    g = torch.Generator().manual_seed(2000 + t + c)
    nh = c // 8
    sign = torch.where(torch.arange(t) % 2 == 0, 1.0, -1.0).double()[:, None]
    q = orth(randn(g, n, nh, t, 8) * 1.5) + 24.0 * sign * U
    k = orth(randn(g, n, nh, t, 8) * 1.5) + 24.0 * U
    return Ref(assemble(q, k, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)


def winner_targets(t):
    return sorted({0, 255, 256, t - 1} & set(range(t)))


@functools.lru_cache(maxsize=None)
def family_moving_max(n, c, t):
    """3: key j carries 0.177 j U, queries +-4 U (alternating): the scores of a row rise (fall) by 0.25 per key = 4 per 16-key
    block = 64 per tile under noise of sigma 0.5, so the running maximum changes at every block and tile for half of the rows and
    never after the first key for the others.  Rows 2.. and T - 14.. instead point at one key each: 0, 255, 256, T - 1."""
    g = torch.Generator().manual_seed(3000 + t + c)
    nh = c // 8
    w = torch.linalg.qr(torch.cat([U[:, None], randn(g, 8, 7)], dim=1))[0][:, 1:]  # orthonormal, orthogonal to U
    sign = torch.where(torch.arange(t) % 2 == 0, 1.0, -1.0).double()[:, None]
    ramp = 0.25 * math.sqrt(8.0) / 4.0 * torch.arange(t, dtype=torch.float64)[:, None] * U
    q = orth(randn(g, n, nh, t, 8) * 0.7) + 4.0 * sign * U
    k = orth(randn(g, n, nh, t, 8) * 0.7) + ramp
    rows = {}
    for m, j in enumerate(winner_targets(t)):
        k[:, :, j] = 4.0 * w[:, m] + ramp[j]
        for i in (2 + m, t - 14 + m):
            q[:, :, i] = 6.0 * w[:, m]
            rows[i] = j
    ref = Ref(assemble(q, k, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)
    q32, k32 = (heads(ref.qkv[..., i * c:(i + 1) * c].double(), c) for i in range(2))
    for i, j in rows.items():  # the inputs do what the docstring says
        assert bool(((q32[:, :, i:i + 1] @ k32.transpose(-1, -2)).argmax(dim=-1) == j).all()), (i, j)
    return ref


@functools.lru_cache(maxsize=None)
def family_onehot_uniform(n, c, t):
    """4: keys of norm 4.  Rows i % 4 == 0: q = lambda k_j with lambda such that key j leads by 63 in the exponent (one-hot);
    rows i % 4 == 1: q = 0 (uniform weights); the others N(0, 1.5^2).  Every 16-query group has four of each."""
    g = torch.Generator().manual_seed(4000 + t + c)
    nh = c // 8
    k = randn(g, n, nh, t, 8)
    k = 4.0 * k / k.norm(dim=-1, keepdim=True)
    q = randn(g, n, nh, t, 8) * 1.5
    hot = torch.arange(0, t, 4)
    special = winner_targets(t)
    tgt = torch.tensor([special[r] if r < len(special) else (37 * r + 11) % t for r in range(len(hot))])
    dots = k[:, :, tgt] @ k.transpose(-1, -2)
    dots[:, :, torch.arange(len(hot)), tgt] = -math.inf
    lam = 63.0 * math.sqrt(8.0) / (16.0 - dots.amax(dim=-1))
    q[:, :, hot] = lam[..., None] * k[:, :, tgt]
    q[:, :, hot + 1] = 0.0
    ref = Ref(assemble(q, k, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)
    q32, k32 = (heads(ref.qkv[..., i * c:(i + 1) * c].double(), c) for i in range(2))
    s = q32[:, :, hot] @ k32.transpose(-1, -2) / math.sqrt(8.0)
    lead = s[:, :, torch.arange(len(hot)), tgt].clone()
    s[:, :, torch.arange(len(hot)), tgt] = -math.inf
    assert float((lead - s.amax(dim=-1)).min()) >= 60.0
    ref.hot, ref.tgt = hot, tgt
    return ref


@functools.lru_cache(maxsize=None)
def family_range(n, c, t, which):
    """5: v elements ("v"), and k elements too ("kv"), up to +-65504, the end of fp16: v ~ N(0, s^2) clamped with s = 20 .. 2e4 per
    (image, head) and +-65504 planted; k ~ N(0, 2e4^2) clamped with +-65504 planted and q ~ N(0, 2e-4^2), so that the scores stay
    N(0, 4^2)"""
    g = torch.Generator().manual_seed(5000 + t + c)
    nh = c // 8
    big = 65504.0

    def reach(x):
        x = x.clamp(-big, big)
        pos = torch.randint(0, t, (8,), generator=g)
        for e, p in enumerate(pos.tolist()):
            x[:, :, p, e] = big if e % 2 else -big
        x[:, :, 0, 0], x[:, :, t - 1, 7] = big, -big
        return x

    v = reach(randn(g, n, nh, t, 8) * v_scales(n, nh, g) * (2.0e4 / 30.0))
    if which == "kv":
        q, k = randn(g, n, nh, t, 8) * 2.0e-4, reach(randn(g, n, nh, t, 8) * 2.0e4)
    else:
        q, k = randn(g, n, nh, t, 8) * 1.5, randn(g, n, nh, t, 8) * 1.5
    return Ref(assemble(q, k, v), c)


@functools.lru_cache(maxsize=None)
def family_floor(n, c, t, prescale):
    """7: family 1 at a = 1.5 with v scaled by 1e-7 (3e-9 .. 3e-6 per (image, head)), optionally times 2^23 (exact)"""
    base = family_scale(n, c, t, 1.5).qkv.clone()
    base[..., 2 * c:] *= 1.0e-7
    base[..., 2 * c:] *= prescale
    return Ref(base, c)


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


@functools.lru_cache(maxsize=None)
def family_mixed_workgroups(n, c, t):
    """5b: k ~ N(0, 100^2); queries 0 .. 255 ~ N(0, 0.04^2), a workgroup that the two-pass kernel rebalances (every q' < 2^-3, scores
    N(0, 4^2)), the other queries ~ N(0, 1^2), workgroups that it does not (scores N(0, 100^2)), over the same keys"""
    g = torch.Generator().manual_seed(5500 + t + c)
    nh = c // 8
    q = randn(g, n, nh, t, 8)
    q[:, :, :256] *= 0.04
    return Ref(assemble(q, randn(g, n, nh, t, 8) * 100.0, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)


@pytest.mark.parametrize("run,t", runners_by((512, 1280)))
def test_rebalanced_and_plain_workgroups_over_the_same_keys(run, t):
    """Family 5b: the power-of-two rebalancing of q' against the keys is each workgroup's own"""
    for n, c in run.shapes:
        ref = family_mixed_workgroups(n, c, t)
        check_bound("5b", run, ref, run.attention(ref.qkv, c))


# ---- family 6: beyond the range, non-finite ----------------------------------------------------------------------------------------
_BASE_OUT = {}


def base_output(run, n, c, t):
    key = (run.name, n, c, t)
    if key not in _BASE_OUT:
        _BASE_OUT[key] = run.attention(family_scale(n, c, t, 1.5).qkv, c)
    return _BASE_OUT[key]


def sites(n, c, t):
    """operand -> (image, head, token, dim): three different (image, head) pairs"""
    pairs = [(i, h) for i in range(n) for h in range(c // 8)]
    pick = (pairs[0], pairs[len(pairs) // 2], pairs[-1])
    return {"v": pick[0] + (t // 3, 5), "k": pick[1] + (t - 2, 2), "q": pick[2] + (17, 6)}


def plant(qkv, c, site, operand, value):
    i, h, tok, d = site
    qkv = qkv.clone()
    qkv[i, tok, "qkv".index(operand) * c + 8 * h + d] = value
    return qkv


def head_slice(x, i, h):
    return x[i, :, 8 * h:8 * h + 8]


def check_confined(run, t, n, c, got, planted):
    """everything outside the planted (image, head) pairs -- and, for q, outside the planted query row; for v, outside the planted
    dim -- is bitwise what the run without the planted values gave"""
    base = base_output(run, n, c, t)
    touched = torch.zeros(n, t, c, dtype=torch.bool)
    for operand, (i, h, tok, d) in planted.items():
        if operand == "q":
            touched[i, tok, 8 * h:8 * h + 8] = True
        elif operand == "v":
            touched[i, :, 8 * h + d] = True
        else:
            touched[i, :, 8 * h:8 * h + 8] = True
    same = (got == base) | touched
    assert bool(same.all()), f"{int((~same).sum())} outputs outside the planted heads / rows changed"
    return touched


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


# ---- backward on the forward it actually gets ----------------------------------------------------------------------------------------
class BwdRef:
    """dy, the float64 autograd truth of dqkv and y, and float32 CPU autograd's dqkv"""

    def __init__(self, qkv, c, seed):
        n, t, _ = qkv.shape
        self.dy = torch.randn(n, t, c, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()
        self.want, self.y64 = self.autograd(qkv, c, torch.float64)
        self.g32 = self.autograd(qkv, c, torch.float32)[0]

    def autograd(self, qkv, c, dtype):
        x = qkv.clone().to(dtype).requires_grad_(True)
        y = formula(x, c, dtype)
        y.backward(self.dy.to(dtype))
        return x.grad, y.detach()


def third_errors(g, want, c):
    """(N, T, 3C) -> (N, 3, heads): max |g - want| / max |want| per (image, head) and per third dq | dk | dv"""
    n, t, _ = want.shape
    r = lambda x: x.reshape(n, t, 3, c // 8, 8).abs().amax(dim=(1, 4))
    return r(g.double() - want.double()) / r(want.double())


@functools.lru_cache(maxsize=None)
def bwd_case(n, c, t, family, a):
    ref = family_scale(n, c, t, a) if family == 1 else family_offset(n, c, t)
    return ref, BwdRef(ref.qkv, c, seed=t + int(10 * a))


BWD_CASES = [(1, 1.5), (1, 4.0), (1, 8.0), (2, 0.0)]


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
