"""Shared by the attention test modules (tests/test_attention_*.py): the float64 / float32 torch-CPU restatement of
softmax(q k^T / sqrt(8)) v per head, the metric per (image, head), the input families, the bounds' constants, the valid-extent
inputs of the backward kernels and the training-step helpers of the routing tests.  Nothing here loads a library: a kernel is
reached through the `attention` callable of the arm a test hands in (tests/abi.py has the launchers).

Every (image, head) has its own V scale (0.03 .. 30, shuffled), so a result in the wrong head or image, or an error that only
shows in a small-scale head, fails.  tests/test_attention_precision.py's docstring has the bounds and how they were measured.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

K_EXACT = 15.3  # 2 x 7.65
K_SPLIT = 9.84  # 2 x 4.92
K_BWD = 30.0    # 2 x 14.98
FLOOR = 2.0 ** -24

U = torch.tensor([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype=torch.float64) / math.sqrt(8.0)  # the fixed direction


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


def ratios(ref, got):
    """(error, error / max(err_fp32, 2^-24)) per (image, head)"""
    e = head_errors(got, ref.truth, ref.vmax, ref.c)
    return e, e / torch.maximum(ref.e32, torch.full_like(ref.e32, FLOOR))


def check_bound(head, ref, got, k):
    """print `head` and the figures of the worst (image, head), then assert the bound err <= k max(err_fp32, 2^-24) on every
    (image, head); returns (error per (image, head), largest ratio)"""
    e, ratio = ratios(ref, got)
    i = int(ratio.argmax())
    print(f"{head}: err {float(e.flatten()[i]):.3e} fp32 {float(ref.e32.flatten()[i]):.3e} ratio {float(ratio.max()):.2f} "
          f"(largest err {float(e.max()):.3e})")
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert float(ratio.max()) <= k, (float(ratio.max()), ratio)
    return e, float(ratio.max())


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


@functools.lru_cache(maxsize=None)
def family_mixed_workgroups(n, c, t):
    """5b: k ~ N(0, 100^2); queries 0 .. 255 ~ N(0, 0.04^2), a workgroup that the two-pass kernel rebalances (every q' < 2^-3, scores
    N(0, 4^2)), the other queries ~ N(0, 1^2), workgroups that it does not (scores N(0, 100^2)), over the same keys"""
    g = torch.Generator().manual_seed(5500 + t + c)
    nh = c // 8
    q = randn(g, n, nh, t, 8)
    q[:, :, :256] *= 0.04
    return Ref(assemble(q, randn(g, n, nh, t, 8) * 100.0, randn(g, n, nh, t, 8) * v_scales(n, nh, g)), c)


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


# ---- backward ------------------------------------------------------------------------------------------------------------------------
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


# ---- valid extents of the backward kernels ------------------------------------------------------------------------------------------
EXTENT_CASES = [(16, 16, 9, 9), (16, 16, 9, 10), (32, 32, 18, 20), (64, 64, 36, 36)]  # (H, W, valid_h, valid_w)
EXTENT_C, EXTENT_N = 64, 2


def extent_inputs(h, w, vh, vw, seed, N=EXTENT_N, C=EXTENT_C):
    """qkv / y / dy (N, H, W, .) float32 with garbage margins, and the float64 reference dqkv of the valid tokens"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(N, h, w, 3 * C, generator=g, dtype=torch.float64) * 1.5
    dy = torch.randn(N, h, w, C, generator=g, dtype=torch.float64)
    q32 = qkv.float()
    crop = q32[:, :vh, :vw].reshape(N, vh * vw, 3 * C).double().requires_grad_(True)
    heads = lambda t: t.reshape(N, vh * vw, C // 8, 8).transpose(1, 2)
    q, k, v = (heads(crop[..., i * C:(i + 1) * C]) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / np.sqrt(8.0), dim=-1)
    y64 = (p @ v).transpose(1, 2).reshape(N, vh, vw, C)
    dy32 = dy.float()
    y64.backward(dy32[:, :vh, :vw].double())
    want = crop.grad.reshape(N, vh, vw, 3 * C)
    y = torch.empty(N, h, w, C)
    y[:, :vh, :vw] = y64.detach().float()
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[:vh, :vw] = True
    garbage = lambda t: t.masked_fill(~inside[None, :, :, None], float("nan")).masked_fill(
        (~inside[None, :, :, None]) & (torch.arange(t.shape[-1]) % 2 == 0), 3e38)
    return garbage(q32), garbage(y), garbage(dy32), want, inside


def check_extent_grad(dqkv, want, inside, vh, vw):
    """dqkv within 2e-5 of max |want| on the valid tokens, +0 outside them"""
    got = dqkv[:, :vh, :vw].double()
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 2e-5, err
    out = dqkv[:, ~inside]
    assert bool((out == 0).all()) and not bool(torch.signbit(out).any()), "dqkv outside the valid extent is not zero"


# ---- routing and the training step -------------------------------------------------------------------------------------------------
class LaunchCounter:
    """stands in for native.PROFILER: counts launches per key (no timing)"""

    def __init__(self):
        self.n = {}
        self._pending = None

    def annotate(self, key, flops, nbytes):
        self._pending = key

    def call(self, name, fn, args):
        key, self._pending = self._pending or name, None
        self.n[key] = self.n.get(key, 0) + 1
        return fn(*args)


FORWARD_KEYS = ("attention_kernel", "attention_f16x2_kernel", "attention_f32_tiled_kernel", "dmd_attention", "dmd_attention_valid",
                "dmd_attention_f32")


def two_level_denoiser():
    """the two-level 16 x 16 network of tests/test_simt_host.py on the CPU (attention over 64 tokens at its 8x8 level) with one
    training batch and the inputs of one inference call: (den, batch, noisy, obs)"""
    import diamond_amd as D
    from diamond_amd.inner_model import InnerModelConfig
    from diamond_amd.testing import fill_module_, synthetic_actions, synthetic_frames
    from tests import wide_configs as W

    cfg = dict(W.DENOISER, depths=[1, 1], channels=[64, 96], attn_depths=[0, 1])
    den = D.Denoiser(D.DenoiserConfig(inner_model=InnerModelConfig(**cfg), sigma_data=0.5, sigma_offset_noise=0.3))
    fill_module_(den, W.WEIGHT_SEED)
    den.setup_training(D.SigmaDistributionConfig(**W.SIGMA_DIST))
    den.randn_fn = lambda shape: torch.randn(*shape)
    g = torch.Generator().manual_seed(31)
    frames, act = synthetic_frames(g, 1, 5, 3, 16, 16), synthetic_actions(g, 4, 1, 5)
    batch = SimpleNamespace(obs=frames, act=act, mask_padding=torch.ones(1, 5, dtype=torch.bool))
    return den, batch, torch.randn(1, 3, 16, 16, generator=g), frames[:, :4].reshape(1, 12, 16, 16)


def training_step(den, batch, seed=77):
    den.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    loss, _ = den(batch)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in den.named_parameters()}


def assert_training_parity(new, old):
    """every parameter gradient within 2e-5 of max |g| (README, "Parity")"""
    bad = {}
    for k, g in old.items():
        err = float((new[k].double() - g.double()).abs().max() / g.double().abs().max().clamp_min(1e-30))
        if not err <= 2e-5:
            bad[k] = err
    assert not bad, bad


def device_denoiser():
    """the default denoiser at 64x64 with attention at its 32x32 level: 1024 tokens, batch 2"""
    import diamond_amd as D
    from diamond_amd.testing import fill_module_
    from tests.conftest import WEIGHT_SEED

    agent = D.Agent(D.default_agent_config(denoiser_attn_depths=(0, 1, 0, 0)))
    fill_module_(agent, WEIGHT_SEED)
    den = agent.to("cuda").eval().denoiser
    den.train()
    den.setup_training(D.SigmaDistributionConfig(loc=-0.4, scale=1.2, sigma_min=2e-3, sigma_max=20))
    return den


def device_batches(count):
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    g = torch.Generator().manual_seed(8)
    return [SimpleNamespace(obs=synthetic_frames(g, 2, 5, 3, 64, 64).cuda(), act=synthetic_actions(g, 4, 2, 5).cuda(),
                            mask_padding=torch.ones(2, 5, dtype=torch.bool).cuda()) for _ in range(count)]


def check_graphed_training_step_is_bitwise_the_eager_loop(monkeypatch):
    """the launches record into a hipGraph (no allocation, no synchronisation) and replay exactly the eager loop, in the manner of
    tests/test_offgrid_train.py"""
    from diamond_amd.train_graph import GraphedTrainStep

    monkeypatch.setenv("DIAMOND_ATTN_BWD_MIN_T", "1024")

    def setup():
        den = device_denoiser()
        table = {}

        def randn_fn(shape):  # device-resident noise, the same at every step for both runs
            if shape not in table:
                table[shape] = torch.randn(*shape, generator=torch.Generator().manual_seed(len(table) + 99)).cuda()
            return table[shape]

        den.randn_fn = randn_fn
        return den, torch.optim.AdamW(den.parameters(), lr=3e-4, capturable=True), device_batches(2)

    warm, steps = 2, 2
    den, opt, batches = setup()
    init = {k: v.detach().clone() for k, v in den.state_dict().items()}
    losses_e = []
    for i in range(warm + steps):
        loss, _ = den(batches[0] if i < warm else batches[i % 2])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(den.parameters(), 1.0)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if i >= warm:
            losses_e.append(loss.detach().clone())
    params_e = {k: v.detach().clone() for k, v in den.named_parameters()}

    den2, opt2, batches2 = setup()
    den2.load_state_dict(init)
    gstep = GraphedTrainStep(den2, opt2, 1.0, batches2[0], warmup_steps=warm)
    losses_g = [gstep(batches2[(warm + i) % 2])[0].clone() for i in range(steps)]
    torch.cuda.synchronize()
    assert len({float(x) for x in losses_g}) == steps, "the replayed step must see the new batch / the updated weights"
    assert all(torch.equal(a, b) for a, b in zip(losses_e, losses_g)), (losses_e, losses_g)
    assert max(float((p.detach() - params_e[k]).abs().max()) for k, p in den2.named_parameters()) == 0.0
    assert max(float((p.detach() - init[k]).abs().max()) for k, p in den2.named_parameters()) > 1e-4, "parameters did not train"
