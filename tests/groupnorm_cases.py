"""Shared by the two runners of tests/test_groupnorm_precision.py: the input families of the GroupNorm sites, applied per (image,
group), and float64 / float32 torch-CPU RESTATEMENTS of what each site computes, written from include/diamond_hip.h and
models/blocks.py:

    GroupNorm(G = max(1, C / 32) groups of C / G channels, eps 1e-5, statistics of the valid extent) * (1 +) mul + add [, SiLU]

Truth is the restatement in float64 over the float32 inputs; the measuring stick is the same code in float32 (F.group_norm, F.silu,
F.conv2d, autograd).  Nothing here knows a kernel.

An ARM is one launch of three images.  The three images belong to different families, one of them benign (N(0.3, 1.5^2), what
every other test of these kernels draws), and the groups of one image carry different parameters of their family: a value taken
from the wrong image or group is a wrong value.  Where an image has a single group (C = 32, 48) `shift` selects which of the
image's group parameters it gets; the tests run both.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
OTHER_EPS = (0.0, 1e-6, 1e-4)  # the truth must tell these from EPS on every arm with sigma <= 1e-2

BENIGN = ("benign",)


def _img(family: int, groups: Sequence[tuple], film: str = "plain") -> dict:
    return dict(family=family, groups=list(groups), film=film)


# family 0: benign; 1: small spread; 2: constant groups; 3: offset mean = r sigma; 4: one outlier; 5: channel scales inside a
# group; 6: FiLM edges; 7: non-finite
ARMS: Dict[str, List[dict]] = {
    "small-const": [_img(1, [("small", 1e-2), ("small", 1e-3)]), _img(2, [("const", 0.7), ("const", -3.25)]), _img(0, [BENIGN])],
    "small-offset": [_img(0, [BENIGN]), _img(1, [("small", 3.16e-3), ("small", 1e-1)]), _img(3, [("offset", 10.0, 1.0), ("offset", 30.0, 1.0)])],
    "offset-small": [_img(3, [("offset", 30.0, 0.01), ("offset", 10.0, 0.01)]), _img(0, [BENIGN]), _img(1, [("small", 1e-4), ("small", 1e-2)])],
    "zero-outlier": [_img(2, [("const", 0.0)]), _img(4, [("outlier", 1e4), ("outlier", -1e4)]), _img(0, [BENIGN])],
    "scales-film": [_img(5, [("chanscale", 1e-3, 1e3), ("chanscale", 1e3, 1e-3)]), _img(0, [BENIGN]), _img(6, [BENIGN], film="edges")],
    "nan": [_img(0, [BENIGN]), _img(7, [("nan",), BENIGN]), _img(2, [("const", 0.0), ("const", 0.7)])],
}
FAMILY_OF = {arm: tuple(im["family"] for im in imgs) for arm, imgs in ARMS.items()}


def tt(a: np.ndarray, dtype) -> torch.Tensor:
    """a copy of a (possibly read-only) array as a tensor of `dtype`"""
    return torch.tensor(np.asarray(a)).to(dtype)


def groups_of(c: int) -> int:
    return max(1, c // 32)


def group_spec(arm: str, image: int, group: int, shift: int = 0) -> tuple:
    specs = ARMS[arm][image]["groups"]
    return specs[(group + shift) % len(specs)]


def sees_eps(arm: str, c: int, shift: int = 0) -> List[Tuple[int, int]]:
    """the (image, group) pairs of the arm with sigma <= 1e-2: where eps = 1e-5 must be told from 0, 1e-6 and 1e-4"""
    out = []
    for i in range(len(ARMS[arm])):
        for j in range(groups_of(c)):
            s = group_spec(arm, i, j, shift)
            if (s[0] == "small" and s[1] <= 1e-2) or (s[0] == "offset" and s[2] <= 1e-2):
                out.append((i, j))
    return out


def _fill(spec: tuple, rng: np.random.Generator, pix: int, gs: int) -> np.ndarray:
    """(pix, gs) float64 values of one (image, group)"""
    z = rng.standard_normal((pix, gs))
    kind = spec[0]
    if kind == "benign":
        return 0.3 + 1.5 * z
    if kind == "small":
        return spec[1] * (z - z.mean())  # mean 0
    if kind == "const":
        return np.full((pix, gs), spec[1])
    if kind == "offset":
        r, sigma = spec[1], spec[2]
        return sigma * (r + (z - z.mean()) / z.std())
    if kind == "outlier":
        z[pix // 3, gs // 2] = spec[1]
        return z
    if kind == "chanscale":
        s = spec[1] * (spec[2] / spec[1]) ** (np.arange(gs) / (gs - 1))
        return z * s[rng.permutation(gs)]
    if kind == "nan":
        z = 0.3 + 1.5 * z
        z[pix // 2, gs // 3] = math.nan
        return z
    raise ValueError(spec)


class Act:
    """one normalised activation of an arm: x (N, H, W, C) float32 NHWC, its FiLM / affine parameters as the kernel gets them
    (mul, add: (N, C) float32; plus_one: the factor is 1 + mul), the valid extent the statistics are taken over"""

    def __init__(self, arm: str, h: int, w: int, c: int, plus_one: bool = True, valid: Optional[Tuple[int, int]] = None, shift: int = 0,
                 seed: int = 0):
        rng = np.random.default_rng([sum(map(ord, arm)), h, w, c, shift, seed])
        imgs = ARMS[arm]
        n, g, gs = len(imgs), groups_of(c), c // groups_of(c)
        hv, wv = valid or (h, w)
        x = rng.standard_normal((n, h, w, c)) * 1.5 + 0.3  # (beyond the valid extent: benign values that must not be read)
        m = rng.standard_normal((n, c)) * 0.3
        a = rng.standard_normal((n, c)) * 0.3
        for i, im in enumerate(imgs):
            for j in range(g):
                spec = group_spec(arm, i, j, shift)
                x[i, :hv, :wv, j * gs:(j + 1) * gs] = _fill(spec, rng, hv * wv, gs).reshape(hv, wv, gs)
            if im["film"] == "edges":
                ch = np.arange(c)
                m[i, ch % 4 == 0] = -1.0   # 1 + mul = 0: the output is add
                a[i, ch % 4 == 1] = 20.0
                a[i, ch % 4 == 2] = -20.0
                a[i, ch % 4 == 3] = -100.0  # exp overflows under SiLU: -0
        self.arm, self.n, self.h, self.w, self.c, self.hv, self.wv = arm, n, h, w, c, hv, wv
        self.plus_one = plus_one
        self.x = np.ascontiguousarray(x.astype(np.float32))
        self.mul = np.ascontiguousarray((m if plus_one else 1.0 + m).astype(np.float32))
        self.add = np.ascontiguousarray(a.astype(np.float32))

    def sums(self) -> np.ndarray:
        """(N, G, 1, 2) float64 sum and sum of squares over the valid extent: one statistics tile"""
        g = groups_of(self.c)
        v = self.x[:, :self.hv, :self.wv].astype(np.float64).reshape(self.n, -1, g, self.c // g)
        return np.ascontiguousarray(np.stack([v.sum(axis=(1, 3)), (v * v).sum(axis=(1, 3))], axis=-1)[:, :, None, :])

    def count(self) -> float:
        return float(self.hv * self.wv * (self.c // groups_of(self.c)))

    def normalised(self, dtype, silu: bool, eps: float = EPS, x: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(N, C, hv, wv) in `dtype`: the restatement on the valid extent"""
        x = tt(self.x, dtype) if x is None else x
        return norm_act(x[:, :self.hv, :self.wv].permute(0, 3, 1, 2), tt(self.mul, dtype),
                        tt(self.add, dtype), self.plus_one, silu, eps)


def norm_act(x_nchw: torch.Tensor, mul: Optional[torch.Tensor], add: Optional[torch.Tensor], plus_one: bool, silu: bool,
             eps: float = EPS) -> torch.Tensor:
    # contiguous NCHW on purpose: torch's channels-last GroupNorm forms E[x^2] - mean^2 in the tensor's own precision, and in
    # float32 that is off by 6e-5 at mean = 30 sigma -- no measuring stick; the NCHW kernel's moments are Welford's (1e-6 there)
    y = F.group_norm(x_nchw.contiguous(), groups_of(x_nchw.shape[1]), eps=eps)
    if mul is not None:
        y = y * ((1.0 + mul) if plus_one else mul)[:, :, None, None]
    if add is not None:
        y = y + add[:, :, None, None]
    return F.silu(y) if silu else y


def mean_rstd(sums: np.ndarray, count: float, eps: float = EPS) -> Tuple[np.ndarray, np.ndarray]:
    """what fp64 makes of (sum, sum of squares) partial tiles (..., T, 2): the kernels' own formula"""
    s = sums.astype(np.float64).sum(axis=-2)
    m = s[..., 0] / count
    var = np.maximum(s[..., 1] / count - m * m, 0.0)  # (NaN stays NaN)
    var = np.where(np.isnan(s[..., 1]), np.nan, var)
    return m, 1.0 / np.sqrt(var + eps)


def true_mean_rstd(x_nhwc: np.ndarray, hv: int, wv: int, eps: float = EPS) -> Tuple[np.ndarray, np.ndarray]:
    """two-pass float64 mean and rstd of every (image, group) over the valid extent"""
    n, _, _, c = x_nhwc.shape
    g = groups_of(c)
    v = x_nhwc[:, :hv, :wv].astype(np.float64).reshape(n, -1, g, c // g)
    m = v.mean(axis=(1, 3))
    var = ((v - m[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return m, 1.0 / np.sqrt(var + eps)


def conv(xs: Sequence[torch.Tensor], w: np.ndarray, bias: Optional[np.ndarray], dtype) -> torch.Tensor:
    """F.conv2d(cat(xs), w, bias, padding = k // 2) in `dtype`; NCHW"""
    k = w.shape[-1]
    b = None if bias is None else tt(bias, dtype)
    return F.conv2d(torch.cat(list(xs), dim=1), tt(w, dtype), b, padding=k // 2)


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def conv_weight(rng: np.random.Generator, cout: int, cin: int, k: int) -> np.ndarray:
    return (rng.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k)).astype(np.float32)


# ---- the two-convolution chain: the first convolution puts ITS OUTPUT into families 1 and 3 -------------------------------------------
# Every operand of the first convolution is a short dyadic number -- inputs are multiples of 2^-6 below 4 times a power of two per
# image, weights are +-2^-7 or +-2^-3 at a few positions, the bias is an integer -- so every product and every partial sum is exact
# in float32 AND in the split-fp16 arithmetic (h = x, l = 0), in any order: the kernel's intermediate is the float64 intermediate,
# bit for bit, and what the second convolution shows is the epilogue's statistics and the normalisation alone.  (A small-spread
# output made of small dense weights would leave the split arithmetic's contract instead: operands carry an absolute 2^-25.)
IMAGE_SCALE = (1.0, 0.5, 2.0)  # of the first convolution's input, per image
CHAIN_BIAS = 15.0


def dyadic_input(rng: np.random.Generator, shape: Tuple[int, ...]) -> np.ndarray:
    """N(0, 1) rounded to multiples of 2^-6, |x| < 4, times the image's scale"""
    z = np.clip(np.round(rng.standard_normal(shape) * 64.0) / 64.0, -3.984375, 3.984375)
    return (z * np.asarray(IMAGE_SCALE).reshape((-1,) + (1,) * (len(shape) - 1))).astype(np.float32)


def sparse_dyadic_weight(rng: np.random.Generator, cout: int, cin: int, k: int, kinds: Sequence[int]) -> np.ndarray:
    """group j of the output channels: kinds[j] == 1 -> one weight of +-2^-7 per channel (sigma = 0.0078 per unit input),
    kinds[j] == 3 -> 64 weights of +-2^-3 (sigma = 1)"""
    w = np.zeros((cout, cin * k * k), dtype=np.float32)
    for co in range(cout):
        cnt, mag = (1, 2.0 ** -7) if kinds[co // 32] == 1 else (64, 2.0 ** -3)
        pos = rng.choice(cin * k * k, size=min(cnt, cin * k * k), replace=False)
        w[co, pos] = mag * rng.choice([-1.0, 1.0], size=len(pos))
    return np.ascontiguousarray(w.reshape(cout, cin, k, k))


def chain_first_conv(rng: np.random.Generator, cout: int, cin: int, k: int, shift: int) -> Tuple[np.ndarray, np.ndarray, list, list]:
    """weights and bias of a first convolution whose output group j is
         family 1 (mean 0, sigma = 0.0078 s_image = 0.0078, 0.0039, 0.0156)                      for (j + shift) even,
         family 3 (mean 15, sigma = s_image: r = 15, 30, 7.5)                                  for (j + shift) odd;
    returns (w, bias, kinds, [(sigma per unit input scale, mean)] per group)"""
    kinds = [1 if (j + shift) % 2 == 0 else 3 for j in range(groups_of(cout))]
    w = sparse_dyadic_weight(rng, cout, cin, k, kinds)
    bias = np.zeros(cout, dtype=np.float32)
    claims = []
    for j, kind in enumerate(kinds):
        if kind == 3:
            bias[32 * j:32 * j + 32] = CHAIN_BIAS
        n_w = min(1 if kind == 1 else 64, cin * k * k)
        claims.append(((2.0 ** -7 if kind == 1 else 2.0 ** -3) * math.sqrt(n_w), 0.0 if kind == 1 else CHAIN_BIAS))
    return w, bias, kinds, claims


# ---- the 8x8 chains: ResBlocks (+ attention, concatenated skips) as models/blocks.py states them ------------------------------------
def attention(qkv_nchw: torch.Tensor, c: int) -> torch.Tensor:
    n, _, h, w = qkv_nchw.shape
    t = h * w
    q, k, v = qkv_nchw.reshape(n, 3, c // 8, 8, t).permute(0, 1, 2, 4, 3).unbind(1)
    att = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(8.0), dim=-1)
    return (att @ v).transpose(2, 3).reshape(n, c, h, w)


def lowres_chain(x_nhwc: np.ndarray, blocks: List[dict], dtype, eps: float = EPS) -> torch.Tensor:
    """blocks: dicts of float32 numpy parameters (w1, b1, w2, b2, f1 = (mul, add), f2 = (mul, add), cat, save, attn and then wqkv,
    bqkv, wo, bo, gam, bet; cat: wp, bp).  Returns NHWC."""
    t = lambda a: tt(a, dtype)
    cur = t(x_nhwc).permute(0, 3, 1, 2)
    slots = {0: cur}
    for b in blocks:
        inp = torch.cat([cur, slots[1]], dim=1) if b["cat"] else cur
        r = conv([inp], b["wp"], b["bp"], dtype) if b["cat"] else cur
        h = conv([norm_act(inp, t(b["f1"][0]), t(b["f1"][1]), True, True, eps)], b["w1"], b["b1"], dtype)
        cur = conv([norm_act(h, t(b["f2"][0]), t(b["f2"][1]), True, True, eps)], b["w2"], b["b2"], dtype) + r
        if b["attn"]:
            n = cur.shape[0]
            xn = norm_act(cur, t(b["gam"])[None].expand(n, -1), t(b["bet"])[None].expand(n, -1), False, False, eps)
            y = attention(conv([xn], b["wqkv"], b["bqkv"], dtype), cur.shape[1])
            cur = xn + conv([y], b["wo"], b["bo"], dtype)
        if b["save"] >= 0:
            slots[b["save"]] = cur
    return nhwc(cur)


@functools.lru_cache(maxsize=None)
def act(arm: str, h: int, w: int, c: int, plus_one: bool = True, valid: Optional[Tuple[int, int]] = None, shift: int = 0, seed: int = 0) -> Act:
    """computed once per case, shared by the tests, never written to"""
    a = Act(arm, h, w, c, plus_one, valid, shift, seed)
    for arr in (a.x, a.mul, a.add):
        arr.setflags(write=False)
    return a


# ---- the metric and the bounds' constants (tests/test_groupnorm_precision.py's docstring has the table; wgrad shares the backward's) ----
K_EXACT = 16.0  # exact-fp32 forward kernels
K_SPLIT = 10.0  # split-fp16 forward kernels
K_BWD = 30.0    # backward kernels (against float32 CPU autograd)
FLOOR_EXACT = 2.0 ** -24
FLOOR_SPLIT = 2.0 ** -20  # dmd_conv_f16ws.hip's header: 3-8e-7 of the output scale per convolution


def rows_errors(got, truth):
    """(B, M) tensors -> (B,): max |got - truth| of a row / max |truth| of the same row, non-finite entries left out; a row whose
    truth is zero throughout has error 0 where got is zero throughout too, else infinity"""
    fin = lambda x: torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(dim=1)
    d, s = fin(got.double() - truth.double()), fin(truth.double())
    return torch.where(s > 0, d / s.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
