"""Shared by the two runners of tests/test_wgrad_precision.py: the input families of the weight-gradient kernels and float64 /
float32 RESTATEMENTS of what dmd_conv2d_wgrad computes, written from include/diamond_hip.h:

    dw[co][ci][ky][kx] = sum_{n, y, x} dy[n, y, x, co] * a[n, y + ky - pad, x + kx - pad, ci],   db[co] = sum dy[n, y, x, co]

over the valid extent, a = 0 outside it.  Truth is that sum in float64 over the float32 inputs (one matrix product per tap); the
measuring stick is float32 F.conv2d autograd on the CPU.  Nothing here knows a kernel.

dw[co][ci] depends on dy[..., co] and a[..., ci] alone, so a FAMILY is assigned per 16-channel block of dy and per 16-channel block
of the source, and an ARM names the families of both sides: block j of a side with B blocks gets kinds[(j + r B) % len(kinds)] in
launch r of the arm (launches(): as many as the shorter side needs to see every kind).  A value taken from the wrong block, tap,
pixel or image is then a wrong value.

Families of dy (float32; the launch maximum is O(1) as grad_ops.pow2_scaled leaves it, family 7 and the 1e5 apart):
  0 benign    N(0, 1)
  1 chan4 / chan2   channel c of the block is 2^-2c (1 .. 2^-30) / 2^-c (1 .. 2^-15) times N(0, 1)
  2 pooled    N(0, 1) times a mask with exactly one nonzero per 2x2 window, its place drawn per (window, channel): maxpool2_bwd's dy
  3 impulse   zero except single pixels: image 0 at (0, 0), image 1 at (hv - 1, wv - 1), image 2 around the sub-tile seam
              (7, 7), (7, 8), (8, 7), (8, 8) as far as they exist, every impulse with its own value per channel and in its own
              channels of the block (the images are summed: an element is then a SINGLE product or an exact zero); with a valid
              extent also just OUTSIDE it ((hv, 3), (3, wv), (hv - 1, wv)), which must contribute nothing
  4 offset    1 + 1e-3 N(0, 1): coherent sums, the bias gradient's worst case
  5 checker   0.75 (-1)^(y + x): against the constant source the centre tap's truth is exactly 0, what remains is the border taps
  6 imgscale / imgzero   images at 1, 2^-12, 2^-24 of N(0, 1) / image 1 all zero
  7 range     1e4 N(0, 1) clamped to +-65000, single entries at +-65504 (the last finite fp16)
  8 nonfinite / big   one NaN, one +Inf, one -Inf at interior pixels of three channels / one finite 1e5
Source blocks (raw, DMD_PROLOGUE_NONE): benign 1.3 N(0, 1) + 0.2; const 0.6; posit |benign|; frames k / 255 * 2 - 1 (always the LAST
block, with cin_real = C - 1 or C - 13 and the padding channels zero); chan2; range; big.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

FAMILY = dict(benign=0, chan4=1, chan2=1, pooled=2, impulse=3, offset=4, checker=5, imgscale=6, imgzero=6, range=7, nonfinite=8, big=8)
BIG = 1.0e5  # finite, beyond fp16: outside the split-fp16 operand contract

# arm -> (dy kinds, source kinds, channels cut off the source: cin_real = C - cut, the last block then holds frame levels)
ARMS: Dict[str, Tuple[tuple, tuple, int]] = {
    "scales": (("chan4", "benign", "chan2", "benign"), ("benign", "chan2"), 0),
    "sparse": (("pooled", "impulse", "benign", "pooled"), ("benign", "posit"), 0),
    # The constant source meets only dy families whose sum against a constant is exact or coherent.  A zero-mean dy against it
    # makes all 16 k k elements of a row the SAME cancelling sum, 0.6 sum dy: max |truth| of the row is then as small as chance
    # has it, and the row's relative error measures that chance, not the kernel (the bias gradient has the same shape: see
    # Case.scale_db).
    "checker": (("checker", "offset", "impulse", "checker"), ("const", "benign"), 0),
    "coherent": (("offset", "benign", "imgscale", "imgzero"), ("posit", "benign"), 0),
    "range": (("range", "benign"), ("benign", "range"), 0),
    "nonfinite": (("nonfinite", "benign"), ("benign", "chan2"), 0),
    "big-dy": (("big", "benign", "offset"), ("benign", "posit"), 0),
    "big-src": (("benign", "pooled"), ("big", "benign"), 0),
    "frames15": (("benign", "pooled"), ("benign",), 1),
    "frames3": (("impulse", "benign"), ("benign",), 13),
}
CHAN_SCALE = dict(chan4=lambda c: 2.0 ** (-2 * c), chan2=lambda c: 2.0 ** -c)


def launches(arm: str, nco: int, nci: int) -> int:
    dyk, srck, _ = ARMS[arm]
    return max(-(-len(dyk) // nco), -(-len(srck) // nci))


def kinds_of(arm: str, nco: int, nci: int, r: int) -> Tuple[tuple, tuple]:
    dyk, srck, cut = ARMS[arm]
    dk = tuple(dyk[(j + r * nco) % len(dyk)] for j in range(nco))
    sk = tuple(srck[(j + r * nci) % len(srck)] for j in range(nci))
    return dk, (sk[:-1] + ("frames",) if cut else sk)


def impulse_pixels(h: int, w: int, hv: int, wv: int):
    """(inside, outside): (image, y, x) of the impulses inside the valid extent, and of those in the margin just beyond it"""
    inside = [(0, 0, 0), (1, hv - 1, wv - 1)] + [(2, y, x) for y in (7, 8) for x in (7, 8) if y < hv and x < wv]
    outside = [(i, y, x) for i, y, x in ((0, hv, 3), (1, 3, wv), (2, hv - 1, wv)) if y < h and x < w]
    return inside, outside


def _range_end(rng, shape):
    v = np.clip(1e4 * rng.standard_normal(shape), -65000.0, 65000.0)
    v[0, 1, 2, 3], v[1, 2, 3, 5], v[2, 5, 4, 11], v[2, 6, 1, 7] = 65504.0, -65504.0, 65504.0, -65504.0
    return v


def dy_block(kind: str, rng: np.random.Generator, n: int, h: int, w: int, hv: int, wv: int) -> np.ndarray:
    """(n, h, w, 16) float64 values of one 16-channel block of dy"""
    z = rng.standard_normal((n, h, w, 16))
    c = np.arange(16)
    if kind == "benign":
        return z
    if kind in CHAN_SCALE:
        return z * CHAN_SCALE[kind](c)
    if kind == "pooled":
        place = rng.integers(0, 4, size=(n, h // 2, w // 2, 16)).repeat(2, axis=1).repeat(2, axis=2)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return z * (place == ((yy % 2) * 2 + xx % 2)[None, :, :, None])
    if kind == "impulse":
        v = np.zeros_like(z)
        inside, outside = impulse_pixels(h, w, hv, wv)
        for j, (i, y, x) in enumerate(inside):  # impulse j lives in the channels c with c % len(inside) == j: the three images are
            mine = c % len(inside) == j         # summed, and an element that one impulse reaches is then ONE product
            v[i, y, x, mine] = (rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16))[mine]
        for i, y, x in outside:
            v[i, y, x] = rng.uniform(0.5, 2.0, 16) * rng.choice([-1.0, 1.0], 16)
        return v
    if kind == "offset":
        return 1.0 + 1e-3 * z
    if kind == "checker":
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return np.broadcast_to((0.75 * (-1.0) ** (yy + xx))[None, :, :, None], z.shape).copy()
    if kind == "imgscale":
        return z * np.array([1.0, 2.0 ** -12, 2.0 ** -24])[(np.arange(n) % 3), None, None, None]
    if kind == "imgzero":
        z[1] = 0.0
        return z
    if kind == "range":
        return _range_end(rng, z.shape)
    if kind == "nonfinite":
        z[0, 3, 3, 2], z[1, 4, 2, 5], z[2, 2, 5, 9] = math.nan, math.inf, -math.inf
        return z
    if kind == "big":
        z[1, 3, 4, 6] = BIG
        return z
    raise ValueError(kind)


def src_block(kind: str, rng: np.random.Generator, n: int, h: int, w: int) -> np.ndarray:
    z = rng.standard_normal((n, h, w, 16))
    if kind == "benign":
        return 1.3 * z + 0.2
    if kind == "posit":
        return np.abs(1.3 * z + 0.2)
    if kind == "const":
        return np.full_like(z, 0.6)
    if kind == "frames":
        return (rng.integers(0, 256, size=z.shape).astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float64)
    if kind == "chan2":
        return z * CHAN_SCALE["chan2"](np.arange(16))
    if kind == "range":
        return _range_end(rng, z.shape)
    if kind == "big":
        z = 1.3 * z + 0.2
        z[2, 4, 3, 3] = BIG
        return z
    raise ValueError(kind)


# ---- the operand contract of the split-fp16 weight gradient (include/diamond_hip.h, dmd_wgrad_params.precision) --------------------
def e_split(x: np.ndarray) -> np.ndarray:
    """|x - (h + l)| <= max(2^-22 |x|, 2^-25) for |x| < 65520; an exact zero is kept exactly"""
    x = np.abs(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0))
    return np.where(x > 0, np.maximum(2.0 ** -22 * x, 2.0 ** -25), 0.0)


def split_hl(x: np.ndarray) -> np.ndarray:
    """h + l of wg_pack_hl, in float64: h = fp16(x), l = fp16(fp32(x - h))"""
    x = x.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        l = (x - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float64), l.astype(np.float64)


def tap_sums(g: np.ndarray, a: np.ndarray, k: int) -> np.ndarray:
    """(Cout, Cin, k, k): sum over images and pixels of g[n, y, x, co] a[n, y + ky - pad, x + kx - pad, ci], a zero outside; in the
    arrays' own precision"""
    n, h, w, co = g.shape
    pad = k // 2
    ap = np.pad(a, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.zeros((co, a.shape[-1], k, k), dtype=g.dtype)
    gm = g.reshape(-1, co).T
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(k):
            for kx in range(k):
                out[:, :, ky, kx] = gm @ ap[:, ky:ky + h, kx:kx + w].reshape(-1, a.shape[-1])
    return out


def stick_f32(dy: np.ndarray, a: np.ndarray, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """float32 F.conv2d autograd on the CPU: (dw, db).  On ONE thread: the order of torch's sums, and with it the stick's own
    error, otherwise moves with the thread count of the machine that runs the test."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        w = torch.zeros(dy.shape[-1], a.shape[-1], k, k, requires_grad=True)
        b = torch.zeros(dy.shape[-1], requires_grad=True)
        y = F.conv2d(torch.tensor(a, dtype=torch.float32).permute(0, 3, 1, 2), w, b, padding=k // 2)
        y.backward(torch.tensor(dy, dtype=torch.float32).permute(0, 3, 1, 2))
        return w.grad, b.grad
    finally:
        torch.set_num_threads(threads)


class Case:
    """one launch: x (N, H, W, C) and dy (N, H, W, Cout) float32 as the kernel gets them, and everything the assertions need,
    computed from the valid extent of those float32 arrays (a64: the float64 activations, x itself for a raw source)"""

    def __init__(self, x: np.ndarray, dy: np.ndarray, k: int, cin_real: int, valid: Optional[Tuple[int, int]] = None,
                 a64: Optional[np.ndarray] = None, a32: Optional[np.ndarray] = None, dy_kinds: tuple = (), src_kinds: tuple = ()):
        n, h, w, c = x.shape
        hv, wv = valid or (h, w)
        self.x, self.dy, self.k, self.cin_real, self.valid, self.hv, self.wv = x, dy, k, cin_real, valid, hv, wv
        self.dy_kinds, self.src_kinds = dy_kinds, src_kinds
        g = dy[:, :hv, :wv].astype(np.float64)
        a = (x[:, :hv, :wv].astype(np.float64) if a64 is None else a64)[..., :cin_real]
        self.g, self.a = g, a
        self.truth = tap_sums(g, a, k)
        with np.errstate(invalid="ignore"):
            self.truth_db = g.reshape(-1, g.shape[-1]).sum(axis=0)
        a_stick = (x[:, :hv, :wv] if a32 is None else a32)[..., :cin_real]
        self.stick, self.stick_db = stick_f32(dy[:, :hv, :wv], a_stick, k)
        # the split-fp16 allowance, per element: A = sum_pixels e(dy) |a| + |dy| e(a) + e(dy) e(a), and its root-sum-square form
        fin = lambda v: np.abs(np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0))
        eg, ea, ag, aa = e_split(g), e_split(a), fin(g), fin(a)
        self.allow = tap_sums(eg, aa, k) + tap_sums(ag, ea, k) + tap_sums(eg, ea, k)
        self.rss = np.sqrt(tap_sums(eg ** 2, aa ** 2, k) + tap_sums(ag ** 2, ea ** 2, k) + tap_sums(eg ** 2, ea ** 2, k))
        # how many products reach an element: 0 -> exactly zero by construction, 1 -> that product
        nz = lambda v: (np.nan_to_num(v, nan=1.0, posinf=1.0, neginf=1.0) != 0).astype(np.float64)
        self.count = tap_sums(nz(g), nz(a), k)
        # ... and how many of them have both operands in the contract's RELATIVE range, 2^-3 <= |x| (below it l is a fp16 subnormal)
        rel = lambda v: ((fin(v) >= 0.125) & np.isfinite(v)).astype(np.float64)
        self.count_rel = tap_sums(rel(g), rel(a), k)
        self.scale_db = np.maximum(fin(self.truth_db), np.sqrt((fin(g) ** 2).reshape(-1, g.shape[-1]).sum(axis=0)))
        self.count_db = nz(g).reshape(-1, g.shape[-1]).sum(axis=0)  # nonzero entries of dy per channel
        # rows (co) / columns (ci) holding a non-finite operand, or a finite one beyond fp16 (which the split routes turn into NaN)
        gm, am = g.reshape(-1, g.shape[-1]), a.reshape(-1, a.shape[-1])
        self.bad_rows, self.bad_cols = ~np.isfinite(gm).all(axis=0), ~np.isfinite(am).all(axis=0)
        with np.errstate(invalid="ignore"):
            self.big_rows, self.big_cols = (np.abs(gm) >= 65520.0).any(axis=0) & ~self.bad_rows, (np.abs(am) >= 65520.0).any(axis=0) & ~self.bad_cols
        for arr in (self.x, self.dy, self.truth, self.truth_db, self.allow, self.rss, self.count):
            arr.setflags(write=False)


def _assemble(arm: str, nco: int, nci: int, n: int, h: int, w: int, r: int, valid, margins_nan: bool):
    dk, sk = kinds_of(arm, nco, nci, r)
    cut = ARMS[arm][2]
    hv, wv = valid or (h, w)
    rng = np.random.default_rng([sum(map(ord, arm)), nco, nci, n, h, w, r, hv, wv])
    dy = np.concatenate([dy_block(kind, rng, n, h, w, hv, wv) for kind in dk], axis=-1)
    x = np.concatenate([src_block(kind, rng, n, h, w) for kind in sk], axis=-1)
    cin_real = 16 * nci - cut
    x[..., cin_real:] = 0.0
    if margins_nan:  # whatever the margins hold is never read -- except the impulses there, finite on purpose: they must not count
        _, outside = impulse_pixels(h, w, hv, wv)
        keep = np.zeros((n, h, w), dtype=bool)
        for i, y, xx in outside:
            keep[i, y, xx] = True
        margin = np.ones((n, h, w), dtype=bool)
        margin[:, :hv, :wv] = False
        dy[margin & ~keep] = math.nan
        x[margin] = math.nan
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(dy.astype(np.float32)), cin_real, dk, sk


@functools.lru_cache(maxsize=None)
def case(arm: str, nco: int, nci: int, taps: int, n: int, h: int, w: int, r: int = 0, valid: Optional[Tuple[int, int]] = None,
         margins_nan: bool = False) -> Case:
    """computed once, shared by the runners and routes, never written to"""
    x, dy, cin_real, dk, sk = _assemble(arm, nco, nci, n, h, w, r, valid, margins_nan)
    return Case(x, dy, 3 if taps == 9 else 1, cin_real, valid, dy_kinds=dk, src_kinds=sk)


def block_rows(dw, nci: int) -> torch.Tensor:
    """(Cout, cin_real, k, k) -> (Cout * nci, 16 k k): one row per (output channel, 16-channel source block); the channels beyond
    cin_real (never written, never part of the gradient) are zero on both sides"""
    dw = torch.as_tensor(np.asarray(dw)) if not torch.is_tensor(dw) else dw
    co, ci, k, _ = dw.shape
    full = torch.zeros(co, 16 * nci, k, k, dtype=dw.dtype)
    full[:, :ci] = dw
    return full.reshape(co * nci, 16 * k * k)
