"""Shared by the two runners of tests/test_linear_precision.py: the input families of dmd_linear, float64 truth and the metric,
written from include/diamond_hip.h:

    C[m, n] = sum_k A[m, k] W[n, k] (+ bias[n]) (+ C0[m, n]), then SiLU if asked.

Nothing here knows a kernel.  Truth is that sum in float64 over the float32 operands; S[m, n] = sum_k |A||W| + |bias| + |C0| is the
scale an order of float32 additions is accurate to, PER OUTPUT ELEMENT: ratio = |got - truth| / (2^-24 S), before SiLU.  Never a
launch maximum: a row 2^-12 below the launch's largest is held to its own S.  The stick is torch's float32 matmul on one thread.

C[m, n] depends on row m of A and row n of W alone, so a FAMILY is assigned per 16-row block of A and per 16-row block of W (the
MFMA's tile), and an ARM names the families of both sides: block j of a side with B blocks gets kinds[(j + r B) % len(kinds)] in
launch r (launches(): as many as the side that needs most to see every kind).  A value taken from the wrong block, row or k is a
wrong value.

  benign    N(0, 1)
  rowscale  row r of the block times 2^-2r (1 .. 2^-30)
  kquarter  the four quarters of K rounded up to 16 times 1, 2^-12, 2^-24, 2^12, rotated by the launch: which quarter is the large
            one moves, a quarter 2^-12 below it is 2^12 x the float32 resolution of the sum
  kstep     the k-th 16-wide step times 2^-(step % 8)
  offset    1 + 1e-3 N(0, 1): coherent sums
  posit     |N(0, 1)|
  impulse   each row nonzero at ONE k, which cycles over 0, 15, 16, 63, 64, Kp/4 - 1, Kp/4, K - 1 (those below K): against a dense
            row the output is a single product, float32(a w) bitwise; against an impulse at another k exactly +0
  zero      every second row all zero: outputs exactly 0, or exactly bias + C0

Chain lengths (csrc/dmd_linear.hip): Kp = K rounded up to 16; Kp >= 512 and Kp % 64 == 0 -> split-K, four chains of Kp / 4 and three
additions; otherwise one chain of Kp.
"""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import numpy as np
import torch

U = 2.0 ** -24
KINDS = ("benign", "rowscale", "kquarter", "kstep", "offset", "posit", "impulse", "zero")
# arm -> (kinds of A's blocks, kinds of W's blocks)
ARMS = {
    "benign": (("benign",), ("benign",)),
    "scales": (("rowscale", "kquarter", "kstep", "benign", "kquarter"), ("benign", "kstep", "rowscale", "kquarter")),
    "coherent": (("offset", "posit", "benign"), ("posit", "offset")),
    "exact": (("impulse", "zero", "impulse", "benign"), ("benign", "impulse", "zero")),
}


def pad16(k: int) -> int:
    return (k + 15) // 16 * 16


def splits(k: int) -> bool:
    """dmd_linear's rule, on the rounded K"""
    return pad16(k) >= 512 and pad16(k) % 64 == 0


def chain(k: int) -> int:
    """the longest serial float32 chain behind an output element"""
    return pad16(k) // 4 + 3 if splits(k) else pad16(k)


def blocks(rows: int) -> int:
    return -(-rows // 16)


def launches(arm: str, m: int, n: int) -> int:
    ak, wk = ARMS[arm]
    return max(-(-len(ak) // blocks(m)), -(-len(wk) // blocks(n)))


def kinds_of(arm: str, m: int, n: int, r: int) -> Tuple[tuple, tuple]:
    ak, wk = ARMS[arm]
    return (tuple(ak[(j + r * blocks(m)) % len(ak)] for j in range(blocks(m))),
            tuple(wk[(j + r * blocks(n)) % len(wk)] for j in range(blocks(n))))


def impulse_ks(k: int) -> list:
    kp = pad16(k)
    out = []
    for v in (0, 15, 16, 63, 64, kp // 4 - 1, kp // 4, k - 1):
        if 0 <= v < k and v not in out:
            out.append(v)
    return out


def block(kind: str, rng: np.random.Generator, k: int, r: int, shift: int = 0) -> np.ndarray:
    """(16, K) float64 values of one 16-row block; shift: where an impulse block begins in the cycle of k"""
    z = rng.standard_normal((16, k))
    ks, kp = np.arange(k), pad16(k)
    if kind == "benign":
        return z
    if kind == "rowscale":
        return z * (2.0 ** (-2 * np.arange(16)))[:, None]
    if kind == "kquarter":
        return z * np.roll(np.array([1.0, 2.0 ** -12, 2.0 ** -24, 2.0 ** 12]), r)[np.minimum(ks * 4 // kp, 3)][None, :]
    if kind == "kstep":
        return z * (2.0 ** -((ks // 16) % 8))[None, :]
    if kind == "offset":
        return 1.0 + 1e-3 * z
    if kind == "posit":
        return np.abs(z)
    if kind == "impulse":
        cyc, v = impulse_ks(k), np.zeros_like(z)
        for j in range(16):
            v[j, cyc[(j + r + shift) % len(cyc)]] = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
        return v
    if kind == "zero":
        z[1::2] = 0.0
        return z
    raise ValueError(kind)


def silu64(v: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return v / (1.0 + np.exp(-v))


def stick_f32(a: np.ndarray, w: np.ndarray, bias=None, c0=None) -> np.ndarray:
    """torch's float32 matmul on the CPU, on ONE thread: the order of its sums otherwise moves with the machine"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        c = torch.tensor(a) @ torch.tensor(w).t()
        if bias is not None:
            c = c + torch.tensor(bias)
        if c0 is not None:
            c = c + torch.tensor(c0)
        return c.numpy()
    finally:
        torch.set_num_threads(threads)


class Case:
    """one launch: a (M, K), w (N, K), bias (N) or None, c0 (M, N) or None, float32 as the kernel gets them, and what the
    assertions need, computed from those float32 arrays"""

    def __init__(self, a, w, bias=None, c0=None, a_kinds: tuple = (), w_kinds: tuple = ()):
        self.a, self.w, self.bias, self.c0, self.a_kinds, self.w_kinds = a, w, bias, c0, a_kinds, w_kinds
        a64, w64 = a.astype(np.float64), w.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            self.truth = a64 @ w64.T
            self.s = np.abs(np.nan_to_num(a64, nan=0.0, posinf=0.0, neginf=0.0)) @ np.abs(np.nan_to_num(w64, nan=0.0, posinf=0.0, neginf=0.0)).T
            if bias is not None:
                self.truth, self.s = self.truth + bias.astype(np.float64), self.s + np.abs(bias.astype(np.float64))
            if c0 is not None:
                self.truth, self.s = self.truth + c0.astype(np.float64), self.s + np.abs(c0.astype(np.float64))
        self.count = (a64 != 0).astype(np.float64) @ (w64 != 0).astype(np.float64).T  # products that reach an element
        # what an element no product reaches / one product reaches holds, in the kernel's float32 order: + bias, then + c0
        # (a single product of two float32 is exact in float64: its float32 rounding is np.float32(a) * np.float32(w))
        with np.errstate(invalid="ignore", over="ignore"):
            one = (a64 @ w64.T).astype(np.float32)
            if bias is not None:
                one = one + bias[None, :]
            if c0 is not None:
                one = one + c0
        self.few = one  # valid where count <= 1
        for arr in (self.a, self.w, self.truth, self.s, self.count, self.few):
            arr.setflags(write=False)

    @functools.cached_property
    def stick(self) -> np.ndarray:
        return stick_f32(self.a, self.w, self.bias, self.c0)

    def ratio(self, got: np.ndarray) -> np.ndarray:
        """|got - truth| / (2^-24 S) per element; where S = 0 (nothing reaches the element) 0 for an exact zero, inf otherwise"""
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.abs(got.astype(np.float64) - self.truth)
            return np.where(self.s > 0, d / (U * np.where(self.s > 0, self.s, 1.0)), np.where(got == 0, 0.0, np.inf))

    def block_max(self, ratio: np.ndarray) -> dict:
        """(A kind, W kind) -> the largest ratio over the blocks of that pair"""
        out = {}
        for i, ka in enumerate(self.a_kinds):
            for j, kw in enumerate(self.w_kinds):
                out[(ka, kw)] = max(out.get((ka, kw), 0.0), float(ratio[16 * i:16 * i + 16, 16 * j:16 * j + 16].max()))
        return out


@functools.lru_cache(maxsize=None)
def case(arm: str, m: int, n: int, k: int, r: int = 0, bias: bool = False, c0: bool = False) -> Case:
    """computed once, shared by the runners and routes, never written to"""
    ak, wk = kinds_of(arm, m, n, r)
    rng = np.random.default_rng([sum(map(ord, arm)), m, n, k, r])
    a = np.concatenate([block(kind, rng, k, r) for kind in ak])[:m].astype(np.float32)
    w = np.concatenate([block(kind, rng, k, r, shift=3) for kind in wk])[:n].astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32) if bias else None
    c = rng.standard_normal((m, n)).astype(np.float32) if c0 else None
    return Case(np.ascontiguousarray(a), np.ascontiguousarray(w), b, c, ak, wk)
