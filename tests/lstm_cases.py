"""Shared by the two runners of tests/test_lstm_cell_precision.py: the input families of dmd_lstm_pointwise(_bwd), the closed form in
float64 and in float32, and the metric.  Nothing here knows a kernel.

    i, f, o = sigmoid(gates i, f, o), g = tanh(gate g);  c = f c_prev + i g;  h = o tanh(c)
    dcv = dc + dh o (1 - tanh(c)^2);  dg_i = dcv g i (1 - i), dg_f = dcv c_prev f (1 - f), dg_g = dcv i (1 - g^2),
    dg_o = dh tanh(c) o (1 - o), dc_prev = dcv f

Truth is that in float64 of the float32 inputs -- for the backward INCLUDING c as given (the float32 rounding of the float64 cell
state, not a kernel's output) --, with 1 - sigmoid(x) = sigmoid(-x) and 1 - tanh(x)^2 = 1 / cosh(x)^2 so that float64 itself does
not cancel at a gate of +-20.  The stick is the formula as written above in float32 numpy.

An error is per element and relative to the UNCANCELLED scale of its output (the float32 factors 1 - i, 1 - tanh^2, 1 - o are
accurate to 2^-24 of 1, not of themselves), plus an absolute 2^-126 for expf's under- and overflow, where float32 holds an exact
0 or 1:

    S_c = |f c_prev| + |i g|     S_h = |o| min(1, S_c)     S_d = |dc| + |dh o|
    dg_i: S_d |g|   dg_f: S_d |c_prev|   dg_g: S_d |i|   dg_o: |dh tanh(c)|   dc_prev: S_d

A FAMILY is assigned per row of the batch, row j of launch r of N rows gets FAMILIES[(j + r N) % 8]: rows of different families share
a launch, so a value read from a neighbouring row, gate or column is a wrong value.

  benign     gates 2 N(0, 1), c_prev, dh, dc N(0, 1)
  saturated  gates 12 N(0, 1), c_prev 4 N(0, 1)
  gate-i/f/g/o   benign with that one gate at +-20 (the sign per column): a swapped gate or factor shows
  huge       gates +-200, c_prev +-60: sigmoid and tanh are exactly 0 / 1 / +-1, everything finite
  zero       benign with dh = dc = 0: dgates and dc_prev exactly 0
"""
from __future__ import annotations

import functools
import math

import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -126
CAP = 32.0
FAMILIES = ("benign", "saturated", "gate-i", "gate-f", "gate-g", "gate-o", "huge", "zero")
SHAPES = [(1, 1), (3, 40), (7, 64), (5, 103)]  # one element; a tail of the 256-thread block; two blocks; Hd no multiple of 4
ARMS = ("both", "dh-none", "dc-none")
FORWARD, BACKWARD = ("h", "c"), ("dg_i", "dg_f", "dg_g", "dg_o", "dc_prev")


def launches(n: int) -> int:
    return -(-len(FAMILIES) // n)


def families(n: int, r: int) -> tuple:
    return tuple(FAMILIES[(j + r * n) % len(FAMILIES)] for j in range(n))


@functools.lru_cache(maxsize=None)
def inputs(n: int, hd: int, r: int):
    """(gates (N, 4 Hd), c_prev, dh, dc, families), float32, read-only"""
    rng = np.random.default_rng([n, hd, r])
    gates, cp = 2.0 * rng.standard_normal((n, 4, hd)), rng.standard_normal((n, hd))
    dh, dc = rng.standard_normal((n, hd)), rng.standard_normal((n, hd))
    fam = families(n, r)
    for j, kind in enumerate(fam):
        sign = np.where((np.arange(hd) + j) % 2 == 0, 1.0, -1.0)
        if kind == "saturated":
            gates[j], cp[j] = 6.0 * gates[j], 4.0 * cp[j]
        elif kind.startswith("gate-"):
            gates[j, "ifgo".index(kind[-1])] = 20.0 * sign
        elif kind == "huge":
            gates[j] = 200.0 * rng.choice([-1.0, 1.0], (4, hd))
            cp[j] = 60.0 * rng.choice([-1.0, 1.0], hd)
        elif kind == "zero":
            dh[j], dc[j] = 0.0, 0.0
    out = tuple(np.ascontiguousarray(x.astype(np.float32)) for x in (gates.reshape(n, 4 * hd), cp, dh, dc))
    for x in out:
        x.setflags(write=False)
    return out + (fam,)


def _gates(gates, dtype):
    n, hd4 = gates.shape
    return gates.astype(dtype).reshape(n, 4, hd4 // 4).transpose(1, 0, 2)


def sig64(x):
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x)))


def sech2(x):
    with np.errstate(over="ignore"):
        return 4.0 / (np.exp(x) + np.exp(-x)) ** 2


def forward64(gates, cp):
    """-> ({h, c}, {their scales})"""
    gi, gf, gg, go = _gates(gates, np.float64)
    cp = cp.astype(np.float64)
    i, f, g, o = sig64(gi), sig64(gf), np.tanh(gg), sig64(go)
    c = f * cp + i * g
    s_c = np.abs(f * cp) + np.abs(i * g)
    return dict(h=o * np.tanh(c), c=c), dict(h=np.abs(o) * np.minimum(1.0, s_c), c=s_c)


def backward64(gates, cp, c_new, dh, dc):
    """dh / dc None: a zero gradient.  -> ({dg_i, dg_f, dg_g, dg_o, dc_prev}, {their scales})"""
    gi, gf, gg, go = _gates(gates, np.float64)
    cp, cn = cp.astype(np.float64), c_new.astype(np.float64)
    dh = np.zeros_like(cp) if dh is None else dh.astype(np.float64)
    dc = np.zeros_like(cp) if dc is None else dc.astype(np.float64)
    i, f, g, o = sig64(gi), sig64(gf), np.tanh(gg), sig64(go)
    tc = np.tanh(cn)
    dcv = dc + dh * o * sech2(cn)
    s_d = np.abs(dc) + np.abs(dh * o)
    val = dict(dg_i=dcv * g * i * sig64(-gi), dg_f=dcv * cp * f * sig64(-gf), dg_g=dcv * i * sech2(gg), dg_o=dh * tc * o * sig64(-go),
               dc_prev=dcv * f)
    scale = dict(dg_i=s_d * np.abs(g), dg_f=s_d * np.abs(cp), dg_g=s_d * np.abs(i), dg_o=np.abs(dh * tc), dc_prev=s_d)
    return val, scale


def _sig32(x):
    with np.errstate(over="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-x))


def forward32(gates, cp):
    gi, gf, gg, go = _gates(gates, np.float32)
    i, f, g, o = _sig32(gi), _sig32(gf), np.tanh(gg), _sig32(go)
    c = f * cp + i * g
    return dict(h=o * np.tanh(c), c=c)


def backward32(gates, cp, c_new, dh, dc):
    gi, gf, gg, go = _gates(gates, np.float32)
    one = np.float32(1.0)
    dh = np.zeros_like(cp) if dh is None else dh
    dc = np.zeros_like(cp) if dc is None else dc
    i, f, g, o = _sig32(gi), _sig32(gf), np.tanh(gg), _sig32(go)
    tc = np.tanh(c_new)
    dcv = dc + dh * o * (one - tc * tc)
    out = dict(dg_i=dcv * g * i * (one - i), dg_f=dcv * cp * f * (one - f), dg_g=dcv * i * (one - g * g), dg_o=dh * tc * o * (one - o),
               dc_prev=dcv * f)
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def ratio(got, truth, scale):
    """|got - truth| / (2^-24 scale + 2^-126), per element"""
    return np.abs(got.astype(np.float64) - truth) / (U * scale + FLOOR)


def arm_grads(arm: str, dh, dc):
    return (None if arm == "dh-none" else dh), (None if arm == "dc-none" else dc)


def split_dgates(dg):
    """(N, 4 Hd) -> dg_i, dg_f, dg_g, dg_o"""
    n, hd4 = dg.shape
    return dict(zip(BACKWARD[:4], dg.reshape(n, 4, hd4 // 4).transpose(1, 0, 2)))


def by_family(fam, ratios: dict) -> dict:
    """(family, output) -> the largest ratio over the rows of that family"""
    out = {}
    for name, r in ratios.items():
        for j, kind in enumerate(fam):
            out[(kind, name)] = max(out.get((kind, name), 0.0), float(r[j].max()))
    return out


@functools.lru_cache(maxsize=None)
def stick_table(arm: str) -> dict:
    """(family, output) -> the float32 formula's largest ratio over every shape and launch of the arm: one figure per (family,
    output), so that a launch of a single element is not held to the accident of that element"""
    table = {}
    for n, hd in SHAPES:
        for r in range(launches(n)):
            gates, cp, dh, dc, fam = inputs(n, hd, r)
            dh_, dc_ = arm_grads(arm, dh, dc)
            t, s = forward64(gates, cp)
            c_new = t["c"].astype(np.float32)
            tb, sb = backward64(gates, cp, c_new, dh_, dc_)
            got = {**forward32(gates, cp), **backward32(gates, cp, c_new, dh_, dc_)}
            t.update(tb)
            s.update(sb)
            for key, v in by_family(fam, {k: ratio(got[k], t[k], s[k]) for k in got}).items():
                table[key] = max(table.get(key, 0.0), v)
    return table


def limit(arm: str, family: str, output: str) -> float:
    """4 x the stick (expf / tanhf of another library may differ by an ulp or two per factor, over up to five factors), never
    above 32 x 2^-24 of the uncancelled scale"""
    return min(4.0 * stick_table(arm)[(family, output)], CAP)
