"""dmd_linear's numerics away from benign N(0, 1) operands: every nn.Linear of the three networks and the LSTM's GEMMs, all four
instances (linear_mfma_kernel / linear_mfma_t_kernel, plain and split-K), on the SIMT interpreter and on the device (-m gpu), through
the same C ABI (tests/abi.py), the same inputs and the same assertions.  C and the padding of every leading dimension start as NaN.

Inputs, truth and metric: tests/linear_cases.py.  ratio = |got - float64 truth| / (2^-24 S) PER OUTPUT ELEMENT, S = sum |a||w| +
|bias| + |c0|, taken before SiLU.

Bounds
  rigorous   ratio <= L + 4, L the longest serial float32 chain behind an element (Kp on the plain route, Kp / 4 + 3 on split-K);
             the 4: bias, accumulate, and the second-order terms.  The standard bound of a float32 sum of L terms: no order of
             correct float32 additions can exceed it, a dropped term or a product of reduced precision does.
  expected   ratio <= 2 sqrt(L) + 8: what rounding errors that do not conspire give, with room (the largest interpreter figures,
             coherent sums on one chain of 1008, sit 2.4x below it: profiles/linear_precision.txt).
  exact      an element no product reaches is exactly +0 (or float32(bias + c0)); one that ONE product reaches is float32(a w) bitwise.
  routes     split-K exactly where Kp >= 512 and Kp % 64 == 0, summed ((w0 + w1) + w2) + w3: bitwise that combination of four
             plain launches on the K quarters where the rule splits, and NOT that combination where it does not.
  the rest   power-of-two scaling, the storage order, a K tail, the leading dimensions and the operands' alignment change no bit;
             a NaN / Inf stays in its row / column; bias, then accumulate, then SiLU.
"""
import math

import numpy as np
import pytest

from tests import abi
from tests import linear_cases as LC

# the smallest shapes that reach every path: ragged 16- / 32- / 64-tiles, the clamp rows, one row, one column; K below LIN_DEPTH
# steps (16, 48), with a tail (72, 1000, 1020), split (512, 576, 1020 -> 1024, 1024, 2048) and not (496, 528, 608, 1000 -> 1008)
SHAPE_OF_K = {16: (70, 33), 48: (33, 70), 72: (48, 48), 256: (5, 70), 496: (70, 1), 512: (70, 48), 528: (33, 33), 576: (1, 70),
              608: (48, 5), 1000: (33, 70), 1020: (70, 33), 1024: (48, 70), 2048: (70, 70)}
KS = tuple(SHAPE_OF_K)
# arm -> (bias, c0) variants
VARIANTS = {"benign": [(True, True)], "scales": [(False, False)], "coherent": [(True, False)], "exact": [(False, False), (True, True)]}
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_bits(x, y):
    return x.shape == y.shape and bool((bits(x) == bits(y)).all())


def launch(run, a, w, bias=None, c0=None, pad=(0, 0, 3), **kw):
    """abi.linear with ldc = N + 3 unless asked otherwise: the padding columns of C must still be NaN afterwards"""
    got, storage = abi.linear(run, a, w, bias, c0, pad=pad, **kw)
    assert np.isnan(storage[:, got.shape[1]:]).all(), "the call wrote beyond column N of C"
    return got


def check_case(run, tag, c, got, k):
    """print the largest ratio of every (A family, W family) pair beside torch's, then assert the module's bounds and exact values"""
    L = LC.chain(k)
    ratio, torch_ratio = c.ratio(got), c.ratio(c.stick)
    mine, theirs = c.block_max(ratio), c.block_max(torch_ratio)
    rigorous, expected = L + 4, 2 * math.sqrt(L) + 8
    for pair in mine:
        print(f"LINPREC {run.name} {tag} K={k} {'split' if LC.splits(k) else 'plain'} a={pair[0]} w={pair[1]}: ratio {mine[pair]:.2f} "
              f"torch {theirs[pair]:.2f} expected {expected:.1f} rigorous {rigorous}")
    assert np.isfinite(got).all()
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert float(ratio.max()) <= rigorous, (float(ratio.max()), worst)
    assert float(ratio.max()) <= expected, (float(ratio.max()), worst)
    few = c.count <= 1
    assert bool((bits(got)[few] == bits(c.few)[few]).all()), \
        f"{int((bits(got)[few] != bits(c.few)[few]).sum())} elements that at most one product reaches are not that product / +0 / bias + c0"


@pytest.mark.parametrize("run,arm,k", abi.arms(abi.Simt, abi.Gpu, [(arm, k) for arm in VARIANTS for k in KS]))
def test_error_per_element(run, arm, k):
    m, n = SHAPE_OF_K[k]
    for bias, c0 in VARIANTS[arm]:
        for r in range(LC.launches(arm, m, n)):
            c = LC.case(arm, m, n, k, r, bias, c0)
            check_case(run, f"{arm}{'+bias+c0' if c0 else '+bias' if bias else ''} r{r} {m}x{n}", c, launch(run, c.a, c.w, c.bias, c.c0), k)


# the storage orders on a subset: a tail, a split tail, split, the plain route above 512
@pytest.mark.parametrize("run,shape,mode", abi.arms(abi.Simt, abi.Gpu, [(s, mo) for s in [(33, 5, 72), (5, 33, 1000), (48, 70, 512), (70, 48, 528), (33, 48, 1020)]
                                                                      for mo in MODES[1:]]))
def test_storage_orders_and_leading_dimensions(run, shape, mode):
    """either operand given as (K, rows), lda / ldw / ldc wider than the rows by NaN floats: the bounds, and bitwise the plain call
    on K-contiguous copies zero-padded to K rounded up to 16"""
    m, n, k = shape
    ta, tw = mode
    c = LC.case("scales", m, n, k, 0, True, True)
    got = launch(run, c.a, c.w, c.bias, c.c0, trans_a=ta, trans_w=tw, pad=(3, 1, 2))
    check_case(run, f"scales+bias+c0 {m}x{n} trans={ta}{tw}", c, got, k)
    zp = lambda x: np.pad(x, ((0, 0), (0, LC.pad16(k) - k)))
    assert same_bits(got, launch(run, zp(c.a), zp(c.w), c.bias, c.c0, pad=(0, 0, 0)))


@pytest.mark.parametrize("run,k", abi.arms(abi.Simt, abi.Gpu, list(KS)))
def test_split_k_rule_and_order(run, k):
    """Kp >= 512 and Kp % 64 == 0: C is ((c0 + c1) + c2) + c3 bitwise, ci = dmd_linear on the i-th Kp / 4 slice of the zero-padded
    operands (a slice below 512 takes the plain route, whose chain over the slice is a wave's chain over its quarter).  Any other
    K: C is NOT that combination on positive operands (every reordering of such a sum moves some of 33 x 48 elements) -- equal
    means the route changed.  K = 2048: a quarter is 512 and no launch runs that as ONE chain, so the slices are no restatement
    there (the figure is printed); test_split_k_order_in_exact_arithmetic pins that K."""
    m, n = 33, 48
    rng = np.random.default_rng(k)
    a, w = np.abs(rng.standard_normal((m, k))).astype(np.float32), np.abs(rng.standard_normal((n, k))).astype(np.float32)
    kp = LC.pad16(k)
    ap, wp = np.pad(a, ((0, 0), (0, kp - k))), np.pad(w, ((0, 0), (0, kp - k)))
    got = launch(run, a, w)
    q = kp // 4
    part = [launch(run, ap[:, i * q:(i + 1) * q], wp[:, i * q:(i + 1) * q]) for i in range(4)]
    comb = ((part[0] + part[1]) + part[2]) + part[3]
    assert comb.dtype == np.float32
    differing = int((bits(got) != bits(comb)).sum())
    print(f"LINPREC {run.name} route K={k} Kp={kp} rule={'split' if LC.splits(k) else 'plain'}: {differing} of {m * n} elements differ from ((c0 + c1) + c2) + c3")
    if not LC.splits(k):
        assert differing > 0
    elif not LC.splits(q):
        assert differing == 0


def _f32_sum(values):
    s = np.float32(0.0)
    for v in values:
        s = np.float32(s + np.float32(v))
    return s


@pytest.mark.parametrize("run,k", abi.arms(abi.Simt, abi.Gpu, [k for k in KS if LC.splits(k)]))
def test_split_k_order_in_exact_arithmetic(run, k):
    """Five single products per element -- one in quarter 0, two in quarter 1 (in different 16-wide steps), one each in quarters 2
    and 3 -- whose values are every arrangement of (2^24, -2^24, 1, 1, 1): each float32 addition is then exact or a tie, and the
    result names the order.  It must be ((w0 + w1) + w2) + w3 of the quarters' own chains; one chain over K, (w0 + w1) + (w2 + w3)
    and wave 0 added last each give other values on some arrangement (asserted of the arithmetic, without a kernel)."""
    import itertools

    kp = LC.pad16(k)
    q = kp // 4
    ks = [3, q + 1, q + 20, 2 * q + 5, min(4 * q, k) - 1]
    cols = sorted(set(itertools.permutations((2.0 ** 24, -2.0 ** 24, 1.0, 1.0, 1.0))))
    a = np.zeros((5, k), dtype=np.float32)
    a[:, ks] = 1.0
    w = np.zeros((len(cols), k), dtype=np.float32)
    w[:, ks] = np.array(cols, dtype=np.float32)
    quarters = lambda v: (_f32_sum(v[:1]), _f32_sum(v[1:3]), _f32_sum(v[3:4]), _f32_sum(v[4:]))
    want = np.array([_f32_sum(quarters(v)) for v in cols], dtype=np.float32)
    others = {"one chain": [_f32_sum(v) for v in cols],
              "pairs": [np.float32(_f32_sum(quarters(v)[:2]) + _f32_sum(quarters(v)[2:])) for v in cols],
              "wave 0 last": [_f32_sum(quarters(v)[1:] + quarters(v)[:1]) for v in cols]}
    for name, o in others.items():
        assert not same_bits(np.array(o, dtype=np.float32), want), name
    got = launch(run, a, w)
    assert same_bits(got, np.broadcast_to(want, got.shape)), [(cols[j], float(got[0, j]), float(want[j])) for j in np.nonzero(bits(got[0]) != bits(want))[0][:4]]


@pytest.mark.parametrize("run,arm,k", abi.arms(abi.Simt, abi.Gpu, [("benign", 72), ("scales", 512), ("scales", 1000), ("coherent", 528)]))
def test_power_of_two_invariance(run, arm, k):
    m, n = SHAPE_OF_K[k]
    c = LC.case(arm, m, n, k, 0)
    assert same_bits(launch(run, c.a * np.float32(2.0 ** 40), c.w * np.float32(2.0 ** -40)), launch(run, c.a, c.w))


# ---- the epilogue: a K = 16 impulse product feeds chosen pre-activations ---------------------------------------------------------------
def feed(run, v, bias=None, c0=None, silu=False, m=5):
    """C[i, j] = 1 * v[j] (+ bias[j]) (+ c0[i, j]): row i of A is 1 at k = i % 16, W[j] holds v[j] at every k"""
    a = np.zeros((m, 16), dtype=np.float32)
    a[np.arange(m), np.arange(m) % 16] = 1.0
    w = np.repeat(np.asarray(v, dtype=np.float32)[:, None], 16, axis=1)
    return launch(run, a, w, bias, c0, silu=silu)


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_silu_range(run):
    """|v| <= 87: relative error <= 4 x 2^-24 against float64; v < -88.8: below 2^-126 in magnitude and not positive (expf
    overflows: v / inf); v > 88.8: v exactly (expf underflows against 1); NaN gives NaN"""
    rng = np.random.default_rng(7)
    mid = np.concatenate([np.linspace(-87.0, 87.0, 60), rng.uniform(-20.0, 20.0, 20), [1e-3, -1e-3, 1e-20, -1e-20, 0.5, -0.5]]).astype(np.float32)
    low = np.array([-88.9, -100.0, -1e4, -3e38], dtype=np.float32)
    high = np.array([88.9, 100.0, 1e4, 3e38], dtype=np.float32)
    v = np.concatenate([mid, low, high, [np.nan, 0.0]]).astype(np.float32)
    assert same_bits(feed(run, v[:-2]), np.broadcast_to(v[:-2], (5, v.size - 2))), "the pre-activation is not the impulse product"
    got = feed(run, v, silu=True)
    i0, i1, i2 = mid.size, mid.size + low.size, mid.size + low.size + high.size
    truth = LC.silu64(mid.astype(np.float64))
    rel = np.abs(got[:, :i0] - truth) / np.abs(truth)
    print(f"LINPREC {run.name} silu |v| <= 87: relative error {float(rel.max()) / LC.U:.2f} x 2^-24")
    assert float(rel.max()) <= 4 * LC.U
    assert bool((np.abs(got[:, i0:i1]) < 2.0 ** -126).all()) and not bool((got[:, i0:i1] > 0).any())
    print(f"LINPREC {run.name} silu v < -88.8: {got[0, i0:i1].tolist()}")
    assert same_bits(got[:, i1:i2], np.broadcast_to(high, (5, high.size)))
    assert np.isnan(got[:, i2]).all() and bool((got[:, i2 + 1] == 0).all())


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_epilogue_order(run):
    """bias, then accumulate, then SiLU: the pre-activation is float32(float32(p + bias) + c0) bitwise -- values at which the
    other order rounds differently --, and SiLU is taken of that"""
    rng = np.random.default_rng(11)
    n = 70
    p = rng.standard_normal(n).astype(np.float32)
    bias = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 4, n)).astype(np.float32)
    c0 = (rng.standard_normal((5, n)) * 2.0 ** rng.integers(-20, 4, (5, n))).astype(np.float32)
    pre = (p + bias)[None, :] + c0
    assert pre.dtype == np.float32 and int((bits(pre) != bits(p[None, :] + (bias[None, :] + c0))).sum()) > 0
    assert same_bits(feed(run, p, bias, c0), pre)
    assert same_bits(feed(run, p, bias), np.broadcast_to(p + bias, (5, n)))
    got = feed(run, p, bias, c0, silu=True)
    truth = LC.silu64(pre.astype(np.float64))
    rel = np.abs(got - truth) / np.abs(truth)
    print(f"LINPREC {run.name} bias + accumulate + silu: relative error {float(rel.max()) / LC.U:.2f} x 2^-24 of silu(float32 pre-activation)")
    assert float(rel.max()) <= 4 * LC.U


# ---- containment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run,shape,mode", abi.arms(abi.Simt, abi.Gpu, [((33, 48, 72), (0, 0)), ((33, 48, 72), (1, 1)), ((70, 33, 1024), (0, 0)),
                                                                      ((5, 70, 528), (0, 1))]))
def test_nonfinite_stays_in_its_row_and_column(run, shape, mode):
    m, n, k = shape
    ta, tw = mode
    c = LC.case("benign", m, n, k, 0, True)
    clean = launch(run, c.a, c.w, c.bias, trans_a=ta, trans_w=tw)
    for m0, k0 in ((0, 0), (m - 1, k - 1), (m // 2, k // 2 + 1)):
        a = c.a.copy()
        a[m0, k0] = np.nan
        got = launch(run, a, c.w, c.bias, trans_a=ta, trans_w=tw)
        assert np.isnan(got[m0]).all()
        assert same_bits(np.delete(got, m0, axis=0), np.delete(clean, m0, axis=0))
    for n0, k0 in ((0, k - 1), (n - 1, 0), (n // 2, k // 4)):
        w = c.w.copy()
        w[n0, k0] = np.inf
        got = launch(run, c.a, w, c.bias, trans_a=ta, trans_w=tw)
        assert not np.isfinite(got[:, n0]).any()
        assert same_bits(np.delete(got, n0, axis=1), np.delete(clean, n0, axis=1))


@pytest.mark.parametrize("run,m,n,k", abi.arms(abi.Simt, abi.Gpu, [(33, 5, 72), (5, 33, 1000), (48, 33, 1020), (1, 1, 5)], tag=abi.joined_by_x))
def test_nan_beyond_a_k_tail_is_never_read(run, m, n, k):
    """K-contiguous: the floats behind K of every row; transposed: the row behind K and the floats behind every row.  All NaN, the
    result finite and bitwise the call on zero-padded copies"""
    c = LC.case("benign", m, n, k, 0)
    zp = lambda x: np.pad(x, ((0, 0), (0, LC.pad16(k) - k)))
    want = launch(run, zp(c.a), zp(c.w))
    assert np.isfinite(want).all()
    for ta, tw in MODES:
        assert same_bits(launch(run, c.a, c.w, trans_a=ta, trans_w=tw, pad=(5, 7, 3)), want), (ta, tw)
        assert same_bits(launch(run, c.a, c.w, trans_a=ta, trans_w=tw, pad=(4, 8, 0)), want), (ta, tw)


@pytest.mark.parametrize("run,k", abi.arms(abi.Simt, abi.Gpu, [48, 576, 1000]))
def test_accumulate_onto_c_far_above_and_far_below_the_product(run, k):
    m, n = SHAPE_OF_K[k]
    base = LC.case("benign", m, n, k, 0)
    for name, scale in (("1e6", 1e6), ("2^-20", 2.0 ** -20)):
        c = LC.Case(base.a, base.w, None, (base.truth * scale).astype(np.float32), base.a_kinds, base.w_kinds)
        check_case(run, f"benign c0={name}xproduct {m}x{n}", c, launch(run, c.a, c.w, None, c.c0), k)


# ---- operands that do not begin on a 16-byte boundary ----------------------------------------------------------------------------------
@pytest.mark.parametrize("run,m,n,k", abi.arms(abi.Simt, abi.Gpu, [(5, 7, 32), (33, 48, 512), (70, 33, 48)], tag=abi.joined_by_x))
def test_unaligned_operands(run, m, n, k):
    """K % 16 == 0, lda % 4 == 0, A / W 1 .. 3 floats past a 16-byte boundary: a legal call (any 4-byte-aligned pointer), which
    the host must keep off the 16-byte-load instance.  Bitwise the aligned call."""
    c = LC.case("scales", m, n, k, 0, True)
    want = launch(run, c.a, c.w, c.bias)
    check_case(run, f"scales+bias {m}x{n} aligned", c, want, k)
    for off in [(o, 0) for o in (1, 2, 3)] + [(0, o) for o in (1, 2, 3)] + [(1, 1), (2, 3), (3, 2)]:
        assert same_bits(launch(run, c.a, c.w, c.bias, offset=off), want), off
