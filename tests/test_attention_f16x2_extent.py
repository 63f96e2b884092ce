"""dmd_attention_f16x2 (attention_f16x2_kernel<true>: the split-fp16 two-pass kernel over the valid tokens of any extent) and the
route to it (engine.attention in default precision, ATTN_F16X2_EXTENT_MIN_T / DIAMOND_ATTN_F16X2_MIN_T), on the SIMT interpreter
(the kernel's own source, arrays fenced: an out-of-bounds access fails there; a wave that missed a barrier is a diagnosed deadlock)
and on the device (-m gpu).  `out` starts as NaN in every test; the margins of every extent hold NaN and +-Inf.

Against float64 of the CROPPED tensors, per (image, head), every head at its own V scale (attention_cases.Ref):
    err <= K_SPLIT x max(err_fp32, 2^-24)
K_SPLIT is attention_cases' constant for the on-grid kernel, imported: the arithmetic per (query, key) pair is the same,
a masked key adds exactly 0.  profiles/attention_f16x2_extent_precision.txt has the measured ratios of every case below
(`python tools/attention_fwd_bench.py --f16x2-precision` writes it).

Shapes (H, W, vh, vw); valid tokens: 1 (one query, one key: 255 masked keys, three waves without a query); 255 / 257 (one key
short of a tile / one key into the second: a second workgroup with ONE valid query); 576 (24 x 24 whole grid, T % 256 != 0: two
whole tiles and a quarter); 360 (18 x 20 of 32 x 32); 323 (17 x 19 of 32 x 32: odd row width, the second workgroup has 67 valid
queries, two of its waves none); 1296 (36 x 36 of 64 x 64, device only).  The interpreter arm runs N = 2, C = 16, the device arm
N = 2, C = 24 (three heads: a wrong head stride shows)."""
import functools
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

from tests import abi
from tests import attention_cases as P

K = P.K_SPLIT
N = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXTENTS = [(1, 1, 1, 1), (1, 255, 1, 255), (1, 257, 1, 257), (24, 24, 24, 24), (32, 32, 18, 20), (32, 32, 17, 19)]
GPU_ONLY_EXTENTS = [(64, 64, 36, 36)]
PARTIAL = (32, 32, 18, 20)  # 360 tokens: a whole tile and a partial one
ODD = (32, 32, 17, 19)      # 323 tokens


# ---- the two arms ------------------------------------------------------------------------------------------------------------------
def _arm(name, run, c):
    """`run` is dmd_attention_f16x2 on an extent (status=True: (rc, out) without raising), `attention` its flat call (N, T, 3C) ->
    (N, T, C), the shape attention_cases' helpers expect of an arm; `other` is dmd_attention on the same runner.  Tensors"""
    def launch(qkv, h, w, vh, vw, c, **kw):
        got = abi.attention(run, qkv, c, "dmd_attention_f16x2", (h, w, vh, vw), **kw)
        return (got[0], torch.from_numpy(got[2])) if kw.get("status") else torch.from_numpy(got)

    return SimpleNamespace(name=name, run=launch, c=c, attention=lambda qkv, c: launch(qkv, 1, qkv.shape[1], 1, qkv.shape[1], c),
                           other=lambda qkv, c: torch.from_numpy(abi.attention_default(run, qkv, c)))


SIMT = _arm("simt-f16x2-extent", abi.Simt, 16)
GPU = _arm("gpu-f16x2-extent", abi.Gpu, 24)
BOTH = abi.arms(SIMT, GPU)


both = functools.partial(abi.arms, SIMT, GPU)  # both(cases): (arm, *case) on the two arms


# ---- extents -----------------------------------------------------------------------------------------------------------------------
def embed(flat, extent, fill="nonfinite"):
    """the tokens of `flat` (N, vh vw, X) as the (vh, vw) extent of an (H, W) grid whose margins hold NaN / +Inf / -Inf by channel
    ("nonfinite") or 1e5 / -3e38 / 0 ("finite")"""
    h, w, vh, vw = extent
    n, tv, x = flat.shape
    assert tv == vh * vw
    ch = torch.arange(x) % 3
    a, b, c = (math.nan, math.inf, -math.inf) if fill == "nonfinite" else (1.0e5, -3.0e38, 0.0)
    grid = torch.where(ch == 0, a, torch.where(ch == 1, b, c)).float().expand(n, h, w, x).clone()
    grid[:, :vh, :vw] = flat.reshape(n, vh, vw, x)
    return grid


def crop(out, extent):
    _, _, vh, vw = extent
    return out[:, :vh, :vw].reshape(out.shape[0], vh * vw, out.shape[-1])


def margin(out, extent):
    h, w, vh, vw = extent
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[:vh, :vw] = True
    return out[:, ~inside]


def on_extent(arm, flat, extent, c, fill="nonfinite"):
    """the flat tokens through the kernel as `extent`: the cropped output; the margin rows of `out` have to be +0"""
    out = arm.run(embed(flat, extent, fill), *extent, c)
    m = margin(out, extent)
    assert bool((m == 0).all()) and not bool(torch.signbit(m).any()), "out outside the valid extent is not +0"
    return crop(out, extent)


ratios = P.ratios


def check_bound(family, arm, ref, got, what=""):
    """print the figures of the worst (image, head), then assert the bound on every (image, head)"""
    n, t, _ = ref.qkv.shape
    return P.check_bound(f"ATTF16X {arm.name} family={family}{what} tv={t} N={n} C={ref.c}", ref, got, K)[1]


SCALES = (1.5, 4.0, 8.0, 16.0)


def family_cases(t, c):
    """(label, Ref) of the finite-input families that take the ordinary bound, at one (tv, C)"""
    for a in SCALES:
        yield f"1 a={a}", P.family_scale(N, c, t, a)
    yield "2 offset", P.family_offset(N, c, t)
    yield "3 moving max", P.family_moving_max(N, c, t)
    yield "4 one-hot / uniform", P.family_onehot_uniform(N, c, t)
    yield "5 v", P.family_range(N, c, t, "v")
    yield "5 kv", P.family_range(N, c, t, "kv")
    yield "7 v*1e-7*2^23", P.family_floor(N, c, t, 2.0 ** 23)


def tokens(extent):
    return extent[2] * extent[3]


@pytest.mark.parametrize("arm,extent", both([(e,) for e in EXTENTS + GPU_ONLY_EXTENTS], simt_if=lambda e: e not in GPU_ONLY_EXTENTS))
def test_extent_vs_fp64_of_the_cropped_tensors_with_non_finite_margins(arm, extent):
    ref = P.family_scale(N, arm.c, tokens(extent), 1.5)
    assert not bool(torch.isfinite(margin(embed(ref.qkv, extent), extent)).any())
    check_bound("extent", arm, ref, on_extent(arm, ref.qkv, extent, arm.c), what=" " + "x".join(map(str, extent)))


# ---- the families on an extent with a partial last tile -----------------------------------------------------------------------------
@pytest.mark.parametrize("arm,a", both(SCALES))
def test_score_magnitude(arm, a):
    """Family 1: q, k ~ a N(0, 1): scores up to +-700 at a = 16"""
    ref = P.family_scale(N, arm.c, tokens(PARTIAL), a)
    check_bound(1, arm, ref, on_extent(arm, ref.qkv, PARTIAL, arm.c), what=f" a={a}")


@pytest.mark.parametrize("arm", BOTH)
def test_common_offset(arm):
    """Family 2: the subtraction of the row maximum under scores of +-204 +- O(5)"""
    ref = P.family_offset(N, arm.c, tokens(PARTIAL))
    check_bound(2, arm, ref, on_extent(arm, ref.qkv, PARTIAL, arm.c))


@pytest.mark.parametrize("arm", BOTH)
def test_maximum_moving_with_the_key_index(arm):
    """Family 3: the row maximum rises at every block and tile for half of the rows, into the masked tile; winners exactly at keys
    0, 255, 256 and tv - 1 (the last unmasked key)"""
    ref = P.family_moving_max(N, arm.c, tokens(PARTIAL))
    check_bound(3, arm, ref, on_extent(arm, ref.qkv, PARTIAL, arm.c))


@pytest.mark.parametrize("arm", BOTH)
def test_onehot_and_uniform_rows(arm):
    """Family 4: a one-hot row returns its key's v row; a q = 0 row the mean of V over the VALID keys (a masked key that kept a
    weight, or a valid one that lost it, shows here at once)"""
    ref = P.family_onehot_uniform(N, arm.c, tokens(PARTIAL))
    got = on_extent(arm, ref.qkv, PARTIAL, arm.c)
    check_bound(4, arm, ref, got)
    v = ref.qkv[..., 2 * arm.c:].double()
    lim = ref.per_element(ref.limit(K))
    assert bool(((got[:, ref.hot].double() - v[:, ref.tgt]).abs() <= lim[:, ref.hot]).all()), "a one-hot row is not its key's v"
    mean = v.mean(dim=1, keepdim=True)
    assert bool(((got[:, ref.hot + 1].double() - mean).abs() <= lim[:, ref.hot + 1]).all()), "a q = 0 row is not the mean of V"


@pytest.mark.parametrize("arm,which", both(["v", "kv"]))
def test_operands_up_to_the_end_of_fp16(arm, which):
    """Family 5: v ("v"), and k too ("kv"), reaching +-65504; "kv" has q ~ 2e-4: both workgroups rebalance"""
    ref = P.family_range(N, arm.c, tokens(PARTIAL), which)
    check_bound(5, arm, ref, on_extent(arm, ref.qkv, PARTIAL, arm.c), what=f" {which}")


@pytest.mark.parametrize("arm", BOTH)
def test_absolute_floor(arm):
    """Family 7, as test_attention_precision holds the on-grid kernel to it: v * 1e-7 is off by at most 2^-24 + 1e-5 |truth|
    (the fp16 pieces stop at 2^-25), the same tensor times 2^23 is within the ordinary bound"""
    t = tokens(PARTIAL)
    ref = P.family_floor(N, arm.c, t, 1.0)
    got = on_extent(arm, ref.qkv, PARTIAL, arm.c)
    err = (got.double() - ref.truth).abs()
    print(f"ATTF16X {arm.name} family=7 v*1e-7 tv={t}: largest |got - truth| {float(err.max()):.3e} = {float(err.max()) * 2.0 ** 25:.2f} x 2^-25")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= 2.0 ** -24 + 1.0e-5 * ref.truth.abs()).all()), float(err.max())
    up = P.family_floor(N, arm.c, t, 2.0 ** 23)
    check_bound(7, arm, up, on_extent(arm, up.qkv, PARTIAL, arm.c), what=" v*1e-7*2^23")


@pytest.mark.parametrize("arm", BOTH)
def test_rebalanced_and_plain_workgroups_over_the_same_keys(arm):
    """Family 5b at tv = 323: valid queries 0 .. 255 are tiny (their workgroup rebalances), the 67 of the second workgroup are
    plain (it does not; its 189 absent queries are zeros and stay out of its qmax), over the same keys"""
    ref = P.family_mixed_workgroups(N, arm.c, tokens(ODD))
    check_bound("5b", arm, ref, on_extent(arm, ref.qkv, ODD, arm.c))


@pytest.mark.parametrize("arm", BOTH)
def test_absent_queries_stay_out_of_the_rebalancing(arm):
    """tv = 323 with EVERY valid query tiny against keys near the end of fp16 (family 5 "kv"): the second workgroup has to
    rebalance by its 67 valid queries; garbage taken for a query there (the margins hold Inf and, in the other fill, 1e5) would
    switch it off and cost the relative error (ratios of 500 .. 1300 without rebalancing)"""
    ref = P.family_range(N, arm.c, tokens(ODD), "kv")
    for fill in ("nonfinite", "finite"):
        check_bound(5, arm, ref, on_extent(arm, ref.qkv, ODD, arm.c, fill), what=f" kv, margins {fill}")


# ---- bitwise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm,t", both([256, 512]))
def test_whole_tile_grids_are_bitwise_dmd_attention(arm, t):
    """the extent (1, T, 1, T) with T % 256 == 0 runs the on-grid inner loops on the same operands"""
    qkv = P.family_scale(N, arm.c, t, 4.0).qkv
    got = arm.attention(qkv, arm.c)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, arm.other(qkv, arm.c))


@pytest.mark.parametrize("arm,extent", both([(PARTIAL,), (ODD,), ((24, 24, 24, 24),)]))
def test_an_extent_is_bitwise_the_flat_call_on_the_compacted_tokens(arm, extent):
    """(H, W, vh, vw) == (1, tv, 1, tv) on the compacted tokens; with the whole grid, (H, W, H, W) == (1, H W, 1, H W)"""
    qkv = P.family_scale(N, arm.c, tokens(extent), 4.0).qkv
    flat = arm.attention(qkv, arm.c)
    assert bool(torch.isfinite(flat).all()) and torch.equal(on_extent(arm, qkv, extent, arm.c), flat)


@pytest.mark.parametrize("arm", BOTH)
def test_two_launches_and_two_margin_fills_are_bitwise_equal(arm):
    """nothing outside the extent is read: NaN / +-Inf in the margins and 1e5 / -3e38 / 0 there give the same bits, as do two
    launches"""
    qkv = P.family_scale(N, arm.c, tokens(ODD), 4.0).qkv
    first = on_extent(arm, qkv, ODD, arm.c)
    assert bool(torch.isfinite(first).all())
    assert torch.equal(first, on_extent(arm, qkv, ODD, arm.c))
    assert torch.equal(first, on_extent(arm, qkv, ODD, arm.c, fill="finite"))


@pytest.mark.parametrize("arm", BOTH)
def test_an_image_and_a_head_do_not_depend_on_the_others(arm):
    """N = 1 is bitwise the slice of N = 3, and one head alone (C = 8) bitwise its slice of the C-channel call"""
    t, c = tokens(ODD), arm.c
    qkv = P.family_scale(3, c, t, 4.0).qkv
    full = on_extent(arm, qkv, ODD, c)
    assert bool(torch.isfinite(full).all())
    for i in range(3):
        assert torch.equal(on_extent(arm, qkv[i:i + 1].contiguous(), ODD, c), full[i:i + 1]), i
    hd = c // 8 - 1
    one = torch.cat([qkv[..., s * c + 8 * hd:s * c + 8 * hd + 8] for s in range(3)], dim=-1).contiguous()
    assert torch.equal(on_extent(arm, one, ODD, 8), full[..., 8 * hd:8 * hd + 8])


# ---- beyond the range, non-finite, inside the extent -------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", BOTH)
def test_a_finite_value_beyond_fp16_is_loud_and_confined(arm):
    """Family 6a on the 18 x 20 extent: 1.0e5 in one v, one k (token tv - 2: the masked tile) and one q element of three
    (image, head) pairs: every output they feed is non-finite or within the bound, never finite and wrong; everything else is
    bitwise the run without them"""
    t, c = tokens(PARTIAL), arm.c
    where = P.sites(N, c, t)
    qkv = P.family_scale(N, c, t, 1.5).qkv
    for operand, site in where.items():
        qkv = P.plant(qkv, c, site, operand, 1.0e5)
    ref = P.Ref(qkv, c)
    got = on_extent(arm, qkv, PARTIAL, c)
    touched = P.check_confined(arm, t, N, c, got, where)
    lim = ref.per_element(ref.limit(K))
    wrong = torch.isfinite(got) & ~((got.double() - ref.truth).abs() <= lim)
    assert not bool(wrong.any()), f"{int(wrong.sum())} outputs are finite and wrong"
    assert bool(torch.isfinite(got[~touched]).all()) and not bool(torch.isfinite(got[touched]).all())


@pytest.mark.parametrize("arm,operand", both(["q", "k", "v"]))
def test_non_finite_operands_behave_as_in_float32(arm, operand):
    """Family 6b on the 18 x 20 extent: NaN, +Inf, -Inf in one element of q, k or v: finite exactly where the float32 CPU
    evaluation of the cropped tensors is, the finite part within the bound, everything outside the planted head / row / dim
    bitwise unchanged.  (An infinite q against the ZERO rows staged for the masked keys is 0 x Inf: the selection of -inf keeps it
    out of the row, or every such row would be NaN where float32 has numbers.)"""
    t, c = tokens(PARTIAL), arm.c
    failures = []
    site = P.sites(N, c, t)[operand]
    for value in (math.nan, math.inf, -math.inf):
        ref = P.Ref(P.plant(P.family_scale(N, c, t, 1.5).qkv, c, site, operand, value), c)
        got = on_extent(arm, ref.qkv, PARTIAL, c)
        P.check_confined(arm, t, N, c, got, {operand: site})
        fin, fin32 = torch.isfinite(got), torch.isfinite(ref.y32)
        both_ = fin & fin32 & torch.isfinite(ref.truth)
        err = torch.where(both_, (got.double() - ref.truth).abs(), torch.zeros_like(ref.truth))
        over = err > ref.per_element(ref.limit(K))
        print(f"ATTF16X {arm.name} family=6b {operand}={value} tv={t}: finite {int(fin.sum())} (float32: {int(fin32.sum())}), "
              f"{int((fin != fin32).sum())} differ, {int(over.sum())} finite outputs over the bound")
        if bool((fin != fin32).any()):
            failures.append(f"{operand}={value}: {int((fin & ~fin32).sum())} finite where float32 is not, "
                            f"{int((~fin & fin32).sum())} non-finite where float32 is finite")
        if bool(over.any()):
            failures.append(f"{operand}={value}: {int(over.sum())} finite outputs over the bound")
    assert not failures, failures


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", BOTH)
def test_rejects_an_extent_outside_the_grid_and_another_head_dim(arm):
    """a nonzero status and no launch: `out` keeps its NaN"""
    qkv = embed(P.family_scale(N, arm.c, 81, 1.5).qkv, (16, 16, 9, 9))
    for vh, vw in ((17, 9), (9, 17), (0, 9), (9, 0)):
        with pytest.raises(RuntimeError, match="valid extent"):
            arm.run(qkv, 16, 16, vh, vw, arm.c)
        rc, out = arm.run(qkv, 16, 16, vh, vw, arm.c, status=True)
        assert rc != 0 and bool(torch.isnan(out).all())
    rc, out = arm.run(qkv, 16, 16, 9, 9, arm.c, head_dim=4, status=True)
    assert rc != 0 and bool(torch.isnan(out).all())
    with pytest.raises(RuntimeError, match="head_dim"):
        arm.run(qkv, 16, 16, 9, 9, arm.c, head_dim=16)


# ---- the threshold -----------------------------------------------------------------------------------------------------------------
def test_default_threshold_follows_from_the_recorded_table():
    """profiles/attention_f16x2_extent.json: "derived_threshold" is the smallest measured token count from which dmd_attention_f16x2
    beats attention_kernel (what these shapes ran before) at every measured shape by more than the block-to-block spread, and the
    table holds every shape the rule was to be read from.  engine.ATTN_F16X2_EXTENT_MIN_T is that number -- unless it is at or
    below the 360 valid tokens (18 x 20) of the 68 x 76 training step's upper attention level, whose launches
    tests/test_offgrid_train.py pins to dmd_attention_valid: then it is the smallest measured count above 360 (the table gives
    256, the default is 576)."""
    from diamond_amd import engine as E

    with open(os.path.join(ROOT, "profiles", "attention_f16x2_extent.json")) as f:
        table = json.load(f)
    shapes = table["shapes"]
    have = {(s["H"], s["W"], s["valid"][0], s["valid"][1]) for s in shapes}
    assert have >= {(32, 32, 18, 20), (32, 32, 17, 19), (64, 64, 36, 36), (1, 320, 1, 320), (1, 576, 1, 576), (1, 256, 1, 256),
                    (1, 1024, 1, 1024), (1, 4096, 1, 4096)}, have
    for s in shapes:
        med, spread = s["median_us"], s["block_spread_us"]
        assert s["faster_by_more_than_the_spread"] == (med["attention_kernel"] - med["f16x2_extent"]
                                                       > max(spread["attention_kernel"], spread["f16x2_extent"])), s
    counts = sorted({s["valid_tokens"] for s in shapes})
    wins = [t for t in counts if all(s["faster_by_more_than_the_spread"] for s in shapes if s["valid_tokens"] >= t)]
    assert wins and table["derived_threshold"] == wins[0], "the record is stale"
    pinned = 360
    assert table["pinned_old_route_tokens"] == pinned
    default = min(t for t in counts if t >= wins[0] and t > pinned)
    assert table["default_threshold"] == E.ATTN_F16X2_EXTENT_MIN_T == default, (wins[0], default, E.ATTN_F16X2_EXTENT_MIN_T)
    assert E.ATTN_F16X2_EXTENT_MIN_T >= counts[0], "nothing below the smallest measured count is routed"
    on_grid = [s for s in shapes if s["H"] == 1 and s["valid_tokens"] in (1024, 4096)]
    assert len(on_grid) == 2 and all(s["on_grid_within_the_spread_of_dmd_attention"] and s["bitwise_dmd_attention"] for s in on_grid)


# ---- routing on the interpreter ----------------------------------------------------------------------------------------------------
def test_routing_switch_on_the_interpreter(monkeypatch):
    """the two-level 16 x 16 network of test_attention_f32_tiled's routing test (attention over the whole 8 x 8 grid: 64 tokens,
    T % 256 != 0): DIAMOND_ATTN_F16X2_MIN_T=64 sends every attention forward to attention_f16x2_kernel through dmd_attention_f16x2,
    in inference and in a training step (whose backward count matches); =0 and unset give attention_kernel and a direct
    dmd_attention call's bits; DIAMOND_ATTN_PRECISION=f32 goes before it"""
    from diamond_amd import engine as E
    from diamond_amd import native as nv
    from tests.simt.host_harness import engine_on_interpreter

    assert E.ATTN_F16X2_EXTENT_MIN_T == 0 or E.ATTN_F16X2_EXTENT_MIN_T > 64
    den, batch, noisy, obs = P.two_level_denoiser()
    act = batch.act

    seen, names = [], []
    attention = E.attention

    def spy(qkv, c, head_dim=8, precision=None):
        out = attention(qkv, c, head_dim, precision)
        seen.append((qkv.t.clone(), out.clone(), c))
        return out

    monkeypatch.setattr(E, "attention", spy)
    variables = ("DIAMOND_ATTN_PRECISION", "DIAMOND_ATTN_F32_MIN_T", "DIAMOND_ATTN_F16X2_MIN_T", "DIAMOND_ATTN_BWD_MIN_T")

    class Counter(P.LaunchCounter):
        def call(self, name, fn, args):
            names.append(name)
            return super().call(name, fn, args)

    def forward(env):
        for k in variables:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        counter = Counter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        del seen[:], names[:]
        out = den.compute_model_output(noisy, obs, act[:, :4], 1.3)
        return out, {k: v for k, v in counter.n.items() if k in P.FORWARD_KEYS + ("dmd_attention_f16x2",)}, list(seen), set(names)

    with engine_on_interpreter():
        o_def, n_def, s_def, _ = forward({})
        o_new, n_new, s_new, c_new = forward({"DIAMOND_ATTN_F16X2_MIN_T": "64"})
        o_off, n_off, _, c_off = forward({"DIAMOND_ATTN_F16X2_MIN_T": "0"})
        o_far, n_far, _, _ = forward({"DIAMOND_ATTN_F16X2_MIN_T": "65"})
        o_f32, n_f32, _, c_f32 = forward({"DIAMOND_ATTN_F16X2_MIN_T": "64", "DIAMOND_ATTN_PRECISION": "f32"})
        o_x, n_x, _, _ = forward({"DIAMOND_ATTN_PRECISION": "f32"})
        attn = len(s_def)
        assert attn >= 1 and n_def == {"attention_kernel": attn}, n_def
        for qkv, out, c in s_def:  # unset: a direct dmd_attention call's bits (64 tokens: attention_kernel)
            assert qkv.shape[1] * qkv.shape[2] == 64
            assert torch.equal(out.reshape(1, 64, c), SIMT.other(qkv.reshape(1, 64, 3 * c), c))
        assert n_off == n_def and torch.equal(o_off, o_def) and "dmd_attention_f16x2" not in c_off
        assert n_far == n_def and torch.equal(o_far, o_def), "65 > 64 tokens"
        assert n_new == {"attention_f16x2_kernel": attn} and "dmd_attention_f16x2" in c_new and "dmd_attention" not in c_new, (n_new, c_new)
        for qkv, out, c in s_new:  # the new route: a direct dmd_attention_f16x2 call's bits
            assert torch.equal(out.reshape(1, 64, c), SIMT.attention(qkv.reshape(1, 64, 3 * c), c))
        assert n_f32 == n_x == {"attention_kernel": attn} and torch.equal(o_f32, o_x) and "dmd_attention_f16x2" not in c_f32, n_f32
        assert bool(torch.isfinite(o_new).all()) and not torch.equal(o_new, o_def), "the switch changed nothing"
        assert float((o_new - o_def).abs().max()) <= 1e-4 * float(o_def.abs().max())

        # the training step: the recorded forward takes the switch, the backward differentiates around its y
        den.train()
        for k in variables:
            monkeypatch.delenv(k, raising=False)
        steps = {}
        for value in ("64", "0"):
            monkeypatch.setenv("DIAMOND_ATTN_F16X2_MIN_T", value)
            counter = Counter()
            monkeypatch.setattr(nv, "PROFILER", counter)
            steps[value] = (P.training_step(den, batch), dict(counter.n))
        (loss, grads), n_step = steps["64"]
        (loss0, grads0), n_step0 = steps["0"]
        fwd = {k: v for k, v in n_step.items() if k in P.FORWARD_KEYS}
        assert set(fwd) == {"attention_f16x2_kernel"} and n_step.get("dmd_attention_bwd", 0) == fwd["attention_f16x2_kernel"], n_step
        assert {k: v for k, v in n_step0.items() if k in P.FORWARD_KEYS} == {"attention_kernel": fwd["attention_f16x2_kernel"]}, n_step0
        assert n_step0.get("dmd_attention_bwd", 0) == n_step["dmd_attention_bwd"]
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in grads.values())
        P.assert_training_parity(grads, grads0)
        assert any(not torch.equal(grads[k], grads0[k]) for k in grads0), "the switch changed nothing"


# ---- device model level ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_golden_training_step_68x76_with_the_new_route(monkeypatch):
    """the committed attn0011 68 x 76 fixture (360 valid tokens at the upper attention level, 90 at the lower) with the threshold
    forced to 256: the 1e-4 bar of tests/test_offgrid_train.py on the loss and every gradient, in both conv precisions"""
    from diamond_amd import native as nv
    from tests import test_offgrid_train as OT

    monkeypatch.setenv("DIAMOND_ATTN_F16X2_MIN_T", "256")
    monkeypatch.delenv("DIAMOND_ATTN_PRECISION", raising=False)
    counter = P.LaunchCounter()
    monkeypatch.setattr(nv, "PROFILER", counter)
    OT.check_denoiser_training_step("denoiser_train_attn0011_68x76.pt")
    assert counter.n.get("attention_f16x2_kernel", 0) >= 2, counter.n


@pytest.mark.gpu
def test_model_output_72x72_is_within_parity_of_the_old_route(monkeypatch):
    """attention at the 36 x 36 (1296 tokens) and 18 x 18 (324) levels of a 72 x 72 image, both valid extents of padded grids:
    other bits than attention_kernel's, within the project's parity bar of 1e-4 of max |output|"""
    from diamond_amd import native as nv
    from tests import test_offgrid_train as OT

    monkeypatch.delenv("DIAMOND_ATTN_PRECISION", raising=False)
    den = OT.make_agent(attn_depths=(0, 1, 1, 0)).denoiser
    g = torch.Generator().manual_seed(5)
    noisy, obs = torch.randn(2, 3, 72, 72, generator=g).cuda(), torch.randn(2, 12, 72, 72, generator=g).clamp(-1, 1).cuda()
    act = torch.randint(0, 4, (2, 4), generator=g).cuda()
    got = {}
    for value in ("256", "0"):
        monkeypatch.setenv("DIAMOND_ATTN_F16X2_MIN_T", value)
        counter = P.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        got[value] = (den.compute_model_output(noisy, obs, act, 1.3), counter.n)
    (o_new, n_new), (o_old, n_old) = got["256"], got["0"]
    assert n_new.get("attention_f16x2_kernel", 0) >= 2 and "attention_f16x2_kernel" not in n_old, (n_new, n_old)
    diff = float((o_new - o_old).abs().max() / o_old.abs().max())
    print(f"ATTF16X model output 72x72, the new route against attention_kernel: {diff:.3e} of max |output|")
    assert bool(torch.isfinite(o_new).all()) and not torch.equal(o_new, o_old)
    assert diff <= 1e-4, diff


@pytest.mark.gpu
def test_graphed_training_step_with_the_new_route_is_bitwise_the_eager_loop(monkeypatch):
    """tests/test_offgrid_train.py's graphed 72 x 72 step with attention at the 18 x 18 level (324 valid tokens) and the threshold
    forced to 256: the launch records into the hipGraph like the others (no allocation, no synchronisation, the variable read at
    capture) and replays the eager loop bit for bit"""
    from diamond_amd import native as nv
    from tests import test_offgrid_train as OT

    monkeypatch.setenv("DIAMOND_ATTN_F16X2_MIN_T", "256")
    monkeypatch.delenv("DIAMOND_ATTN_PRECISION", raising=False)
    make_agent = OT.make_agent
    monkeypatch.setattr(OT, "make_agent", lambda: make_agent(attn_depths=(0, 0, 1, 0)))
    counter = P.LaunchCounter()
    monkeypatch.setattr(nv, "PROFILER", counter)
    OT.test_graphed_training_step_72x72_is_bitwise_the_eager_loop()
    assert counter.n.get("attention_f16x2_kernel", 0) >= 1, counter.n

