"""dmd_attention_f32 (attention_f32_tiled_kernel: exact fp32 operands on the fp32 matrix cores, two passes over the keys, tokens
addressed by their valid index) and the switch that routes to it (engine.attention's `precision`, DIAMOND_ATTN_PRECISION,
`attn_precision` on the denoiser's inference and training paths), on the SIMT interpreter (the kernel's own source, arrays fenced:
an out-of-bounds access fails there) and on the device (-m gpu).  `out` starts as NaN in every test.

Against float64, per (image, head), every head at its own V scale (attention_cases.Ref / head_errors):
    err <= K_TILED x max(err_fp32, 2^-24)
K_TILED = twice the largest ratio measured on the MI355X over every case of this file (profiles/attention_f32_tiled_precision.txt
has the table; `python tools/attention_fwd_bench.py --precision` writes it and applies this rule): 2 x 4.7732 rounded up (scaled family, a = 16, T = 320, C = 24,
where attention_kernel has 5.58 on the same inputs; typical 1.0 .. 2.3: the ratio is one of two maxima over a head and scatters,
test_attention_precision.py says how).  It has to stay below K_EXACT = 15.3, attention_kernel's contract: the two-pass exp2 formula evaluated in
float32 on the CPU has a worst ratio of 2.2 over these families, so a kernel that needs more than 15.3 is wrong, not imprecise.

Token counts: 64 one query block, one partial tile; 80 a partial query block and a partial 16-key group; 256 one full tile; 320 a
full plus a partial tile; 512 both staging buffers; 768 / 1024 three / four tiles.  The interpreter arm takes T <= 512 at N = 2,
C = 16, the device arm every T at C = 24 (three heads: a wrong head stride shows) plus C = 64 at T = 1280."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from tests import abi
from tests import attention_cases as P

K_TILED = 9.55  # 2 x 4.7732, rounded up to two decimals (tools/attention_fwd_bench.py k_tiled)
assert K_TILED <= P.K_EXACT

TS = (64, 80, 256, 320, 512, 768, 1024)
N = 2


# ---- the two arms ------------------------------------------------------------------------------------------------------------------
def _arm(name, run, c, entry="dmd_attention_f32"):
    """`run` is the entry point on an extent, `attention` its flat call (N, T, 3C) -> (N, T, C), the shape attention_cases' helpers
    expect of an arm; `other` is dmd_attention (exact=True: attention_kernel) on the same runner.  All return tensors"""
    launch = lambda qkv, h, w, vh, vw, c, **kw: torch.from_numpy(abi.attention(run, qkv, c, entry, (h, w, vh, vw), **kw))
    return SimpleNamespace(name=name, run=launch, c=c, attention=lambda qkv, c: launch(qkv, 1, qkv.shape[1], 1, qkv.shape[1], c),
                           other=lambda qkv, c, exact=False: torch.from_numpy(abi.attention_default(run, qkv, c, exact)))


SIMT = _arm("simt-f32", abi.Simt, 16)
GPU = _arm("gpu-f32", abi.Gpu, 24)
BOTH = abi.arms(SIMT, GPU)


def arms(*more, ts=TS, wide=True):
    """(arm, t, c, *extra) cases: the interpreter arm gets T <= 512 only, the device arm every T and (wide) C = 64 at T = 1280"""
    extras = [()] if not more else [e if isinstance(e, tuple) else (e,) for e in more]
    cases = [(t, c) + e for t, c in [(t, None) for t in ts] + ([(1280, 64)] if wide else []) for e in extras]
    return abi.arms(SIMT, GPU, cases, simt_if=lambda t, c, *e: c is None and t <= 512,
                    tag=lambda t, c, *e: "-".join([str(t)] + ([f"c{c}"] if c else []) + [str(x) for x in e]),
                    values=lambda arm, t, c, *e: (t, c or arm.c) + e)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
ratios = P.ratios


def check_bound(family, arm, ref, got, what=""):
    """print the figures of the worst (image, head), then assert the bound on every (image, head)"""
    n, t, _ = ref.qkv.shape
    return P.check_bound(f"ATTF32 {arm.name} family={family}{what} T={t} N={n} C={ref.c}", ref, got, K_TILED)[1]



SCALES = (1.5, 4.0, 8.0, 16.0)


def precision_cases(t, c):
    """(label, Ref) of every finite-input family at one (T, C): what K_TILED is measured over (tools/attention_fwd_bench.py)"""
    for a in SCALES:
        yield f"1 a={a}", P.family_scale(N, c, t, a)
    yield "2 offset", P.family_offset(N, c, t)
    yield "3 moving max", P.family_moving_max(N, c, t)
    yield "4 one-hot / uniform", P.family_onehot_uniform(N, c, t)
    yield "5 v", P.family_range(N, c, t, "v")
    yield "5 kv", P.family_range(N, c, t, "kv")
    yield "7 v*1e-7", P.family_floor(N, c, t, 1.0)


# ---- against float64, full grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm,t,c,a", arms(*SCALES))
def test_score_magnitude(arm, t, c, a):
    """Family 1: q, k ~ a N(0, 1): scores up to +-700 at a = 16"""
    ref = P.family_scale(N, c, t, a)
    check_bound(1, arm, ref, arm.attention(ref.qkv, c), what=f" a={a}")


@pytest.mark.parametrize("arm,t,c", arms())
def test_common_offset(arm, t, c):
    """Family 2: the subtraction of the row maximum under scores of +-204 +- O(5)"""
    ref = P.family_offset(N, c, t)
    check_bound(2, arm, ref, arm.attention(ref.qkv, c))


@pytest.mark.parametrize("arm,t,c", arms())
def test_maximum_moving_with_the_key_index(arm, t, c):
    """Family 3: the row maximum rises at every 16-key block and 256-key tile for half of the rows (pass 1's running maximum across
    blocks, tiles and the four lanes of a query), falls for the other half; winners exactly at keys 0, 255, 256, T - 1"""
    ref = P.family_moving_max(N, c, t)
    check_bound(3, arm, ref, arm.attention(ref.qkv, c))


@pytest.mark.parametrize("arm,t,c", arms())
def test_onehot_and_uniform_rows(arm, t, c):
    """Family 4: a one-hot row returns its key's v row, a q = 0 row the mean of V, side by side in every 16-query group"""
    ref = P.family_onehot_uniform(N, c, t)
    got = arm.attention(ref.qkv, c)
    check_bound(4, arm, ref, got)
    v = ref.qkv[..., 2 * c:].double()
    lim = ref.per_element(ref.limit(K_TILED))
    assert bool(((got[:, ref.hot].double() - v[:, ref.tgt]).abs() <= lim[:, ref.hot]).all()), "a one-hot row is not its key's v"
    mean = v.mean(dim=1, keepdim=True)
    assert bool(((got[:, ref.hot + 1].double() - mean).abs() <= lim[:, ref.hot + 1]).all()), "a q = 0 row is not the mean of V"


@pytest.mark.parametrize("arm,t,c,which", arms("v", "kv"))
def test_operands_up_to_the_end_of_fp16(arm, t, c, which):
    """Family 5: v ("v"), and k too ("kv"), reaching +-65504; "kv" has q ~ 2e-4 against k ~ 2e4 .. 6.5e4 (scores N(0, 4^2)): the
    case the split kernel has to rebalance for is plain arithmetic here"""
    ref = P.family_range(N, c, t, which)
    check_bound(5, arm, ref, arm.attention(ref.qkv, c), what=f" {which}")


@pytest.mark.parametrize("arm,t,c", arms())
def test_absolute_floor(arm, t, c):
    """Family 7: v * 1e-7 (3e-9 .. 3e-6 per head): the ordinary bound with no pre-scaling (the split kernel stops at 2^-25)"""
    ref = P.family_floor(N, c, t, 1.0)
    check_bound(7, arm, ref, arm.attention(ref.qkv, c), what=" v*1e-7")


@pytest.mark.parametrize("arm,t,c,operand", arms("q", "k", "v"))
def test_non_finite_operands_behave_as_in_float32(arm, t, c, operand):
    """Family 6b: NaN, +Inf, -Inf in one element of q, k or v: the output is finite exactly where the float32 CPU evaluation is
    finite, the finite part is within the bound, and everything outside the planted head / row / dim is bitwise unchanged."""
    failures = []
    site = P.sites(N, c, t)[operand]
    for value in (math.nan, math.inf, -math.inf):
        ref = P.Ref(P.plant(P.family_scale(N, c, t, 1.5).qkv, c, site, operand, value), c)
        got = arm.attention(ref.qkv, c)
        P.check_confined(arm, t, N, c, got, {operand: site})
        fin, fin32 = torch.isfinite(got), torch.isfinite(ref.y32)
        both = fin & fin32 & torch.isfinite(ref.truth)
        err = torch.where(both, (got.double() - ref.truth).abs(), torch.zeros_like(ref.truth))
        over = err > ref.per_element(ref.limit(K_TILED))
        print(f"ATTF32 {arm.name} family=6b {operand}={value} T={t} N={N} C={c}: finite {int(fin.sum())} (float32: {int(fin32.sum())}), "
              f"{int((fin != fin32).sum())} differ, {int(over.sum())} finite outputs over the bound")
        if bool((fin != fin32).any()):
            failures.append(f"{operand}={value}: {int((fin & ~fin32).sum())} finite where float32 is not, "
                            f"{int((~fin & fin32).sum())} non-finite where float32 is finite")
        if bool(over.any()):
            failures.append(f"{operand}={value}: {int(over.sum())} finite outputs over the bound")
    assert not failures, failures


# ---- what the switch buys ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def beyond_fp16_case(t, c):
    """family 1 at a = 1.5 with 1.0e5 in one k and one v element of two different (image, head) pairs; (Ref, operand -> site)"""
    where = {o: s for o, s in P.sites(N, c, t).items() if o in ("k", "v")}
    qkv = P.family_scale(N, c, t, 1.5).qkv
    for operand, site in where.items():
        qkv = P.plant(qkv, c, site, operand, 1.0e5)
    return P.Ref(qkv, c), where


@pytest.mark.parametrize("arm", BOTH)
def test_a_finite_value_beyond_fp16_is_simply_computed(arm):
    """1.0e5 in one k and one v element of two different (image, head) pairs at T = 256: dmd_attention (the split kernel, today's
    contract) makes the outputs they feed NaN -- the k element every output of its (image, head), the v element its dim there --
    and dmd_attention_f32 computes them: all finite, within the bound of the float64 truth, everything else bitwise unchanged."""
    t, c = 256, arm.c
    ref, where = beyond_fp16_case(t, c)
    qkv = ref.qkv
    default = arm.other(qkv, c)
    touched = torch.zeros(N, t, c, dtype=torch.bool)
    (ki, kh, _, _), (vi, vh_, _, vd) = where["k"], where["v"]
    touched[ki, :, 8 * kh:8 * kh + 8] = True
    touched[vi, :, 8 * vh_ + vd] = True
    assert not bool(torch.isfinite(default[touched]).any()) and bool(torch.isfinite(default[~touched]).all()), "the default route's contract"
    got = arm.attention(qkv, c)
    P.check_confined(arm, t, N, c, got, where)
    check_bound("6a", arm, ref, got, what=" k, v = 1e5")


# ---- valid extent ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extent_inputs(h, w, vh, vw):
    """qkv (N, H, W, 3C) with NaN / 3e38 margins and the Ref of the cropped tensors"""
    qkv, _, _, _, inside = P.extent_inputs(h, w, vh, vw, seed=h + vh + vw)
    return qkv, P.Ref(qkv[:, :vh, :vw].reshape(P.EXTENT_N, vh * vw, 3 * P.EXTENT_C).contiguous(), P.EXTENT_C), inside


@pytest.mark.parametrize("arm,h,w,vh,vw", abi.arms(SIMT, GPU, P.EXTENT_CASES, tag=abi.joined_by_x))
def test_valid_extent_vs_fp64_of_the_cropped_tensors_with_garbage_margins(arm, h, w, vh, vw):
    qkv, ref, inside = extent_inputs(h, w, vh, vw)
    assert not bool(torch.isfinite(qkv[:, ~inside]).all())
    out = arm.run(qkv, h, w, vh, vw, P.EXTENT_C)
    check_bound("extent", arm, ref, out[:, :vh, :vw].reshape(P.EXTENT_N, vh * vw, P.EXTENT_C), what=f" {h}x{w}/{vh}x{vw}")
    margin = out[:, ~inside]
    assert bool((margin == 0).all()) and not bool(torch.signbit(margin).any()), "out outside the valid extent is not +0"


@pytest.mark.parametrize("arm", BOTH)
def test_whole_grid_extent_is_bitwise_the_flat_call(arm):
    t, c = 320, arm.c
    qkv = P.family_scale(N, c, t, 1.5).qkv
    flat = arm.attention(qkv, c)
    grid = arm.run(qkv.reshape(N, 20, 16, 3 * c), 20, 16, 20, 16, c)
    assert bool(torch.isfinite(flat).all()) and torch.equal(grid.reshape(N, t, c), flat)


@pytest.mark.parametrize("arm", BOTH)
def test_rejects_an_extent_outside_the_grid(arm):
    qkv, _, _ = extent_inputs(16, 16, 9, 9)
    for vh, vw in ((17, 9), (9, 17), (0, 9)):
        with pytest.raises(RuntimeError, match="valid extent"):
            arm.run(qkv, 16, 16, vh, vw, P.EXTENT_C)


# ---- invariance --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_launches_are_bitwise_equal():
    """N = 4, C = 64, T = 1024: more workgroups than CUs"""
    n, c, t = 4, 64, 1024
    qkv = torch.randn(n, t, 3 * c, generator=torch.Generator().manual_seed(12)) * 1.5
    first = GPU.run(qkv, 1, t, 1, t, c)
    assert bool(torch.isfinite(first).all()) and torch.equal(first, GPU.run(qkv, 1, t, 1, t, c))


@pytest.mark.parametrize("arm", BOTH)
def test_an_image_and_a_head_do_not_depend_on_the_others(arm):
    """N = 1 is bitwise the slice of N = 3, and one head alone (C = 8) bitwise its slice of the C-channel call"""
    t, c = 320, arm.c
    qkv = P.family_scale(3, c, t, 4.0).qkv
    full = arm.attention(qkv, c)
    assert bool(torch.isfinite(full).all())
    for i in range(3):
        assert torch.equal(arm.attention(qkv[i:i + 1].contiguous(), c), full[i:i + 1]), i
    hd = c // 8 - 1
    one = torch.cat([qkv[..., s * c + 8 * hd:s * c + 8 * hd + 8] for s in range(3)], dim=-1).contiguous()
    assert torch.equal(arm.attention(one, 8), full[..., 8 * hd:8 * hd + 8])


# ---- agreement with attention_kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm,t,c,family", arms(1, 2, ts=(64, 256, 320, 512, 1024), wide=False))
def test_agrees_with_attention_kernel_within_the_two_bounds(arm, t, c, family):
    """the online-softmax kernel (dmd_attention_valid over the whole grid) on the same inputs: within the sum of the two bounds,
    and not the same bits (another summation order, expf against exp2)"""
    ref = P.family_scale(N, c, t, 8.0) if family == 1 else P.family_offset(N, c, t)
    got, exact = arm.attention(ref.qkv, c), arm.other(ref.qkv, c, exact=True)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(exact).all())
    both = ref.per_element(ref.limit(K_TILED) + ref.limit(P.K_EXACT))
    assert bool(((got.double() - exact.double()).abs() <= both).all()), "the two exact kernels disagree by more than their bounds"
    assert not torch.equal(got, exact)


def test_default_threshold_follows_from_the_recorded_table():
    """engine.ATTN_F32_TILED_MIN_T is the smallest measured token count from which the tiled kernel beats attention_kernel at
    every measured shape by more than the block-to-block spread (profiles/attention_f32_tiled.json)"""
    import json
    import os

    from diamond_amd import engine as E

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attention_f32_tiled.json")) as f:
        table = json.load(f)
    shapes = table["shapes"]
    assert {s["valid_tokens"] for s in shapes} >= {256, 1024, 4096} and any(s["H"] > 1 and s["valid_tokens"] >= 1024 for s in shapes)
    counts = sorted({s["valid_tokens"] for s in shapes})
    wins = [t for t in counts if all(s["faster_by_more_than_the_spread"] for s in shapes if s["valid_tokens"] >= t)]
    assert wins and E.ATTN_F32_TILED_MIN_T == wins[0], (wins, E.ATTN_F32_TILED_MIN_T)
    assert table["derived_threshold"] == wins[0] and table["default_threshold"] == E.ATTN_F32_TILED_MIN_T, "the record is stale"
    assert len({s["N"] for s in shapes if s["valid_tokens"] == wins[0]}) >= 2, "the threshold's token count at more than one N"
    assert any(s["H"] > 1 and wins[0] <= s["valid_tokens"] < 1024 for s in shapes), "a valid-extent grid between the threshold and 1024"


# ---- routing on the interpreter ----------------------------------------------------------------------------------------------------
def test_routing_switch_on_the_interpreter(monkeypatch):
    """the two-level network of tests/test_simt_host.py (attention over 64 tokens at its 8x8 level), inference forward and a
    training step: DIAMOND_ATTN_PRECISION=f32 with DIAMOND_ATTN_F32_MIN_T=64 sends every attention forward to
    attention_f32_tiled_kernel, =0 to attention_kernel; the attn_precision="f32" keyword alone does what the variable does; with
    the switches unset the launches and the bits are a direct dmd_attention call's"""
    from diamond_amd import engine as E
    from diamond_amd import native as nv
    from tests.simt.host_harness import engine_on_interpreter

    den, batch, noisy, obs = P.two_level_denoiser()
    act = batch.act

    seen = []
    attention = E.attention

    def spy(qkv, c, head_dim=8, precision=None):
        out = attention(qkv, c, head_dim, precision)
        seen.append((qkv.t.clone(), out.clone(), c))
        return out

    monkeypatch.setattr(E, "attention", spy)

    def forward(env, **kw):
        for k in ("DIAMOND_ATTN_PRECISION", "DIAMOND_ATTN_F32_MIN_T"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        counter = P.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        del seen[:]
        out = den.compute_model_output(noisy, obs, act[:, :4], 1.3, **kw)
        return out, {k: v for k, v in counter.n.items() if k in P.FORWARD_KEYS}, list(seen)

    with engine_on_interpreter():
        o_def, n_def, s_def = forward({})
        o_new, n_new, _ = forward({"DIAMOND_ATTN_PRECISION": "f32", "DIAMOND_ATTN_F32_MIN_T": "64"})
        o_old, n_old, _ = forward({"DIAMOND_ATTN_PRECISION": "f32", "DIAMOND_ATTN_F32_MIN_T": "0"})
        o_kw, n_kw, _ = forward({"DIAMOND_ATTN_F32_MIN_T": "64"}, attn_precision="f32")
        o_kw16, n_kw16, _ = forward({"DIAMOND_ATTN_PRECISION": "f32", "DIAMOND_ATTN_F32_MIN_T": "64"}, attn_precision="f16x2")
        with pytest.raises(ValueError, match="attention precision"):
            forward({}, attn_precision="f64")
        attn = len(s_def)
        assert attn >= 1 and n_def == {"attention_kernel": attn}, n_def
        for qkv, out, c in s_def:  # the default route: a direct dmd_attention call's bits (64 tokens: attention_kernel)
            assert qkv.shape[1] * qkv.shape[2] == 64
            assert torch.equal(out.reshape(1, 64, c), SIMT.other(qkv.reshape(1, 64, 3 * c), c))
        assert n_new == {"attention_f32_tiled_kernel": attn}, n_new
        assert n_old == {"attention_kernel": attn}, n_old
        assert n_kw == n_new and torch.equal(o_kw, o_new)
        assert n_kw16 == n_def and torch.equal(o_kw16, o_def), "the keyword goes before the variable"
        assert bool(torch.isfinite(o_new).all()) and not torch.equal(o_new, o_def), "the switch changed nothing"
        scale = float(o_def.abs().max())
        assert float((o_new - o_def).abs().max()) <= 1e-4 * scale and float((o_old - o_def).abs().max()) <= 1e-4 * scale

        # the training step: the recorded forward takes the switch, the backward differentiates around its y
        den.train()
        monkeypatch.delenv("DIAMOND_ATTN_BWD_MIN_T", raising=False)
        monkeypatch.setenv("DIAMOND_ATTN_PRECISION", "f32")
        monkeypatch.setenv("DIAMOND_ATTN_F32_MIN_T", "64")
        counter = P.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        loss, grads = P.training_step(den, batch)
        fwd = {k: v for k, v in counter.n.items() if k in P.FORWARD_KEYS}
        assert set(fwd) == {"attention_f32_tiled_kernel"} and counter.n.get("dmd_attention_bwd", 0) == fwd["attention_f32_tiled_kernel"], counter.n
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in grads.values())


# ---- device model level ------------------------------------------------------------------------------------------------------------
def _long_attention_records(tape):
    from diamond_amd.engine import AttnRecord

    return [r for r in tape if isinstance(r, AttnRecord) and r.qkv.shape[1] * r.qkv.shape[2] >= 1024]


@pytest.mark.gpu
def test_model_output_with_exact_attention_is_within_parity_of_the_default_route(monkeypatch):
    """the 1024-token denoiser of test_attention_bwd_mfma, batch 2: other bits, within the contract's 1e-4 of max |output|"""
    from diamond_amd import native as nv

    monkeypatch.setenv("DIAMOND_ATTN_F32_MIN_T", "1024")
    monkeypatch.delenv("DIAMOND_ATTN_PRECISION", raising=False)
    den = P.device_denoiser().eval()
    g = torch.Generator().manual_seed(5)
    noisy, obs = torch.randn(2, 3, 64, 64, generator=g).cuda(), torch.randn(2, 12, 64, 64, generator=g).clamp(-1, 1).cuda()
    act = torch.randint(0, 4, (2, 4), generator=g).cuda()
    got = {}
    for name, kw in (("default", {}), ("f32", {"attn_precision": "f32"})):
        counter = P.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        got[name] = (den.compute_model_output(noisy, obs, act, 1.3, **kw), counter.n)
    (o_def, n_def), (o_new, n_new) = got["default"], got["f32"]
    long_t = n_def.get("attention_f16x2_kernel", 0)
    assert long_t >= 1 and "attention_f32_tiled_kernel" not in n_def, n_def
    assert n_new.get("attention_f32_tiled_kernel", 0) == long_t and "attention_f16x2_kernel" not in n_new, n_new
    diff = float((o_new - o_def).abs().max() / o_def.abs().max())
    print(f"ATTF32 model output, exact attention against the default route: {diff:.3e} of max |output|")
    assert bool(torch.isfinite(o_new).all()) and not torch.equal(o_new, o_def)
    assert diff <= 1e-4, diff


@pytest.mark.gpu
def test_training_step_with_the_exact_forward(monkeypatch):
    """loss and every gradient within 1e-4 of the default route's, and the y the attention backward differentiates around is
    bitwise a direct dmd_attention_f32 call on the recorded qkv"""
    from diamond_amd import native as nv
    from diamond_amd import unet_train as UT

    monkeypatch.setenv("DIAMOND_ATTN_F32_MIN_T", "1024")
    den = P.device_denoiser()
    den.randn_fn = lambda shape: torch.randn(*shape)
    batch = P.device_batches(1)[0]
    checked = []
    backward_tape = UT.backward_tape

    def spy(tape, *a, **kw):
        for rec in _long_attention_records(tape):
            n, h, w, _ = rec.qkv.shape
            direct = torch.full_like(rec.out, float("nan"))
            nv.check(nv.lib().dmd_attention_f32(nv.fptr(rec.qkv.t), nv.fptr(direct), n, 1, h * w, 1, h * w, rec.c, 8, nv.stream()),
                     "dmd_attention_f32")
            checked.append(torch.equal(direct, rec.out))
        return backward_tape(tape, *a, **kw)

    got = {}
    for value in ("f32", None):
        if value is None:
            monkeypatch.delenv("DIAMOND_ATTN_PRECISION", raising=False)
            monkeypatch.setattr(UT, "backward_tape", backward_tape)
        else:
            monkeypatch.setenv("DIAMOND_ATTN_PRECISION", value)
            monkeypatch.setattr(UT, "backward_tape", spy)
        counter = P.LaunchCounter()
        monkeypatch.setattr(nv, "PROFILER", counter)
        got[value] = (P.training_step(den, batch), counter.n)
    (l_new, g_new), n_new = got["f32"]
    (l_old, g_old), n_old = got[None]
    long_t = n_old.get("attention_f16x2_kernel", 0)
    assert long_t >= 1 and n_new.get("attention_f32_tiled_kernel", 0) == long_t and "attention_f16x2_kernel" not in n_new, n_new
    assert len(checked) == long_t and all(checked), checked
    worst = max(float((g_new[k].double() - g.double()).abs().max() / g.double().abs().max().clamp_min(1e-30)) for k, g in g_old.items())
    dl = abs(float(l_new) - float(l_old)) / abs(float(l_old))
    print(f"ATTF32 training step, exact attention forward against the default route: loss {dl:.3e}, worst gradient {worst:.3e} of max |g|")
    assert all(bool(torch.isfinite(v).all()) for v in g_new.values())
    assert dl <= 1e-4 and worst <= 1e-4, (dl, worst)
    assert any(not torch.equal(g_new[k], g_old[k]) for k in g_old), "the switch changed nothing"


@pytest.mark.gpu
def test_graphed_training_step_with_the_switch_on_is_bitwise_the_eager_loop(monkeypatch):
    """test_attention_bwd_mfma's graphed-step test with every attention forward exact: the new launch records into the hipGraph
    like the others (no allocation, no synchronisation, the variables read at capture)"""
    from diamond_amd import native as nv

    monkeypatch.setenv("DIAMOND_ATTN_PRECISION", "f32")
    monkeypatch.setenv("DIAMOND_ATTN_F32_MIN_T", "1024")
    counter = P.LaunchCounter()
    monkeypatch.setattr(nv, "PROFILER", counter)
    P.check_graphed_training_step_is_bitwise_the_eager_loop(monkeypatch)
    assert counter.n.get("attention_f32_tiled_kernel", 0) >= 1 and "attention_f16x2_kernel" not in counter.n, counter.n

