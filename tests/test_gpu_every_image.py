"""EVERY image of production-size launches, not a sample (on a real MI355X).

The persistent kernels (conv_f16ws_kernel, conv1x1_stream_kernel) give a workgroup a contiguous range of tiles, walked from a
rotated start, with the normalisation tables rebuilt in a rotating LDS slot whenever the image under a sub-tile changes; a tile of
the 8x8 and 16x16 levels holds up to eight images.  The tests that launch 256 .. 2100 images (test_gpu_tpw.py, test_gpu_proj_fuse.py)
look at six of them.  A slip at some walk positions only -- the second tile after a slot wrap, a tile that straddles two images at
a rotated start, the last, shorter tile range, a stale table for one image of eight -- lands on a handful of images the sample misses.

An image's result does not depend on where its tiles fall, on N, or on its neighbours (include/diamond_hip.h; the same holds for
the GroupNorm backward, the attention cores and the rows of dmd_linear).  So the batch is built from P = 11 DISTINCT images repeated
cyclically (image i is a copy of image i % 11: activations, FiLM rows, residuals, projection sources, gradients).  11 is a prime
above 8, the most images one tile holds: no tile holds two copies of one image and direct neighbours always differ, so a read of
the neighbour's table, statistics or pixels changes the result.  N is never a multiple of 11 (the last period is cut).  Per launch:
  (1) every copy is BITWISE its first occurrence, the emitted GroupNorm partial statistics too (compared on the device; a failure
      names the differing images, N, tiles and tiles_per_wg, from which the walk position can be read off);
  (2) the 11 distinct images of the big launch against the float64 torch-CPU evaluation at the per-op bars of the existing tests
      (2e-5 convolutions and GroupNorm backward, 1e-5 linear and attention) -- with (1): every image of the launch is inside the bar;
  (3) the same 11 images launched alone (tiles_per_wg == 1) give the same bits;
  (4) the big launch repeated once gives the same bits;
  (5) nothing is left unwritten: the outputs are torch.empty, so the block the output will get is filled with NaN and freed right
      before the launch; afterwards the output has to lie in that block and be finite.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import CONV_CASES, gn_ref, rel_err
from tests.test_gpu_proj_fuse import CASES as PROJ_CASES, _inputs, _launch, _params_of
from tests.test_gpu_tpw import NCU, TPW_PARAMS, _agent, _run, _streams, _tiles

pytestmark = pytest.mark.gpu
DEV = "cuda"

P = 11  # distinct images of a batch: a prime above the eight images one tile can hold


# ------------------------------------------------------------------------------------------------------------
# the two helpers: periodic expansion, comparison of the copies
# ------------------------------------------------------------------------------------------------------------
def periodic(t, n):
    """P distinct images (or rows) -> n of them: image i is a copy of image i % P"""
    assert t.shape[0] == P and n % P != 0, (t.shape, n)
    return t[torch.arange(n, device=t.device) % P].contiguous()


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def differing(a, b):
    """the indices along dim 0 at which a and b differ in any bit (compared where the tensors are)"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return (_bits(a) != _bits(b)).flatten(1).any(1).nonzero().flatten().tolist()


def assert_copies(what, t, where=""):
    """(1): t[i] is bitwise t[i % P] for every i"""
    n = t.shape[0]
    bad = differing(t, t[torch.arange(n, device=t.device) % P])
    assert not bad, f"{what}: {len(bad)} of {n} images differ from their first occurrence (image i % {P}); the first: {bad[:20]}{where}"


def assert_same_bits(what, a, b, where=""):
    bad = differing(a, b)
    assert not bad, f"{what}: {len(bad)} of {a.shape[0]} images differ; the first: {bad[:20]}{where}"


def launch_over_poison(launch, shape, main=lambda r: r, dtype=torch.float32):
    """(5): `launch()` with its main output (`main(result)`, a torch.empty of `shape`) lying in a block that held NaN a moment ago.
    Where the caching allocator hands the launch another block, the check is held to the first launch after empty_cache()."""
    for attempt in range(2):
        if attempt:
            torch.cuda.empty_cache()
        poison = torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV)
        ptr = poison.data_ptr()
        del poison
        res = launch()
        out = main(res)
        assert tuple(out.shape) == tuple(shape) and out.dtype == dtype, (out.shape, shape, out.dtype)
        if out.data_ptr() == ptr:
            return res
        del res, out
    raise AssertionError("the caching allocator did not hand the launch the block that was filled with NaN, not even for the first "
                         "launch after torch.cuda.empty_cache(): whether every output element is written could not be checked")


def assert_finite(what, t):
    assert bool(torch.isfinite(t).all()), f"{what}: not finite -- an element of the output block (NaN before the launch) was never written"


def launch_keys(fn):
    """(result, the entry points `fn` launched through and the kernel keys their callers gave them)"""
    from diamond_amd import native as nv

    names = []

    class Names(nv.LaunchProfiler):
        def call(self, name, fn, args):
            names.append(name)
            return super().call(name, fn, args)

    nv.PROFILER = Names()
    try:
        res = fn()
        keys = sorted(set(nv.PROFILER.summary().keys()) | set(names))
    finally:
        nv.PROFILER = None
    return res, keys


def garbage_margins(core, n, hp, wp, g, nan_copies=(3, 14, 20)):
    """(P, vh, vw, C) distinct images -> the (n, hp, wp, C) buffers of their periodic batch: the images are the valid extent, the
    margins of EVERY copy hold other finite garbage (large, so that an unmasked read shows), those of a few copies NaN"""
    _, vh, vw, c = core.shape
    buf = torch.randn(n, hp, wp, c, device=DEV, generator=g) * 40.0 + torch.arange(n, device=DEV).view(n, 1, 1, 1) * 3.0 - 50.0
    for k in nan_copies:
        buf[k % n] = float("nan")
    buf[:, :vh, :vw] = periodic(core, n)
    return buf


# ------------------------------------------------------------------------------------------------------------
# A. convolutions
# ------------------------------------------------------------------------------------------------------------
def conv_ref64(xs, cins, mul, add, wgt, bias, res, prologue, k, up=False, stride=1):
    """float64 torch-CPU evaluation of the launch on NHWC device tensors (the op of test_gpu_tpw.py)"""
    parts, c0 = [], 0
    for x, c in zip(xs, cins):
        y = x.double().cpu().permute(0, 3, 1, 2)
        if prologue:
            sc, sh = mul[:, c0:c0 + c].double().cpu(), add[:, c0:c0 + c].double().cpu()
            y = gn_ref(y, max(1, c // 32)) * (1 + sc[:, :, None, None]) + sh[:, :, None, None]
            if prologue == 1:
                y = y * torch.sigmoid(y)
        parts.append(y)
        c0 += c
    xin = torch.cat(parts, 1)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, wgt.double().cpu(), bias.double().cpu(), stride=stride, padding=1 if k == 3 else 0)
    if res is not None:
        ref = ref + res.double().cpu().permute(0, 3, 1, 2)
    return ref


def _stream_tiles(n, h, w, cin):
    """tiles and tiles_per_wg of conv1x1_stream_kernel (mirrors launch1x1s, csrc/dmd_conv1x1.hip)"""
    tiles = (n * h * w + (128 if cin == 128 else 256) - 1) // (128 if cin == 128 else 256)
    return tiles, (tiles + min(tiles, 1024) - 1) // min(tiles, 1024)


def check_stats64(what, stats, ref):
    """emitted partial statistics of the P distinct images against the float64 result (the bar of test_gpu_tpw.py)"""
    st = stats[:P].cpu().sum(dim=2)
    refg = ref.reshape(P, stats.shape[1], -1)
    e = rel_err(st[..., 1], refg.square().sum(-1))
    assert e < 2e-5, f"{what}: sums of squares {e:.3e}"


@pytest.mark.parametrize("case,precision", TPW_PARAMS)
def test_persistent_conv_every_image(case, precision):
    """every `WsGeom` instance of conv_f16ws_kernel and conv1x1_stream_kernel (both precisions) at tiles_per_wg >= 2: (1) - (5).
    N is the table's, plus one where that is a multiple of 11 (1100 -> 1101: the last period has to be cut)."""
    from diamond_amd import engine as E, native as nv

    name, n, h, w, cins, cout, taps, up, prologue, use_res, head = case
    n += n % P == 0
    stream = _streams(case)
    cin = sum(cins)
    k = 3 if taps == 9 else 1
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    info = _stream_tiles(n, ho, wo, cin) if stream else _tiles(n, ho, wo, 32 if head else cout, taps, stream)
    assert info[1] >= 2, f"{name}: case does not reach tiles_per_wg >= 2 ({info})"
    where = f" (N={n}, tiles={info[0]}, tiles_per_wg={info[1]})"
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, name)))
    xs_d = [torch.randn(P, h, w, c, device=DEV, generator=g) * 1.5 + 0.3 for c in cins]
    wgt = torch.randn(cout, cin, k, k, device=DEV, generator=g) / math.sqrt(cin * k * k)
    bias = torch.randn(cout, device=DEV, generator=g) * 0.1
    mul_d = torch.randn(P, cin, device=DEV, generator=g) * 0.3
    add_d = torch.randn(P, cin, device=DEV, generator=g) * 0.3
    res_d = torch.randn(P, ho, wo, cout, device=DEV, generator=g) if use_res else None
    xs, mul, add = [periodic(x, n) for x in xs_d], periodic(mul_d, n), periodic(add_d, n)
    res = periodic(res_d, n) if use_res else None
    f16 = precision == "f16x2"
    launch = lambda: _run(E, nv, xs, prologue, mul, add, cin, wgt, bias, cout, taps, up, res, head, f16)
    out = launch_over_poison(launch, (n, cout, ho, wo) if head else (n, ho, wo, cout), main=lambda r: r.t)
    torch.cuda.synchronize()
    # (5), (1)
    assert_finite(name, out.t)
    assert_copies(name, out.t, where)
    if out.stats is not None:
        assert_finite(name + " statistics", out.stats)
        assert_copies(name + " statistics", out.stats, where)
    # (2)
    ref = conv_ref64(xs_d, cins, mul_d, add_d, wgt, bias, res_d, prologue, k, up)
    err = rel_err(out.t[:P] if head else out.t[:P].permute(0, 3, 1, 2), ref)
    print(f"{name}/{precision}:{where} rel err vs fp64 on the {P} distinct images: {err:.3e}")
    assert err < 2e-5, f"{name}: rel err {err:.3e}"
    if out.stats is not None:
        check_stats64(name, out.stats, ref)
    # (3)
    small_info = _stream_tiles(P, ho, wo, cin) if stream else _tiles(P, ho, wo, 32 if head else cout, taps, stream)
    assert small_info[1] == 1, small_info
    small = _run(E, nv, xs_d, prologue, mul_d, add_d, cin, wgt, bias, cout, taps, up, res_d, head, f16)
    assert_same_bits(f"{name}: N={n} against the N={P} launch", out.t[:P], small.t, where)
    if out.stats is not None:
        assert_same_bits(f"{name}: statistics, N={n} against the N={P} launch", out.stats[:P], small.stats, where)
    # (4)
    again = launch()
    assert_same_bits(f"{name}: run to run", out.t, again.t, where)
    if out.stats is not None:
        assert_same_bits(f"{name}: statistics, run to run", out.stats, again.stats, where)


PROJ_EVERY = [c for c in PROJ_CASES if c[0] in ("tpw3_64x64_N41_odd", "tpw4_32x32_N256", "tpw2_16x16_N300")]
assert len(PROJ_EVERY) == 3


@pytest.mark.parametrize("name,n,hw", PROJ_EVERY, ids=[c[0] for c in PROJ_EVERY])
def test_fused_projection_every_image(name, n, hw):
    """`proj(cat(xa, xb)) + conv2(silu(norm2(h)))` as one launch (WsGeomProj): (1) - (5), the projection sources periodic too"""
    from diamond_amd import engine as E, native as nv

    tiles = n * (hw // 16) ** 2
    tpw = (tiles + NCU - 1) // NCU
    assert tpw >= 2 and (P * (hw // 16) ** 2 + NCU - 1) // NCU == 1
    where = f" (N={n}, tiles={tiles}, tiles_per_wg={tpw})"
    args_d = _inputs(P, hw, 1234 + n)
    big = [periodic(t, n) for t in args_d[:5]] + args_d[5:]
    assert "WsGeomProj" in E.kernel_key(_params_of(E, nv, *big)), "the fused launch must run the projection geometry"
    out = launch_over_poison(lambda: _launch(E, nv, *big, fused=True), (n, hw, hw, 64), main=lambda r: r.t)
    torch.cuda.synchronize()
    assert_finite(name, out.t)
    assert_finite(name + " statistics", out.stats)
    assert_copies(name, out.t, where)
    assert_copies(name + " statistics", out.stats, where)
    h, xa, xb, mul, add, w2, b2, wp, bp = args_d
    ref = conv_ref64([h], [64], mul, add, w2, b2, None, 1, 3)
    ref = ref + F.conv2d(torch.cat([xa, xb], dim=3).double().cpu().permute(0, 3, 1, 2), wp.double().cpu(), bp.double().cpu())
    err = rel_err(out.t[:P].permute(0, 3, 1, 2), ref)
    print(f"{name}:{where} rel err vs fp64 on the {P} distinct images: {err:.3e}")
    assert err < 2e-5, f"{name}: rel err {err:.3e}"
    check_stats64(name, out.stats, ref)
    small = _launch(E, nv, *args_d, fused=True)
    assert_same_bits(f"{name}: N={n} against the N={P} launch", out.t[:P], small.t, where)
    assert_same_bits(f"{name}: statistics, N={n} against the N={P} launch", out.stats[:P], small.stats, where)
    again = _launch(E, nv, *big, fused=True)
    assert_same_bits(f"{name}: run to run", out.t, again.t, where)
    assert_same_bits(f"{name}: statistics, run to run", out.stats, again.stats, where)


def test_valid_extent_conv_every_image():
    """64 -> 64, 3x3, NORM_SILU with per-image FiLM rows, residual, split-fp16, a 72x72 VALID EXTENT in an 80x80 buffer at N = 23:
    25 tiles per image, 575 tiles, 3 per workgroup.  Positions outside the extent read as zero whatever the buffer holds
    (include/diamond_hip.h): the input and residual margins of every copy hold other garbage, those of three copies NaN.  The
    valid part of the output and all of the statistics: (1) - (5); the images alone as two launches of six (150 tiles each)."""
    from diamond_amd import engine as E, native as nv

    n, c, (vh, vw), (hp, wp) = 23, 64, (72, 72), (80, 80)
    tiles = n * (hp // 16) * (wp // 16)
    tpw = (tiles + NCU - 1) // NCU
    assert (tiles, tpw) == (575, 3)
    where = f" (N={n}, tiles={tiles}, tiles_per_wg={tpw})"
    g = torch.Generator(device=DEV).manual_seed(7223)
    x_d = torch.randn(P, vh, vw, c, device=DEV, generator=g) * 1.5 + 0.3
    r_d = torch.randn(P, vh, vw, c, device=DEV, generator=g)
    mul_d = torch.randn(P, c, device=DEV, generator=g) * 0.3
    add_d = torch.randn(P, c, device=DEV, generator=g) * 0.3
    wgt = torch.randn(c, c, 3, 3, device=DEV, generator=g) / math.sqrt(c * 9)
    bias = torch.randn(c, device=DEV, generator=g) * 0.1
    xb, rb = garbage_margins(x_d, n, hp, wp, g), garbage_margins(r_d, n, hp, wp, g, nan_copies=(5, 14, 22))
    mul, add = periodic(mul_d, n), periodic(add_d, n)
    wp32, wp16, bpad = nv.pack_conv_weight(wgt), nv.pack_conv_weight_f16x2(wgt), nv.pad_vector(bias, nv.cout_pad(c))

    def run(xbuf, rbuf, m, a):
        spec = E.NormSpec(mul=m, add=a, mul_stride=c, add_stride=c, plus_one=True)
        return E.conv2d([(E.gn_stats(xbuf, (vh, vw)), nv.PROLOGUE_NORM_SILU, spec)], wp32, bpad, c, residual=E.Act(rbuf, valid=(vh, vw)),
                        w_f16=wp16)

    (out, keys) = launch_keys(lambda: launch_over_poison(lambda: run(xb, rb, mul, add), (n, hp, wp, c), main=lambda r: r.t))
    torch.cuda.synchronize()
    assert any(k.startswith("conv_f16ws_kernel") for k in keys), keys
    assert out.valid == (vh, vw)
    got = out.t[:, :vh, :vw].contiguous()
    assert_finite("valid extent", got)  # (the margins of the output are nobody's: left out)
    assert_finite("valid extent statistics", out.stats)
    assert_copies("valid extent", got, where)
    assert_copies("valid extent statistics", out.stats, where)
    ref = conv_ref64([x_d], [c], mul_d, add_d, wgt, bias, r_d, 1, 3)
    err = rel_err(got[:P].permute(0, 3, 1, 2), ref)
    print(f"valid extent 72x72 in 80x80:{where} rel err vs fp64 on the {P} distinct images: {err:.3e}")
    assert err < 2e-5, err
    check_stats64("valid extent", out.stats, ref)
    for lo, hi in ((0, 6), (5, 11)):
        assert ((hi - lo) * 25 + NCU - 1) // NCU == 1
        small = run(xb[lo:hi].contiguous(), rb[lo:hi].contiguous(), mul[lo:hi].contiguous(), add[lo:hi].contiguous())
        assert_same_bits(f"valid extent: N={n} against images {lo}..{hi - 1} alone", got[lo:hi], small.t[:, :vh, :vw].contiguous(), where)
        assert_same_bits(f"valid extent statistics: N={n} against images {lo}..{hi - 1} alone", out.stats[lo:hi], small.stats, where)
    again = run(xb, rb, mul, add)
    assert_same_bits("valid extent: run to run", got, again.t[:, :vh, :vw].contiguous(), where)
    assert_same_bits("valid extent statistics: run to run", out.stats, again.stats, where)


def _grid_case(name):
    """a CONV_CASES row (3x3, no upsampling, NHWC) as a row of GRID_CASES in exact fp32"""
    _, _, h, w, cins, cout, taps, stride, up, prologue, use_res, nchw = next(c for c in CONV_CASES if c[0] == name)
    assert taps == 9 and not up and not nchw
    return (name + "_f32", h, w, cins, cout, stride, prologue, use_res, "f32")


GRID_CASES = [
    # name, H, W, [Cin...], Cout, stride, prologue, residual, precision
    ("down_64to32_f16x2", 64, 64, [64], 64, 2, 0, False, "f16x2"),
    _grid_case("c64_16x16"),
    _grid_case("cat128_32x32"),
]


@pytest.mark.parametrize("name,h,w,cins,cout,stride,prologue,use_res,precision", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_conv_mfma_every_image(name, h, w, cins, cout, stride, prologue, use_res, precision):
    """conv_mfma_kernel (not persistent: a workgroup per tile) at N = 45 -- the stride-2 conv in split-fp16, `c64_16x16` and
    `cat128_32x32` of CONV_CASES in exact fp32: independence of the grid position, (1), (2), (4) (and (5))"""
    from diamond_amd import engine as E, native as nv

    n, cin = 45, sum(cins)
    ho, wo = h // stride, w // stride
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, name)))
    xs_d = [torch.randn(P, h, w, c, device=DEV, generator=g) * 1.5 + 0.3 for c in cins]
    wgt = torch.randn(cout, cin, 3, 3, device=DEV, generator=g) / math.sqrt(cin * 9)
    bias = torch.randn(cout, device=DEV, generator=g) * 0.1
    mul_d = torch.randn(P, cin, device=DEV, generator=g) * 0.3
    add_d = torch.randn(P, cin, device=DEV, generator=g) * 0.3
    res_d = torch.randn(P, ho, wo, cout, device=DEV, generator=g) if use_res else None
    wp32, bpad = nv.pack_conv_weight(wgt), nv.pad_vector(bias, nv.cout_pad(cout))

    def run(xs, mul, add, res):
        srcs, c0 = [], 0
        for x in xs:
            spec = E.NormSpec(mul=mul[:, c0:], add=add[:, c0:], mul_stride=cin, add_stride=cin, plus_one=True) if prologue else None
            srcs.append((E.gn_stats(x) if prologue else E.Act(x), prologue, spec))
            c0 += x.shape[3]
        return E.conv2d(srcs, wp32, bpad, cout, stride=stride, residual=E.Act(res) if res is not None else None,
                        fast_math=precision == "f16x2")

    xs, mul, add = [periodic(x, n) for x in xs_d], periodic(mul_d, n), periodic(add_d, n)
    res = periodic(res_d, n) if use_res else None
    where = f" (N={n}, conv_mfma_kernel: one workgroup per tile)"
    out, keys = launch_keys(lambda: launch_over_poison(lambda: run(xs, mul, add, res), (n, ho, wo, cout), main=lambda r: r.t))
    torch.cuda.synchronize()
    assert any(k.startswith("conv_mfma_kernel") for k in keys) and not any(k.startswith("conv_f16ws") for k in keys), keys
    assert_finite(name, out.t)
    assert_finite(name + " statistics", out.stats)
    assert_copies(name, out.t, where)
    assert_copies(name + " statistics", out.stats, where)
    ref = conv_ref64(xs_d, cins, mul_d, add_d, wgt, bias, res_d, prologue, 3, stride=stride)
    err = rel_err(out.t[:P].permute(0, 3, 1, 2), ref)
    print(f"{name}:{where} rel err vs fp64 on the {P} distinct images: {err:.3e}")
    assert err < 2e-5, f"{name}: rel err {err:.3e}"
    check_stats64(name, out.stats, ref)
    again = run(xs, mul, add, res)
    assert_same_bits(f"{name}: run to run", out.t, again.t, where)
    assert_same_bits(f"{name}: statistics, run to run", out.stats, again.stats, where)


# ------------------------------------------------------------------------------------------------------------
# B. GroupNorm backward: every route of gn_bwd_route, per sample
# ------------------------------------------------------------------------------------------------------------
def gn_route(n, hw, c):
    """mirror of gn_bwd_route (csrc/dmd_backward.hip) at the default DIAMOND_GN_BWD_FUSED"""
    if 256 % (c // 4) != 0 or (c % 32 != 0 and c > 32):
        return "GENERAL"
    t = (hw + 255) // 256
    if t == 1:
        return "FUSED_REGS" if n <= 256 else "FUSED"
    return "TILES_U4" if t * n <= 1024 else "TILES_U1"


def gn_bwd_ref64(x, mul, add, da, dskip, identity):
    """float64 autograd of act(GroupNorm(x) * (1 + mul[n]) + add[n]) on NHWC tensors of the P distinct images: the gradients of x and
    of EVERY sample's own FiLM rows"""
    x = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    mul, add = mul.double().cpu().requires_grad_(True), add.double().cpu().requires_grad_(True)
    c = x.shape[1]
    u = gn_ref(x, max(1, c // 32)) * (1 + mul[:, :, None, None]) + add[:, :, None, None]
    a = u if identity else u * torch.sigmoid(u)
    tot = (a * da.double().cpu().permute(0, 3, 1, 2)).sum()
    if dskip is not None:
        tot = tot + (x * dskip.double().cpu().permute(0, 3, 1, 2)).sum()
    tot.backward()
    return x.grad.permute(0, 2, 3, 1), mul.grad, add.grad


def check_gn_bwd_per_sample(what, dx, dmul, dadd, want):
    for i in range(P):
        for key, got, ref in (("dx", dx[i], want[0][i]), ("dmul", dmul[i], want[1][i]), ("dadd", dadd[i], want[2][i])):
            e = rel_err(got, ref)
            assert e < 2e-5, f"{what}: {key} of image {i}: {e:.3e}"


GN_ROUTES = [  # route, C, side, N
    ("FUSED_REGS", 64, 16, 200),
    ("FUSED", 64, 16, 300),
    ("TILES_U4", 32, 32, 100),
    ("TILES_U1", 32, 32, 300),
    ("GENERAL", 48, 16, 300),
]
GN_ARMS = [("silu", False, False), ("silu-dskip", True, False), ("identity-dskip", True, True)]


@pytest.mark.parametrize("arm,skip,identity", GN_ARMS, ids=[a[0] for a in GN_ARMS])
@pytest.mark.parametrize("route,c,side,n", GN_ROUTES, ids=[r[0] for r in GN_ROUTES])
def test_gn_bwd_every_image_per_sample(route, c, side, n, arm, skip, identity):
    """dmd_gn_silu_bwd with per-image FiLM rows on a periodic batch: dx, dmul[n] and dadd[n] of every image bitwise its first
    occurrence's, those of the 11 distinct images against float64 autograd PER SAMPLE (a sum over n would hide two samples' rows
    swapped); the 11 images alone (another route, the same bits: dmd_backward.hip); run to run; nothing unwritten.  identity: the
    attention pre-norm."""
    from diamond_amd import engine as E, grad_ops as G

    assert gn_route(n, side * side, c) == route, (gn_route(n, side * side, c), route)
    where = f" (N={n}, route {route}, C={c}, {side}x{side})"
    g = torch.Generator(device=DEV).manual_seed(n + c + side + 2 * skip + identity)
    x_d = torch.randn(P, side, side, c, device=DEV, generator=g) * 1.7 + 0.4
    da_d = torch.randn(P, side, side, c, device=DEV, generator=g)
    ds_d = torch.randn(P, side, side, c, device=DEV, generator=g) if skip else None
    mul_d = torch.randn(P, c, device=DEV, generator=g) * 0.3
    add_d = torch.randn(P, c, device=DEV, generator=g) * 0.3

    def run(x, mul, add, da, ds, poison=False):
        spec = E.NormSpec(mul=mul, add=add, mul_stride=c, add_stride=c, plus_one=True)
        xa = E.gn_stats(x)
        launch = lambda: G.gn_bwd(xa, spec, da, ds, identity)
        return launch_over_poison(launch, tuple(x.shape), main=lambda r: r[0]) if poison else launch()

    big = [periodic(t, n) if t is not None else None for t in (x_d, mul_d, add_d, da_d, ds_d)]
    dx, dma = run(*big, poison=True)
    torch.cuda.synchronize()
    for key, t in (("dx", dx), ("dmul", dma[0]), ("dadd", dma[1])):
        assert_finite(f"{route}/{arm} {key}", t)
        assert_copies(f"{route}/{arm} {key}", t, where)
    want = gn_bwd_ref64(x_d, mul_d, add_d, da_d, ds_d, identity)
    check_gn_bwd_per_sample(f"{route}/{arm}", dx, dma[0], dma[1], want)
    dx11, dma11 = run(x_d, mul_d, add_d, da_d, ds_d)
    for key, a, b in (("dx", dx, dx11), ("dmul", dma[0], dma11[0]), ("dadd", dma[1], dma11[1])):
        assert_same_bits(f"{route}/{arm} {key}: N={n} against the N={P} launch", a[:P], b, where)
    dx2, dma2 = run(*big)
    assert_same_bits(f"{route}/{arm} dx: run to run", dx, dx2, where)
    assert_same_bits(f"{route}/{arm} dmul, dadd: run to run", dma.transpose(0, 1), dma2.transpose(0, 1), where)


def test_gn_bwd_valid_extent_every_image():
    """a 13x17 extent in a 15x20 buffer at N = 513 (two tiles per image, the second partial; T N = 1026: one pixel per trip), a
    skip gradient, per-image FiLM rows; the margins of x, da and dskip of every copy hold other garbage, those of three copies NaN.
    dx is exactly zero outside the extent."""
    from diamond_amd import engine as E, grad_ops as G

    n, c, (vh, vw), (hp, wp) = 513, 32, (13, 17), (15, 20)
    assert gn_route(n, hp * wp, c) == "TILES_U1"
    where = f" (N={n}, route TILES_U1, {vh}x{vw} in {hp}x{wp})"
    g = torch.Generator(device=DEV).manual_seed(513)
    x_d = torch.randn(P, vh, vw, c, device=DEV, generator=g) * 1.7 + 0.4
    da_d = torch.randn(P, vh, vw, c, device=DEV, generator=g)
    ds_d = torch.randn(P, vh, vw, c, device=DEV, generator=g)
    mul_d = torch.randn(P, c, device=DEV, generator=g) * 0.3
    add_d = torch.randn(P, c, device=DEV, generator=g) * 0.3
    xb = garbage_margins(x_d, n, hp, wp, g, nan_copies=(3, 258, 512))
    dab = garbage_margins(da_d, n, hp, wp, g, nan_copies=(4, 258, 500))
    dsb = garbage_margins(ds_d, n, hp, wp, g, nan_copies=(5, 258, 511))
    spec = E.NormSpec(mul=periodic(mul_d, n), add=periodic(add_d, n), mul_stride=c, add_stride=c, plus_one=True)
    xa = E.gn_stats(xb, (vh, vw))
    dx, dma = launch_over_poison(lambda: G.gn_bwd(xa, spec, dab, dsb), (n, hp, wp, c), main=lambda r: r[0])
    torch.cuda.synchronize()
    inside = torch.zeros(hp, wp, dtype=torch.bool, device=DEV)
    inside[:vh, :vw] = True
    outside = dx[:, ~inside]
    bad = (outside != 0).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"dx outside the valid extent is not zero in images {bad[:20]}{where}"
    for key, t in (("dx", dx), ("dmul", dma[0]), ("dadd", dma[1])):
        assert_finite(f"valid extent {key}", t)
        assert_copies(f"valid extent {key}", t, where)
    want = gn_bwd_ref64(x_d, mul_d, add_d, da_d, ds_d, False)
    check_gn_bwd_per_sample("valid extent", dx[:, :vh, :vw], dma[0], dma[1], want)
    dx2, dma2 = G.gn_bwd(xa, spec, dab, dsb)
    assert_same_bits("valid extent dx: run to run", dx, dx2, where)
    assert_same_bits("valid extent dmul, dadd: run to run", dma.transpose(0, 1), dma2.transpose(0, 1), where)


# ------------------------------------------------------------------------------------------------------------
# C. dmd_linear: an output row is summed in the same order whatever the batch size
# ------------------------------------------------------------------------------------------------------------
LINEAR_ARMS = [(7168, 256, 0, 0)] + [(nn, kk, ta, tw) for nn, kk in ((512, 1024), (33, 72)) for ta, tw in ((0, 0), (1, 0), (0, 1), (1, 1))]


@pytest.mark.parametrize("n,k,ta,tw", LINEAR_ARMS, ids=[f"N{a[0]}-K{a[1]}-ta{a[2]}-tw{a[3]}" for a in LINEAR_ARMS])
def test_linear_every_row(n, k, ta, tw):
    """M = 1000 rows of period 11 -- plain (7168, 256), split-K (512, 1024), masked K tail (33, 72), the latter two also with either
    operand a transposed view (test_linear_transposed.py's modes): with a bias, accumulated onto a periodic C, with SiLU.  Rows that
    are copies are bitwise equal, rows 0 .. 10 within 1e-5 of float64 and bitwise the M = 11 call."""
    from diamond_amd import engine as E

    m = 1000
    g = torch.Generator(device=DEV).manual_seed(m + n + k + 2 * ta + tw)
    a_d = torch.randn(P, k, device=DEV, generator=g)
    w = torch.randn(n, k, device=DEV, generator=g) / math.sqrt(k)
    bias = torch.randn(n, device=DEV, generator=g)
    c_d = torch.randn(P, n, device=DEV, generator=g)
    stored = lambda t, trans: t.t().contiguous().t() if trans else t  # (rows, K) logical; transposed: a view of a row-major (K, rows) matrix
    a, a11, wv = stored(periodic(a_d, m), ta), stored(a_d, ta), stored(w, tw)
    assert (a.stride(1) != 1) == bool(ta) and (wv.stride(1) != 1) == bool(tw)
    a64, w64, b64, c64 = (t.double().cpu() for t in (a_d, w, bias, c_d))
    lin = a64 @ w64.t() + b64
    arms = (("bias", dict(), lambda: None, lin),
            ("bias + accumulate", dict(accumulate=True), lambda: periodic(c_d, m), lin + c64),
            ("bias + silu", dict(silu=True), lambda: None, lin * torch.sigmoid(lin)))
    for what, kw, c0, ref in arms:
        out = E.linear(a, wv, bias, out=c0(), **kw)
        where = f" (M={m}, N={n}, K={k}, trans_a={ta}, trans_w={tw}, {what})"
        assert_finite(what, out)
        assert_copies("dmd_linear rows", out, where)
        err = rel_err(out[:P], ref)
        assert err < 1e-5, f"rows 0..{P - 1} vs fp64 {err:.3e}{where}"
        small = E.linear(a11, wv, bias, out=None if c0() is None else c_d.clone(), **kw)
        assert_same_bits("dmd_linear rows, M=1000 against M=11", out[:P], small, where)


# ------------------------------------------------------------------------------------------------------------
# D. attention cores: the result of an image does not depend on N or on the other heads
# ------------------------------------------------------------------------------------------------------------
ATT_N, ATT_C = 23, 64


def attention_ref64(qkv):
    """softmax(q k^T / sqrt(8)) v per head in float64 on the CPU, image by image: (n, T, 3C) -> (n, T, C)"""
    from tests.attention_cases import formula

    return formula(qkv.cpu(), ATT_C, torch.float64)


ATT_ARMS = [  # name, grid (H, W), extent or None, precision, entry point, kernel
    ("attention_kernel_T64", (8, 8), None, None, "dmd_attention", "attention_kernel"),
    ("attention_f16x2_kernel_T256", (16, 16), None, None, "dmd_attention", "attention_f16x2_kernel"),
    ("dmd_attention_f16x2_24x25_of_32x32", (32, 32), (24, 25), None, "dmd_attention_f16x2", "attention_f16x2_kernel"),
    ("dmd_attention_f32_24x25_of_32x32", (32, 32), (24, 25), "f32", "dmd_attention_f32", "attention_f32_tiled_kernel"),
]


@pytest.mark.parametrize("name,grid,extent,precision,entry,kernel", ATT_ARMS, ids=[a[0] for a in ATT_ARMS])
def test_attention_every_image(name, grid, extent, precision, entry, kernel, monkeypatch):
    """engine.attention on N = 23 images of periodic qkv, C = 64: every image bitwise its first occurrence, the 11 distinct ones
    within 1e-5 of the float64 softmax formula and bitwise the N = 11 launch, run to run, nothing unwritten.  The extent arms: the
    margins of every copy hold other garbage (three copies NaN), valid rows compared, the remaining rows +0."""
    from diamond_amd import engine as E

    for key in ("DIAMOND_ATTN_PRECISION", "DIAMOND_ATTN_F32_MIN_T", "DIAMOND_ATTN_F16X2_MIN_T"):
        monkeypatch.delenv(key, raising=False)
    n, c, (h, w) = ATT_N, ATT_C, grid
    vh, vw = extent or grid
    where = f" (N={n}, {name})"
    g = torch.Generator(device=DEV).manual_seed(h * w + vh + (precision == "f32"))
    qkv_d = torch.randn(P, vh, vw, 3 * c, device=DEV, generator=g) * 1.5
    qkv = garbage_margins(qkv_d, n, h, w, g) if extent else periodic(qkv_d, n)

    def run(t):
        return E.attention(E.Act(t, valid=extent), c, precision=precision)

    (out, keys) = launch_keys(lambda: launch_over_poison(lambda: run(qkv), (n, h, w, c)))
    torch.cuda.synchronize()
    assert keys == sorted((entry, kernel)), keys
    assert_finite(name, out)
    assert_copies(name, out, where)
    got = out[:, :vh, :vw]
    ref = attention_ref64(qkv_d.reshape(P, vh * vw, 3 * c)).reshape(P, vh, vw, c)
    err = rel_err(got[:P], ref)
    print(f"{name}: rel err vs fp64 on the {P} distinct images: {err:.3e}")
    assert err < 1e-5, f"{name}: rel err {err:.3e}"
    if extent:
        inside = torch.zeros(h, w, dtype=torch.bool, device=DEV)
        inside[:vh, :vw] = True
        m = out[:, ~inside]
        assert bool((m == 0).all()) and not bool(torch.signbit(m).any()), f"{name}: out outside the valid extent is not +0"
    small = run(qkv[:P].contiguous())
    assert_same_bits(f"{name}: N={n} against the N={P} launch", out[:P], small, where)
    again = run(qkv)
    assert_same_bits(f"{name}: run to run", out, again, where)


def attention_bwd_ref64(qkv, dy):
    """float64 autograd of the softmax formula, image by image: (n, T, 3C), (n, T, C) -> dqkv (n, T, 3C)"""
    from tests.attention_cases import formula

    outs = []
    for x, d in zip(qkv.double().cpu(), dy.double().cpu()):
        x = x[None].clone().requires_grad_(True)
        formula(x, ATT_C, torch.float64).backward(d[None])
        outs.append(x.grad)
    return torch.cat(outs)


@pytest.mark.parametrize("side", [16, 32], ids=["scalar_pair_T256", "mfma_pair_T1024"])
def test_attention_bwd_every_image(side, monkeypatch):
    """grad_ops.attention_bwd on N = 23 periodic images, one T under attn_bwd_mfma_min_t() (the scalar pair) and one over it (the
    tiled fp32-MFMA pair): dqkv of every image bitwise its first occurrence's, the 11 distinct ones within 1e-5 of float64 autograd
    (dq, dk and dv each on its own scale) and bitwise the N = 11 launch, run to run, nothing unwritten."""
    from diamond_amd import engine as E, grad_ops as G

    for key in ("DIAMOND_ATTN_BWD_MIN_T", "DIAMOND_ATTN_PRECISION", "DIAMOND_ATTN_F32_MIN_T", "DIAMOND_ATTN_F16X2_MIN_T"):
        monkeypatch.delenv(key, raising=False)
    n, c, t = ATT_N, ATT_C, side * side
    mfma = t >= G.attn_bwd_mfma_min_t()
    assert mfma == (side == 32)
    where = f" (N={n}, T={t}, {'dmd_attention_bwd_mfma' if mfma else 'dmd_attention_bwd'})"
    g = torch.Generator(device=DEV).manual_seed(t)
    qkv_d = torch.randn(P, side, side, 3 * c, device=DEV, generator=g) * 1.5
    dy_d = torch.randn(P, side, side, c, device=DEV, generator=g)

    def run(qkv, dy, poison=False):
        a = E.Act(qkv)
        rec = E.AttnRecord(a, E.attention(a, c), c, 8)
        launch = lambda: G.attention_bwd(rec, dy)
        return launch_over_poison(launch, tuple(qkv.shape)) if poison else launch()

    qkv, dy = periodic(qkv_d, n), periodic(dy_d, n)
    dqkv, keys = launch_keys(lambda: run(qkv, dy, poison=True))
    torch.cuda.synchronize()
    assert ("dmd_attention_bwd_mfma" in keys) == mfma and ("dmd_attention_bwd" in keys) == (not mfma), keys
    assert_finite("dqkv", dqkv)
    assert_copies("dqkv", dqkv, where)
    want = attention_bwd_ref64(qkv_d.reshape(P, t, 3 * c), dy_d.reshape(P, t, c)).reshape(P, side, side, 3 * c)
    for i, key in enumerate(("dq", "dk", "dv")):
        err = rel_err(dqkv[:P, ..., i * c:(i + 1) * c], want[..., i * c:(i + 1) * c])
        print(f"attention backward{where}: {key} rel err vs fp64 on the {P} distinct images: {err:.3e}")
        assert err < 1e-5, f"{key}: {err:.3e}{where}"
    small = run(qkv_d, dy_d)
    assert_same_bits(f"dqkv: N={n} against the N={P} launch", dqkv[:P], small, where)
    again = run(qkv, dy)
    assert_same_bits("dqkv: run to run", dqkv, again, where)


# ------------------------------------------------------------------------------------------------------------
# E. model level, B = 267: the only way to lowres_chain_kernel and the head conv at production batch
# ------------------------------------------------------------------------------------------------------------
MODEL_B = 267


def test_denoiser_every_env():
    """Denoiser.compute_model_output at B = 267 on periodic (x, obs, act) and one sigma: the output of every env is bitwise its
    first copy's, and the 8x8 level ran as lowres_chain_kernel."""
    from diamond_amd.testing import synthetic_actions, synthetic_frames
    from oracle import diamond_oracle as O

    ag = _agent()
    g = torch.Generator().manual_seed(267)
    b = MODEL_B
    obs = periodic(synthetic_frames(g, P, 12, 64, 64), b).to(DEV)
    act = periodic(synthetic_actions(g, 4, P, 4), b).to(DEV)
    sigma = O.build_sigmas(O.SamplerSpec())[2]
    x = periodic(torch.randn(P, 3, 64, 64, generator=g), b).to(DEV) * float(sigma) + obs[:, -3:] * 0.5
    f, keys = launch_keys(lambda: ag.denoiser.compute_model_output(x, obs, act, sigma))
    torch.cuda.synchronize()
    assert "lowres_chain_kernel" in keys, keys
    assert any(k.startswith("conv_f16ws_kernel") for k in keys), keys
    assert tuple(f.shape) == (b, 3, 64, 64)
    assert_finite("model output", f)
    assert_copies("Denoiser.compute_model_output", f, f" (B={b})")
    again = ag.denoiser.compute_model_output(x, obs, act, sigma)
    assert_same_bits("Denoiser.compute_model_output: run to run", f, again, f" (B={b})")


def test_rew_end_every_env():
    """RewEndModel.predict_rew_end at B = 267, T = 1 on periodic (obs, act, next_obs): logits and LSTM state of every env bitwise
    their first copy's, and the encoder's 8x8 tail ran as dmd_lowres_chain32."""
    from diamond_amd.testing import synthetic_actions, synthetic_frames

    ag = _agent()
    g = torch.Generator().manual_seed(268)
    b = MODEL_B
    obs = periodic(synthetic_frames(g, P, 2, 3, 64, 64), b).to(DEV)
    act = periodic(synthetic_actions(g, 4, P, 1), b).to(DEV)
    m = ag.rew_end_model
    (lr, le, (hx, cx)), keys = launch_keys(lambda: m.predict_rew_end(obs[:, :1], act, obs[:, 1:]))
    torch.cuda.synchronize()
    assert "dmd_lowres_chain32" in keys, keys
    lr2, le2, (hx2, cx2) = m.predict_rew_end(obs[:, :1], act, obs[:, 1:])
    for key, t, t2 in (("logits_rew", lr, lr2), ("logits_end", le, le2), ("hx", hx[0], hx2[0]), ("cx", cx[0], cx2[0])):
        assert t.shape[0] == b, (key, t.shape)
        assert_finite(key, t)
        assert_copies(f"predict_rew_end {key}", t, f" (B={b})")
        assert_same_bits(f"predict_rew_end {key}: run to run", t, t2, f" (B={b})")
