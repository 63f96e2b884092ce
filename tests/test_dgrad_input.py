"""dmd_conv2d_dgrad_input: the data gradient of a network's first 3x3 convolution, written as cropped NCHW image gradients -- on
the SIMT interpreter (the kernel's own source, inputs in fenced arrays: an out-of-bounds access fails there) and on the device
(-m gpu).  Both outputs start as NaN in every test, so an element the kernel does not write shows.

Reference: float64 conv_transpose2d of dy with its margins zeroed.  Precision: the kernel's error, relative to max |want|, is held
to K_DGRAD x the error of float32 CPU conv_transpose2d on the same inputs.  K_DGRAD = twice the largest ratio measured on the
MI355X over the cases below (profiles/dgrad_input_precision.txt has the table, written by tools/dgrad_input_bench.py): 2 x 3.30
(16x16 valid 9x11, Cout = 48, cin = 3; the ratios run from 1.23 to 3.30).  Both sides are fp32 sums of the same 9 Cout products:
the kernel adds them one after the other into one accumulator, the CPU library in blocks, hence a ratio above 1.  The
interpreter's MFMA model forms the same chain and gives the same figures.
Shapes: N = 3; one tile (8x8), a full 16x16 buffer (two row bands), 16x16 with the valid extent 9x11 (partial band, partial
tile, margins); Cout 32 / 48 / 64 (a chunk that is not full, 48 = no multiple of 32); cin / c_split 3/3 (dx_b absent), 6/3,
15/3 (one channel of the group unused), 27/3 (two channel groups)."""
import ctypes
import functools
import os
from types import SimpleNamespace

import pytest
import torch

from tests import abi

K_DGRAD = 6.60  # 2 x 3.30, profiles/dgrad_input_precision.txt

N = 3
BUFFERS = [(8, 8, None), (16, 16, None), (16, 16, (9, 11))]
COUTS = [32, 48, 64]
CHANNELS = [(3, 3), (6, 3), (15, 3), (27, 3)]


# ---- inputs and the reference ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(h, w, valid, cout, cin, n=N, margin=float("nan")):
    """(dy with its margins filled with `margin`, w, float64 reference cropped to the extent, float32 CPU reference)"""
    g = torch.Generator().manual_seed(1000 * h + 100 * (valid[0] if valid else 0) + cout + cin)
    dy = torch.randn(n, h, w, cout, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.3
    vh, vw = valid or (h, w)
    inside = torch.zeros(h, w, dtype=torch.bool)
    inside[:vh, :vw] = True
    clean = torch.where(inside[None, :, :, None], dy, torch.zeros(()))
    dy = torch.where(inside[None, :, :, None], dy, torch.full((), margin))
    want = torch.nn.functional.conv_transpose2d(clean.permute(0, 3, 1, 2).double(), wt.double(), padding=1)[:, :, :vh, :vw].contiguous()
    f32 = torch.nn.functional.conv_transpose2d(clean.permute(0, 3, 1, 2).contiguous(), wt, padding=1)[:, :, :vh, :vw].contiguous()
    return dy.contiguous(), wt, want, f32


def _arm(run):
    """`run` is tests/abi.py's dgrad_input with tensors for its arrays; rc=True: (status, message) of a refused launch"""
    def launch(*args, rc=False, **kw):
        got = abi.dgrad_input(run, *args, status=rc, **kw)
        return got[:2] if rc else tuple(None if a is None else torch.from_numpy(a) for a in got)

    return SimpleNamespace(name=run.name, run=launch)


SIMT, GPU = _arm(abi.Simt), _arm(abi.Gpu)
BOTH = abi.arms(SIMT, GPU)
arms = functools.partial(abi.arms, SIMT, GPU)



def joined(dx_a, dx_b):
    return torch.cat([t for t in (dx_a, dx_b) if t is not None], dim=1)


def rel_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


# ---- against float64 ---------------------------------------------------------------------------------------------------------------
def measure(arm, h, w, valid, cout, cin, c_split):
    """(the kernel's error, float32 CPU conv_transpose2d's), both relative to max |want|"""
    dy, wt, want, f32 = case(h, w, valid, cout, cin)
    got = joined(*arm.run(dy, wt, cin, c_split, valid))
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    return rel_err(got, want), rel_err(f32, want)


@pytest.mark.parametrize("arm,buf,cout,ch", arms([(b, co, ch) for b in BUFFERS for co in COUTS for ch in CHANNELS]))
def test_within_k_of_float32_conv_transpose(arm, buf, cout, ch):
    h, w, valid = buf
    e, e32 = measure(arm, h, w, valid, cout, *ch)
    print(f"DGRADIN {arm.name} buffer {h}x{w} valid {valid} Cout={cout} cin/c_split={ch}: err {e:.3e} float32 CPU {e32:.3e} ratio {e / e32:.2f}")
    assert e <= K_DGRAD * e32, (e, e32)


# ---- margins, batch independence, repeatability ------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", BOTH)
def test_margins_never_contribute(arm):
    """the same valid data with NaN and with 3e38 in the margins of dy: bitwise the same result"""
    h, w, valid, cout, cin = 16, 16, (9, 11), 48, 15
    dy_nan, wt, _, _ = case(h, w, valid, cout, cin)
    dy_big = case(h, w, valid, cout, cin, margin=3e38)[0]
    assert bool(torch.isnan(dy_nan).any()) and float(dy_big.max()) > 2.9e38
    a, b = joined(*arm.run(dy_nan, wt, cin, 3, valid)), joined(*arm.run(dy_big, wt, cin, 3, valid))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("arm", BOTH)
def test_an_image_alone_is_bitwise_its_result_in_a_batch(arm):
    h, w, valid, cout, cin = 16, 16, (9, 11), 64, 27
    dy, wt, _, _ = case(h, w, valid, cout, cin)
    batch = joined(*arm.run(dy, wt, cin, 3, valid))
    for i in (0, 2):
        alone = joined(*arm.run(dy[i:i + 1].contiguous(), wt, cin, 3, valid))
        assert torch.equal(alone[0], batch[i]), i
    # the same image at position 0 and at position 2 of a batch
    swapped = joined(*arm.run(dy[[2, 1, 0]].contiguous(), wt, cin, 3, valid))
    assert torch.equal(swapped[0], batch[2]) and torch.equal(swapped[2], batch[0])


@pytest.mark.parametrize("arm", BOTH)
def test_two_runs_are_bitwise_equal(arm):
    h, w, valid, cout, cin = 16, 16, None, 64, 15
    dy, wt, _, _ = case(h, w, valid, cout, cin)
    first = joined(*arm.run(dy, wt, cin, 3, valid))
    assert bool(torch.isfinite(first).all()) and torch.equal(first, joined(*arm.run(dy, wt, cin, 3, valid)))


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal_at_the_training_shape():
    """N = 32, 64x64, Cout = 64, 15 channels: 256 workgroups"""
    g = torch.Generator().manual_seed(4)
    dy, wt = torch.randn(32, 64, 64, 64, generator=g), torch.randn(64, 15, 3, 3, generator=g) * 0.3
    first = joined(*GPU.run(dy, wt, 15, 12))
    assert bool(torch.isfinite(first).all()) and torch.equal(first, joined(*GPU.run(dy, wt, 15, 12)))
    want = torch.nn.functional.conv_transpose2d(dy[:2].permute(0, 3, 1, 2).double(), wt.double(), padding=1)
    assert rel_err(first[:2], want) <= 1e-5


# ---- the scale factors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", BOTH)
def test_scale_factors_alone_and_together(arm):
    """dx = (sum * post) * s: every factor against the unscaled result multiplied on the host in that order (exact: one fp32
    product each, the same on both sides)"""
    h, w, valid, cout, cin, cs = 16, 16, (9, 11), 32, 6, 3
    dy, wt, _, _ = case(h, w, valid, cout, cin)
    base_a, base_b = arm.run(dy, wt, cin, cs, valid)
    sa = torch.tensor([0.37, 1.9, -2.5])
    one = torch.tensor([0.81])
    rows = lambda s: s.reshape(-1, 1, 1, 1)
    # scale_a per sample / shared by the batch (stride 0), scale_b, post, all three
    a, b = arm.run(dy, wt, cin, cs, valid, scale_a=sa)
    assert torch.equal(a, base_a * rows(sa)) and torch.equal(b, base_b)
    a, b = arm.run(dy, wt, cin, cs, valid, scale_a=one)
    assert torch.equal(a, base_a * one) and torch.equal(b, base_b)
    a, b = arm.run(dy, wt, cin, cs, valid, scale_b=2.0 ** 0.5)
    assert torch.equal(a, base_a) and torch.equal(b, base_b * torch.tensor(2.0 ** 0.5))
    a, b = arm.run(dy, wt, cin, cs, valid, post=2.0 ** -7)
    assert torch.equal(a, base_a * 2.0 ** -7) and torch.equal(b, base_b * 2.0 ** -7) and float(a.abs().max()) > 0
    a, b = arm.run(dy, wt, cin, cs, valid, scale_a=sa, scale_b=3.1, post=0.3)
    p = torch.tensor(0.3)
    assert torch.equal(a, (base_a * p) * rows(sa)) and torch.equal(b, (base_b * p) * torch.tensor(3.1))
    # swap_scales: the device factor on dx_b's channels, the host factor on dx_a's (the denoiser's pack order)
    a, b = arm.run(dy, wt, cin, cs, valid, scale_a=sa, scale_b=3.1, post=0.3, swap=True)
    assert torch.equal(a, (base_a * p) * torch.tensor(3.1)) and torch.equal(b, (base_b * p) * rows(sa))


@pytest.mark.parametrize("arm", BOTH)
def test_an_output_that_is_not_wanted_is_not_computed_into_the_other(arm):
    h, w, valid, cout, cin = 8, 8, None, 32, 6
    dy, wt, _, _ = case(h, w, valid, cout, cin)
    base_a, base_b = arm.run(dy, wt, cin, 3, valid)
    only_a, none_b = arm.run(dy, wt, cin, 3, valid, want_b=False)
    none_a, only_b = arm.run(dy, wt, cin, 3, valid, want_a=False)
    assert none_a is None and none_b is None and torch.equal(only_a, base_a) and torch.equal(only_b, base_b)


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", BOTH)
def test_refused_arguments(arm):
    g = torch.Generator().manual_seed(2)
    dy24, w24 = torch.randn(1, 8, 8, 24, generator=g), torch.randn(24, 3, 3, 3, generator=g)
    rc, msg = arm.run(dy24, w24, 3, 3, rc=True)
    assert rc != 0 and "multiple of 16" in msg, (rc, msg)
    dy, w65 = torch.randn(1, 8, 8, 16, generator=g), torch.randn(16, 65, 3, 3, generator=g)
    rc, msg = arm.run(dy, w65, 65, 3, rc=True)
    assert rc != 0 and "cin 65" in msg, (rc, msg)
    rc, msg = arm.run(dy, w65[:, :3].contiguous(), 3, 3, valid=(9, 8), rc=True)
    assert rc != 0 and "valid extent" in msg, (rc, msg)
    rc, msg = arm.run(dy, w65[:, :3].contiguous(), 3, 3, valid=(8, 8), rc=True)
    assert rc == 0, msg


# ---- the ctypes mirror -------------------------------------------------------------------------------------------------------------
def test_params_struct_layout_matches_the_header():
    """sizeof and every field offset of native.DgradInputParams against dmd_dgrad_input_params compiled with gcc from
    include/diamond_hip.h (the method of test_boundary.test_struct_layouts_match_the_header)"""
    import subprocess
    import tempfile

    from diamond_amd import native
    from tests.conftest import ROOT

    fields = [f for f, _ in native.DgradInputParams._fields_]
    body = 'printf("%zu ", sizeof(dmd_dgrad_input_params));' + "".join(f'printf("%zu ", offsetof(dmd_dgrad_input_params, {f}));' for f in fields)
    src = f'#include <stdio.h>\n#include <stddef.h>\n#include "diamond_hip.h"\nint main(){{{body}return 0;}}'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    mine = [ctypes.sizeof(native.DgradInputParams)] + [getattr(native.DgradInputParams, f).offset for f in fields]
    assert got == mine, list(zip(["sizeof"] + fields, got, mine))
    assert "dmd_conv2d_dgrad_input" in native.EXPORTS and "dmd_conv2d_dgrad_input" in native.LAUNCHERS
