"""Host-side op layer of the hand-written backward passes: one Python call per backward kernel launch, the counterpart of
engine.py for the forward.  Its two callers are the actor-critic encoder's autograd.Function (ac_native.py) and the recorded-tape
backward of the U-Net and the reward / end encoder (unet_train.py):

  maxpool_bwd     dmd_maxpool2_bwd
  wgrad           dmd_conv2d_wgrad (dW, db; reduced at once, or left to a WgradBatch: dmd_wgrad_reduce_jobs)
  dgrad_weights   the packed weights of the data gradient, which is dmd_conv2d (engine.conv2d) on the flipped / transposed weight
  dgrad_input     dmd_conv2d_dgrad_input (the data gradient of a network's FIRST convolution as cropped NCHW image gradients; launched
                  only where autograd asks for an image gradient)
  gn_bwd          dmd_gn_silu_bwd (GroupNorm + FiLM / affine + SiLU or identity)
  pow2_scaled     the 2^k scaling both backward passes run under
  attention_bwd   dmd_attention_bwd / _bwd_valid (one scalar pair of kernels) or, for long token grids, dmd_attention_bwd_mfma
  rew_end_loss    dmd_rew_end_loss (the reward / end model's two cross-entropies, their gradient and confusion matrices: one launch)

Plumbing only, like engine.py; the arithmetic ("f16x2" / "f32") is its callers' choice and arrives as an argument.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import engine as E
from . import native as nv
from .engine import Act, AttnRecord, NormSpec

# Attention backward: from this many VALID tokens on, the tiled fp32-MFMA kernels (dmd_attention_bwd_mfma) instead of the one-thread-
# per-token pair.  Measured (profiles/attention_bwd_mfma.json); the 256 .. 1023 token range stays on the scalar pair, whose launch
# sequence and bits the default 64x64 step is pinned to.  DIAMOND_ATTN_BWD_MIN_T=n overrides it (read at every backward), 0 = never.
# (Both names are re-exported by unet_train.)
ATTN_BWD_MFMA_MIN_T = 1024


def attn_bwd_mfma_min_t() -> int:
    v = os.environ.get("DIAMOND_ATTN_BWD_MIN_T")
    return ATTN_BWD_MFMA_MIN_T if v is None or v == "" else int(v)


def pow2_scaled(d: Tensor) -> Tuple[Tensor, Tensor]:
    """(d * 2^k, 2^-k), k chosen on the device so that the largest entry of d * 2^k is O(1).  A backward pass is linear in the
    gradient it starts from, so it runs on the scaled one and its results are scaled back: exact in fp32, and it keeps the
    split-fp16 operands (absolute error floor 2^-25, dmd_conv_f16ws.hip) far above their floor however small the loss scale is --
    with loss = mean over B*T the raw gradients are ~1e-6.  ONE scalar serves the whole batch and every channel: an output
    channel whose gradient is below 2^-3 of the largest entry still meets the per-channel floor of the split-fp16 weight gradient
    (its row of dW carries the absolute 2^-25 of its operands: include/diamond_hip.h at dmd_wgrad_params.precision has the table)."""
    d = d.detach().float()
    amax = d.abs().amax()
    k = torch.where(amax > 0, torch.floor(-torch.log2(amax.clamp_min(1e-37))), torch.zeros_like(amax)).clamp(-120, 120)
    return d * torch.exp2(k), torch.exp2(-k)


def dgrad_weights(cache: E.PackCache, conv: nn.Conv2d, c0: int, c1: int, cin_pad_to: int = 0,
                  f16x2: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """Packed weights of the transposed convolution restricted to input channels [c0, c1) of `conv`:
    w_t[ci - c0][co][ky][kx] = w[co][ci][K-1-ky][K-1-kx], co zero-padded to `cin_pad_to` (conv_out: 3 -> 16).  (packed fp32,
    split-fp16 pieces); the latter where the caller asks for them (f16x2) and the shape is covered, else None."""
    wp = cache.dgrad_weight(conv, c0, c1, cin_pad_to)
    w16 = None
    if f16x2 and E.f16x2_weight_shape(c1 - c0, cin_pad_to or conv.out_channels, conv.kernel_size[0]):
        w16 = cache.dgrad_weight(conv, c0, c1, cin_pad_to, f16x2=True)
    return wp, w16


def maxpool_bwd(dp: Tensor, arg: Tensor) -> Tensor:
    n, ho, wo, c = dp.shape
    dx = torch.empty(n, ho * 2, wo * 2, c, device=dp.device, dtype=torch.float32)
    nv.check(nv.lib().dmd_maxpool2_bwd(nv.fptr(dp), nv.ptr(arg), nv.fptr(dx), n, ho * 2, wo * 2, c, nv.stream()), "dmd_maxpool2_bwd")
    return dx


class WgradBatch:
    """Weight gradients whose reductions wait for ONE launch per 32 of them (`dmd_wgrad_reduce_jobs`, ABI v10): the backward of a
    denoiser training step holds ~60 weight gradients nobody reads before it is over, and their reductions were ~140 launches
    of a few microseconds of work.  The sums are formed in the undeferred order: bit-identical gradients.

    scale (a one-element fp32 DEVICE tensor, or None): every gradient of the batch leaves the launch multiplied by it -- the 2^-k
    of a backward that ran under pow2_scaled: bitwise the reduction followed by a multiplication pass, without the pass.
    add_colsum: the GroupNorm parameter gradients of a block ride in the same launch (DMD_REDUCE_COLSUM)."""

    def __init__(self, scale: Optional[Tensor] = None) -> None:
        self.jobs: List[nv.WgradReduceJob] = []
        self._keep: List[Tensor] = []  # the workspaces holding the partials (and the outputs) until flush()
        self.scale = scale
        if scale is not None:
            assert scale.numel() == 1 and scale.dtype == torch.float32
            self._keep.append(scale)

    def add(self, job: "nv.WgradReduceJob", *keep: Tensor) -> None:
        if self.scale is not None:
            job.scale = nv.ptr(self.scale)
        self.jobs.append(job)
        self._keep.extend(keep)

    def add_colsum(self, dma: Tensor, dgamma: Tensor, dbeta: Tensor) -> None:
        """dgamma[c] = sum_n dma[0, n, c], dbeta[c] = sum_n dma[1, n, c] (dma: gn_bwd's (2, N, C)): ascending n, fp64 accumulation,
        one rounding to fp32 (then the batch's scale).  Deterministic; not torch's reduction order."""
        two, n, c = dma.shape
        assert two == 2 and dma.is_contiguous() and dma.dtype == torch.float32 and dgamma.numel() == dbeta.numel() == c \
            and dgamma.is_contiguous() and dbeta.is_contiguous()
        job = nv.WgradReduceJob()
        job.kind, job.partials, job.dw, job.dbias, job.num_wg, job.cin_real = nv.REDUCE_COLSUM, nv.ptr(dma), nv.ptr(dgamma), nv.ptr(dbeta), n, c
        self.add(job, dma, dgamma, dbeta)

    def flush(self) -> None:
        if self.jobs:
            table = (nv.WgradReduceJob * len(self.jobs))(*self.jobs)
            nv.check(nv.lib().dmd_wgrad_reduce_jobs(table, len(self.jobs), nv.stream()), "dmd_wgrad_reduce_jobs")
        self.jobs, self._keep = [], []


def wgrad_batch(scale: Optional[Tensor] = None) -> Optional[WgradBatch]:
    """The batch a backward pass defers its weight-gradient reductions to; DIAMOND_WGRAD_DEFER=0: None, every gradient is
    reduced by its own call (same sums).  scale: see WgradBatch."""
    return WgradBatch(scale) if os.environ.get("DIAMOND_WGRAD_DEFER", "1") == "1" else None


# (output channels / 16, input channels / 16) the weight-gradient kernel is instantiated for (csrc/dmd_backward.hip:
# dmd_conv2d_wgrad's dispatch): the shapes of the default configuration's networks
_WGRAD_INSTANCES = {9: {(2, 1), (4, 1), (1, 4), (2, 2), (4, 2), (4, 4)}, 1: {(4, 2), (2, 2), (4, 4)}}


def _wgrad_instance(cout: int, cin: int, taps: int) -> bool:
    return cout % 16 == 0 and cin % 16 == 0 and (cout // 16, cin // 16) in _WGRAD_INSTANCES[taps]


def _pad_channels(t: Tensor, c0: int, c1: int, to: int) -> Tensor:
    """Channels [c0, c1) of an NHWC tensor as a contiguous tensor of `to` channels (zeros behind the slice)."""
    if c1 - c0 == to:
        return t[..., c0:c1].contiguous()
    out = torch.zeros(t.shape[:-1] + (to,), device=t.device, dtype=t.dtype)
    out[..., :c1 - c0] = t[..., c0:c1]
    return out


def _norm_slice(x: Act, spec: NormSpec, c0: int, c1: int, to: int) -> Tuple[Tensor, int, NormSpec]:
    """Statistics and multiplicative / additive parameters of channels [c0, c1) of a normalised source, zero-padded to `to`
    channels: (partial sums, tiles, spec).  A padded group has sums 0 and parameters 0: its activated value is 0.  Groups of another
    size than 32 (one group per slice: the general-group kernel instances) carry no padded groups -- the kernel normalises the
    slice's real channels only."""
    g = E.gn_group_size(x.C)
    assert c0 % g == 0 and (c1 - c0) % g == 0 and to % nv.GN_GROUP == 0 and x.stats is not None, \
        f"normalised source of {x.C} channels cut at [{c0}, {c1}): not whole GroupNorm groups"
    assert g == nv.GN_GROUP or c1 - c0 == g, f"a slice of {c1 - c0} channels of a source in {g}-channel groups: one group per slice"
    stats = x.stats[:, c0 // g:c1 // g]
    if to != c1 - c0 and g == nv.GN_GROUP:
        stats = torch.cat([stats, torch.zeros(stats.shape[0], (to - (c1 - c0)) // g, *stats.shape[2:], device=stats.device, dtype=stats.dtype)], 1)

    def cut(t: Optional[Tensor], stride: int):
        if t is None:
            return None, 0
        rows = t if t.ndim == 2 else t[None]
        rows = rows[:, c0:c1] if stride != 0 else rows[:1, c0:c1]
        out = torch.zeros(rows.shape[0], to, device=t.device, dtype=torch.float32)
        out[:, :c1 - c0] = rows
        return out, (to if stride != 0 else 0)

    mul, ms = cut(spec.mul, spec.mul_stride)
    add, as_ = cut(spec.add, spec.add_stride)
    return stats.contiguous(), x.tiles, NormSpec(mul, add, ms, as_, spec.plus_one)


def _wgrad_tiled(x: Act, prologue: int, spec: Optional[NormSpec], dy: Tensor, taps: int, cin_real: int, want_bias: bool, split: bool,
                 batch: Optional["WgradBatch"], dw_out: Optional[Tensor], c0: int, db_out: Optional[Tensor]):
    """Weight gradient of a convolution the kernel has no instance for (networks wider or narrower than the default
    configuration's 32 / 64 channels: the reference takes any `channels` list, blocks.py:183-222, actor_critic.py:101-113): the
    gradient of output-channel block i w.r.t. input-channel block j depends on those two blocks only, so the (Cout, Cin) plane is
    tiled with the 64 x 64 instance on contiguous, zero-padded channel slices (whole GroupNorm groups of a normalised source,
    with their partial sums and parameters).  Reduced per tile (nothing deferred): the correct path for such shapes, not a fast one."""
    n, h, w, cout = dy.shape
    k = 3 if taps == 9 else 1
    T = 64
    # a normalised source in groups other than 32 channels: one group per tile (its real channels; dmd_conv2d_wgrad picks the
    # general-group instance), zero-padded to the 64 -> 64 shape like every other tile
    step = E.gn_group_size(x.C) if prologue != nv.PROLOGUE_NONE and x.C % nv.GN_GROUP != 0 else T
    if batch is not None:
        dw, db = dw_out, db_out
    else:
        dw = torch.empty(cout, cin_real, k, k, device=dy.device, dtype=torch.float32)
        db = torch.empty(cout, device=dy.device, dtype=torch.float32) if want_bias else None
        c0 = 0
    for ci0 in range(0, cin_real, step):
        ci1 = min(cin_real, ci0 + step)
        cw = (ci1 - ci0 + 15) // 16 * 16  # (the source's own padding: conv_in's 15 channels travel as 16)
        if prologue == nv.PROLOGUE_NONE:
            xt, spec_t = Act(_pad_channels(x.t, ci0, min(x.C, ci0 + cw), T), valid=x.valid), None
        else:
            stats, tiles, spec_t = _norm_slice(x, spec, ci0, ci1, T)
            xt = Act(_pad_channels(x.t, ci0, ci1, T), stats, tiles, valid=x.valid)
        for co0 in range(0, cout, T):
            co1 = min(cout, co0 + T)
            dw_t, db_t = wgrad(xt, prologue, spec_t, _pad_channels(dy, co0, co1, T), taps, ci1 - ci0,
                               want_bias=db is not None and ci0 == 0, split=split)
            dw[co0:co1, c0 + ci0:c0 + ci1] = dw_t[:co1 - co0]
            if db is not None and ci0 == 0:
                db[co0:co1] = db_t[:co1 - co0]
    return dw, db


def wgrad(x: Act, prologue: int, spec: Optional[NormSpec], dy: Tensor, taps: int, cin_real: int,
          want_bias: bool = True, split: bool = False, batch: Optional[WgradBatch] = None, dw_out: Optional[Tensor] = None,
          c0: int = 0, db_out: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """dW, db of a convolution.  split: operands as split-fp16 pairs (needs dy pre-scaled to O(1): pow2_scaled);
    False: exact fp32 fma chain.  batch: the reduction of the partial sums is left to batch.flush(); then dw_out (rows of a
    contiguous OIHW tensor whose input-channel extent may be wider than this source: the gradient lands in channels
    [c0, c0 + cin_real)) and db_out (or None) name where the gradient goes."""
    n, h, w, cout = dy.shape
    k = 3 if taps == 9 else 1
    if not _wgrad_instance(cout, x.C, taps):  # (never at the default configuration)
        return _wgrad_tiled(x, prologue, spec, dy, taps, cin_real, want_bias, split, batch, dw_out, c0, db_out)
    p = nv.WgradParams()
    p.N, p.H, p.W, p.Cout, p.taps, p.cin_real = n, h, w, cout, taps, cin_real
    assert x.t.is_contiguous() and dy.is_contiguous() and tuple(x.shape[:3]) == (n, h, w)
    p.src.x = nv.ptr(x.t)
    p.src.C = x.C
    p.src.prologue = prologue
    if prologue != nv.PROLOGUE_NONE:
        p.src.norm = spec.to_native(x)
    if x.valid is not None:
        p.valid_h, p.valid_w = x.valid
    p.dy = nv.ptr(dy)
    p.precision = nv.PRECISION_F16X2 if split else nv.PRECISION_F32
    if nv.PROFILER is not None:  # (algorithmic work of a weight gradient: the forward conv's MACs; x and dy read once)
        def note():
            # (spelled like rocprofv3's kernel trace: bench.py's records and profiles/*pmc*.json share one key)
            # (the split-fp16 gradient runs on the producer / consumer kernel, csrc/dmd_backward.hip)
            geom = f"WgradGeom<{cout // 16}, {x.C // 16}, {taps}>"
            nv.PROFILER.annotate(f"wgrad_ps_kernel<{geom}, {'true' if prologue else 'false'}>" if split and os.environ.get("DIAMOND_WGRAD_PS", "1") != "0" else
                                 f"wgrad_kernel<{geom}, {'true' if split else 'false'}>",
                                 2.0 * taps * cin_real * cout * n * h * w, 4.0 * n * h * w * (x.C + cout))
    else:
        note = lambda: None
    if batch is not None:
        assert dw_out is not None and dw_out.is_contiguous() and dw_out.shape[0] >= cout and tuple(dw_out.shape[2:]) == (k, k) \
            and c0 + cin_real <= dw_out.shape[1] and (db_out is None or (db_out.is_contiguous() and db_out.numel() >= cout))
        p.dw, p.dbias, p.defer_reduce = nv.ptr(dw_out), nv.ptr(db_out), 1
        job = nv.WgradReduceJob()
        nv.check(nv.lib().dmd_wgrad_job(C.byref(p), C.byref(job)), "dmd_wgrad_job")
        # (the partials only, and they stay alive until the flush: the plan's workgroups, not the 1024 the query sizes for)
        ws = torch.empty(job.num_wg * (job.NB * job.NCO * 256 + job.NCO * 16), device=dy.device, dtype=torch.float32)
        p.workspace = job.partials = nv.ptr(ws)
        job.ld_cin, job.c0 = dw_out.shape[1], c0
        note()
        nv.check(nv.lib().dmd_conv2d_wgrad(C.byref(p), nv.stream()), "dmd_conv2d_wgrad")
        batch.add(job, ws, dw_out) if db_out is None else batch.add(job, ws, dw_out, db_out)
        return dw_out, db_out
    ws = torch.empty(int(nv.lib().dmd_wgrad_workspace_floats(C.byref(p))), device=dy.device, dtype=torch.float32)
    dw = torch.empty(cout, cin_real, k, k, device=dy.device, dtype=torch.float32)
    db = torch.empty(cout, device=dy.device, dtype=torch.float32) if want_bias else None
    p.workspace, p.dw, p.dbias = nv.ptr(ws), nv.ptr(dw), nv.ptr(db)
    note()
    nv.check(nv.lib().dmd_conv2d_wgrad(C.byref(p), nv.stream()), "dmd_conv2d_wgrad")
    return dw, db


def dgrad_input(dy: Act, conv: nn.Conv2d, c_split: int, want_a: bool = True, want_b: bool = True, scale_a: Optional[Tensor] = None,
                scale_b: float = 1.0, post: Optional[Tensor] = None, swap_scales: bool = False) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """Image gradients behind a network's first convolution (dmd_conv2d_dgrad_input, ONE launch): dy = the gradient of conv's
    output (NHWC, its valid extent), -> (dx_a (N, c_split, vh, vw), dx_b (N, cin - c_split, vh, vw)), NCHW and cropped to the
    extent; None for the one not wanted.  dx = (sum * post) * s: post = the one-element 2^-k of a backward that ran under
    pow2_scaled; s = scale_a[n] (a one- or N-element device tensor) for dx_a and the float scale_b for dx_b -- the other way round
    with swap_scales.  Reads conv.weight itself (OIHW): no packed copy, nothing for the audit.  Exact fp32 in both precisions."""
    n, h, w, cout = dy.shape
    vh, vw = dy.valid if dy.valid is not None else (h, w)
    cin = conv.in_channels
    assert conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.out_channels == cout, conv
    assert 0 <= c_split <= cin and (want_a or want_b) and dy.t.is_contiguous() and dy.t.dtype == torch.float32
    wt = conv.weight.detach()
    if wt.dtype != torch.float32 or not wt.is_contiguous():
        wt = wt.float().contiguous()
    dev = dy.t.device
    dx_a = torch.empty(n, c_split, vh, vw, device=dev, dtype=torch.float32) if want_a else None
    dx_b = torch.empty(n, cin - c_split, vh, vw, device=dev, dtype=torch.float32) if want_b else None
    p = nv.DgradInputParams()
    p.N, p.H, p.W, p.valid_h, p.valid_w, p.Cout, p.cin, p.c_split = n, h, w, vh, vw, cout, cin, c_split
    p.dy, p.w, p.dx_a, p.dx_b = nv.ptr(dy.t), nv.fptr(wt), nv.fptr(dx_a), nv.fptr(dx_b)
    if scale_a is not None:
        assert scale_a.numel() in (1, n) and scale_a.dtype == torch.float32 and scale_a.is_contiguous(), (scale_a.shape, scale_a.dtype)
        p.scale_a, p.stride_a = nv.ptr(scale_a), int(scale_a.numel() == n and n > 1)
    p.scale_b = float(scale_b)
    if post is not None:
        assert post.numel() == 1 and post.dtype == torch.float32
        p.post = nv.ptr(post)
    p.swap_scales = int(swap_scales)
    if nv.PROFILER is not None:  # (the forward convolution's MACs; dy read once, the image gradients written)
        nv.PROFILER.annotate("dgrad_input_kernel", 2.0 * 9 * cin * cout * n * vh * vw, 4.0 * n * (h * w * cout + vh * vw * cin))
    nv.check(nv.lib().dmd_conv2d_dgrad_input(C.byref(p), nv.stream()), "dmd_conv2d_dgrad_input")
    return dx_a, dx_b


def _gn_bwd_instance(c: int) -> bool:
    """channel counts dmd_gn_silu_bwd takes (csrc/dmd_backward.hip): 4 ... 256 in powers of two, and the general groups (the
    grouping rule's widths that are not multiples of 32: 48, 80, 144 ...; one workgroup per image)"""
    if c % nv.GN_GROUP != 0 and c > nv.GN_GROUP:
        return c <= 256 and E.gn_width_ok(c)
    return c % 4 == 0 and c <= 256 and 256 % (c // 4) == 0 and (c % nv.GN_GROUP == 0 or c < nv.GN_GROUP)


def gn_bwd_sliced(x: Act, spec: NormSpec, da: Tensor, dskip: Optional[Tensor], identity: bool) -> Tuple[Tensor, Tensor]:
    """GroupNorm backward over a channel count the kernel has no instance for (96, 160, 512 ...: networks wider than the default
    configuration): a group's backward involves its own 32 channels only, so the channels are cut into 256 / 128 / 64 / 32-wide
    runs of whole groups and gn_bwd runs on contiguous copies of each."""
    n, h, w, c = x.shape
    g = nv.GN_GROUP
    assert c % g == 0, f"GroupNorm backward over {c} channels"
    dx = torch.empty_like(x.t)
    dma = torch.empty(2, n, c, device=da.device, dtype=torch.float32)
    c0 = 0
    while c0 < c:
        step = next(s for s in (256, 128, 64, 32) if s <= c - c0)
        c1 = c0 + step
        cut = lambda t: None if t is None else t[..., c0:]
        xs = Act(x.t[..., c0:c1].contiguous(), x.stats[:, c0 // g:c1 // g].contiguous(), x.tiles, valid=x.valid)
        spec_s = NormSpec(cut(spec.mul), cut(spec.add), spec.mul_stride, spec.add_stride, spec.plus_one)
        dx_s, dma_s = gn_bwd(xs, spec_s, da[..., c0:c1].contiguous(), None if dskip is None else dskip[..., c0:c1].contiguous(), identity)
        dx[..., c0:c1] = dx_s
        dma[0, :, c0:c1] = dma_s[0]
        dma[1, :, c0:c1] = dma_s[1]
        c0 = c1
    return dx, dma


def gn_bwd(x: Act, spec: NormSpec, da: Tensor, dskip: Optional[Tensor], identity: bool = False) -> Tuple[Tensor, Tensor]:
    """Backward of the fused prologue act(GroupNorm(x) * mul + add), act = SiLU, or the identity with `identity`: (dx, dma).  da:
    gradient of the activated value; dskip (or None): a gradient that reaches x directly, added into dx.  dma (2, N, C) stacks
    the per-(sample, channel) gradients [dmul; dadd]: a caller that only needs their sums over the batch reduces both with one
    launch (dma.sum(1): the same per-column order as dmul.sum(0) and dadd.sum(0))."""
    n, h, w, c = x.shape
    if not _gn_bwd_instance(c):  # (never at the default configuration)
        return gn_bwd_sliced(x, spec, da, dskip, identity)
    p = nv.GnBwdParams()
    p.N, p.HW, p.C = n, h * w, c
    if x.valid is not None:  # sums and the count over the valid extent, dx zero outside it
        p.W, p.valid_h, p.valid_w = w, x.valid[0], x.valid[1]
    p.identity_activation = int(identity)
    p.x = nv.ptr(x.t)
    p.norm = spec.to_native(x)
    p.da = nv.fptr(da)
    p.dskip = nv.fptr(dskip)
    dx = torch.empty_like(x.t)
    ws = torch.empty(int(nv.lib().dmd_gn_bwd_workspace_bytes(n, h * w, c)), device=da.device, dtype=torch.uint8)
    dma = torch.empty(2, n, c, device=da.device, dtype=torch.float32)
    dmul, dadd = dma[0], dma[1]
    p.dx, p.workspace, p.dmul, p.dadd = nv.ptr(dx), nv.ptr(ws), nv.ptr(dmul), nv.ptr(dadd)
    if nv.PROFILER is not None:  # (HBM-bound: x and da read, dx written, the skip gradient read when there is one)
        nv.PROFILER.annotate("dmd_gn_silu_bwd", 0.0, 4.0 * x.t.numel() * (3 + (dskip is not None)))
    nv.check(nv.lib().dmd_gn_silu_bwd(C.byref(p), nv.stream()), "dmd_gn_silu_bwd")
    return dx, dma


def attention_bwd(rec: AttnRecord, dy: Tensor) -> Tensor:
    """dqkv of a recorded attention launch from dy, the gradient of its output; zero outside the valid extent"""
    n, h, w, _ = rec.qkv.shape
    gh, gw, vh, vw = rec.extent
    dqkv = torch.empty_like(rec.qkv.t)
    ws = torch.empty(int(nv.lib().dmd_attention_bwd_workspace_floats(n, h * w, rec.c)), device=dy.device, dtype=torch.float32)
    dyc = dy.contiguous()
    ptrs = (nv.fptr(rec.qkv.t), nv.fptr(rec.out), nv.fptr(dyc), nv.fptr(dqkv), nv.fptr(ws))
    if 0 < attn_bwd_mfma_min_t() <= vh * vw:  # long token grids: tiled fp32 MFMA kernels
        nv.check_current_device(dy.device)
        if nv.PROFILER is not None:  # 7 contractions of 8 MACs per (query, key) pair and head
            nv.PROFILER.annotate("dmd_attention_bwd_mfma", 14.0 * n * (vh * vw) ** 2 * rec.c, 4.0 * n * vh * vw * 8 * rec.c)
        name, args = "dmd_attention_bwd_mfma", (n, gh, gw, vh, vw)
    elif rec.valid is not None:  # queries and keys of the valid extent only
        name, args = "dmd_attention_bwd_valid", (n, gh, gw, vh, vw)
    else:  # the same pair of kernels over the whole grid
        name, args = "dmd_attention_bwd", (n, h * w)
    nv.check(getattr(nv.lib(), name)(*ptrs, *args, rec.c, rec.head_dim, nv.stream()), name)
    return dqkv


class RewEndLossFn(torch.autograd.Function):
    """dmd_rew_end_loss under autograd: the kernel leaves d(loss_rew + loss_end) / dlogits beside the losses, the backward scales
    its reward columns by the gradient that reaches loss_rew and its end columns by the one that reaches loss_end."""

    @staticmethod
    def forward(ctx, logits: Tensor, rew: Tensor, end: Tensor, mask: Tensor):
        lg = logits.detach().float().contiguous()
        r = lg.shape[0]
        assert lg.shape == (r, 5) and rew.numel() == end.numel() == mask.numel() == r, (lg.shape, rew.shape, end.shape, mask.shape)
        rw = rew.detach().float().contiguous()
        en = end.detach().long().contiguous()
        mk = mask.detach().contiguous()
        assert mk.element_size() == 1, f"mask of dtype {mk.dtype}: one byte per row (bool or uint8)"
        losses = torch.empty(2, device=lg.device, dtype=torch.float32)
        counts = torch.empty(13, device=lg.device, dtype=torch.int64)
        dlogits = torch.empty_like(lg)
        nv.check(nv.lib().dmd_rew_end_loss(nv.fptr(lg), nv.fptr(rw), nv.ptr(en), nv.ptr(mk), nv.fptr(losses), nv.fptr(dlogits), nv.ptr(counts),
                                           r, nv.stream()), "dmd_rew_end_loss")
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(counts)
        return losses, counts

    @staticmethod
    def backward(ctx, dlosses: Tensor, _dcounts):
        (dlogits,) = ctx.saved_tensors
        d = dlosses.detach().float()
        return dlogits * torch.stack((d[0], d[0], d[0], d[1], d[1])), None, None, None


def rew_end_loss(logits: Tensor, rew: Tensor, end: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
    """(losses (2,) = [loss_rew, loss_end], counts (13,) int64 = the 3 x 3 reward and the 2 x 2 end confusion matrix) of logits
    (R, 5) against rew / end (R) over the rows where mask (R; bool or uint8) holds: the masked means of reference
    rew_end_model.py:72-88 with no gather and no host round trip (an all-false mask gives NaN losses and no gradient, like the
    mean of an empty selection)."""
    nv.require_gpu(logits)
    return RewEndLossFn.apply(logits, rew.reshape(-1), end.reshape(-1), mask.reshape(-1))
