"""Actor-critic conv encoder on hand-written HIP kernels, forward AND backward
(reference models/actor_critic.py:101-113 `ActorCriticEncoder`, blocks.py:116-123 `SmallResBlock`).

One `torch.autograd.Function` spans the whole encoder: Conv3x3 -> n x [skip(x) +
Conv3x3(SiLU(GroupNorm(x))), MaxPool2] -> flatten.  The forward saves only the block inputs
(with their GroupNorm statistics) and the pooling argmax; the backward recomputes the
activations inside the wgrad kernel's staging pass.  Kernel map:

  forward   dmd_conv2d (GN+SiLU prologue, bias + residual epilogue), dmd_maxpool2 (+ stats of the
            pooled tensor for the next GroupNorm)
  backward  (launched through grad_ops.py) dmd_maxpool2_bwd -> dmd_conv2d_wgrad (dW, db) -> dmd_conv2d on the flipped/transposed
            weight (dgrad) -> dmd_gn_silu_bwd (dx, dgamma, dbeta; adds the skip-branch gradient); where `obs` requires a
            gradient, dmd_conv2d_dgrad_input behind conv_in's weight gradient (the image gradient: one launch, else none)

The LSTM cell and the two heads downstream run on dmd_linear / dmd_lstm_pointwise(_bwd): lstm_native.LstmHeadsFn.
"""
from __future__ import annotations

import os
import weakref
from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import engine as E
from . import grad_ops as G
from . import native as nv
from .engine import Act, NormSpec


def _maxpool(y: Tensor, valid: Optional[Tuple[int, int]] = None) -> Tuple[Act, Tensor]:
    """MaxPool2d(2) (floor: an odd valid extent loses its last row / column, like F.max_pool2d).  valid: the part of the
    buffer that exists; the pooled tensor is the (vh // 2, vw // 2) part of a buffer half the size, and its GroupNorm
    statistics count that part only."""
    n, h, w, c = y.shape
    out = torch.empty(n, h // 2, w // 2, c, device=y.device, dtype=torch.float32)
    arg = torch.empty(n, h // 2, w // 2, c, device=y.device, dtype=torch.uint8)
    # (statistics for every width the grouping rule allows: dmd_gn_stats takes the groups of 32 and the general ones)
    stats = E.new_stats(n, c, 1, y.device) if (E.gn_width_ok(c) and valid is None) else None
    nv.check(nv.lib().dmd_maxpool2(nv.fptr(y), nv.fptr(out), nv.ptr(arg), nv.ptr(stats), n, h, w, c, nv.stream()), "dmd_maxpool2")
    if valid is not None:
        v2 = (valid[0] // 2, valid[1] // 2)
        return (E.gn_stats(out, v2) if E.gn_width_ok(c) else Act(out, valid=v2)), arg
    return Act(out, stats, 1 if stats is not None else 0), arg


# Arithmetic of the encoder's forward and dgrad convolutions: "f16x2" = split-fp32 on the f16 matrix cores where the
# shape is covered (fp32-class accuracy, see dmd_conv_f16ws.hip), "f32" = exact fp32 MFMA.  The weight gradient
# (contraction over pixels) runs on the split-fp16 instance of the wgrad kernel as well (its operands are pre-scaled to
# O(1) by the 2^k scaling of the backward), on the exact fp32 instance with "f32".
AC_PRECISION = os.environ.get("DIAMOND_AC_PRECISION", "f16x2")


def _w16(cache: E.PackCache, conv: nn.Conv2d) -> Optional[Tensor]:
    return cache.conv_weight_f16x2(conv) if AC_PRECISION == "f16x2" else None


# The backward launchers lived in this module before grad_ops.py; their old spellings stay for callers written against them.
_wgrad, _maxpool_bwd = G.wgrad, G.maxpool_bwd


def _gn_silu_bwd(x: Act, spec: NormSpec, da: Tensor, dskip: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    dx, dma = G.gn_bwd(x, spec, da, dskip)
    return dx, dma[0], dma[1]


class _Plan:
    """Static description of an ActorCriticEncoder: the layer list + the flat parameter order of
    the autograd.Function."""

    def __init__(self, encoder_seq: nn.Sequential) -> None:
        from .blocks import SmallResBlock

        layers = list(encoder_seq)
        assert isinstance(layers[0], nn.Conv2d), "encoder must start with Conv3x3 (actor_critic.py:105)"
        self.conv_in: nn.Conv2d = layers[0]
        self.blocks: List[Tuple[SmallResBlock, bool]] = []
        i = 1
        while i < len(layers):
            blk = layers[i]
            assert isinstance(blk, SmallResBlock), type(blk)
            pool = i + 1 < len(layers) and isinstance(layers[i + 1], nn.MaxPool2d)
            self.blocks.append((blk, pool))
            i += 2 if pool else 1
        # Image sizes the kernels take as they are: every convolution's level a multiple of the 8-pixel tiles.  A block's
        # convolution runs at the size left by the pools BEFORE it (the last pool's output only gets flattened): 64 for the
        # default encoder (levels 64 / 32 / 16 / 8 -> 4).  Other sizes: the valid extent of a padded buffer (_EncoderFn.forward).
        self.grid_multiple = 8 * 2 ** max(sum(1 for _, pool in self.blocks[:i] if pool) for i in range(len(self.blocks)))
        self.params: List[nn.Parameter] = [self.conv_in.weight, self.conv_in.bias]
        for blk, _ in self.blocks:
            gn, conv = blk.f[0].norm, blk.f[2]
            self.params += [gn.weight, gn.bias, conv.weight, conv.bias]
            if not isinstance(blk.skip_projection, nn.Identity):
                self.params += [blk.skip_projection.weight, blk.skip_projection.bias]
        # the flat gradient buffer of a backward: the parameters' gradients back to back in this order (sizes[i] floats each);
        # block j's parameters start at index block_first[j]
        self.sizes: List[int] = [p.numel() for p in self.params]
        self.numel = sum(self.sizes)
        self.block_first: List[int] = []
        i = 2
        for blk, _ in self.blocks:
            self.block_first.append(i)
            i += 4 if isinstance(blk.skip_projection, nn.Identity) else 6


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan: _Plan, cache: E.PackCache, obs: Tensor, *params: Tensor) -> Tensor:
        n, cimg, h, w = obs.shape
        # Image sizes off the kernels' 8-pixel grid at some level (the reference runs any size, MaxPool2d floors:
        # actor_critic.py:45, 72 -> 36 -> 18 -> 9 -> 4) live as the VALID EXTENT of a zero-padded buffer whose levels are all
        # multiples of 8 (include/diamond_hip.h; the denoiser does the same, engine.padded_extent)
        m = plan.grid_multiple
        obs_f, valid = E.pad_to_extent(obs.detach().float(), (h + m - 1) // m * m, (w + m - 1) // m * m)
        x16 = E.nchw_to_nhwc(obs_f, 16)
        ci = plan.conv_in
        x = E.conv2d([(Act(x16, valid=valid), nv.PROLOGUE_NONE, None)], cache.conv_weight(ci), cache.conv_bias(ci), ci.out_channels,
                     w_f16=_w16(cache, ci))
        saved = []
        for blk, pool in plan.blocks:
            gn, conv = blk.f[0].norm, blk.f[2]
            spec = NormSpec(mul=cache.f32(gn.weight), add=cache.f32(gn.bias))
            sp = blk.skip_projection
            if isinstance(sp, nn.Identity):
                r = x
            else:
                r = E.conv2d([(x, nv.PROLOGUE_NONE, None)], cache.conv_weight(sp), cache.conv_bias(sp), sp.out_channels, taps=1,
                             want_stats=False, w_f16=_w16(cache, sp))
            y = E.conv2d([(x, nv.PROLOGUE_NORM_SILU, spec)], cache.conv_weight(conv), cache.conv_bias(conv), conv.out_channels,
                         residual=r, want_stats=not pool, w_f16=_w16(cache, conv))
            arg = None
            nxt = y
            if pool:
                nxt, arg = _maxpool(y.t, y.valid)
            saved.append((x, arg))
            x = nxt
        ctx.plan, ctx.cache, ctx.x16, ctx.saved = plan, cache, Act(x16, valid=valid), saved
        ctx.bundled = len(params) != len(plan.params)  # (the parameters arrive as one _ParamBundleFn output)
        ctx.cimg = cimg
        ctx.out_valid, ctx.out_buf = x.valid, tuple(x.shape[1:3])
        # flatten in the reference's (c, h, w) order (actor_critic.py:71)
        feat = E.nhwc_to_nchw(x.t)
        return E.crop_to_valid(feat, x.valid, nchw=True).flatten(1)

    @staticmethod
    def backward(ctx, dfeat: Tensor):
        """Parameter gradients: every weight / bias gradient and every GroupNorm parameter gradient of this backward is a slice of
        ONE flat fp32 buffer (in the order of plan.params), written by ONE dmd_wgrad_reduce_jobs launch at the end, which also
        applies the 2^-k of the scaled backward.  With the parameter bundle (_ParamBundleFn) the flat buffer is the one gradient
        this node returns; without it (DIAMOND_AC_GRAD_BUNDLE=0) the per-parameter views of it are returned, same bits."""
        plan, cache = ctx.plan, ctx.cache
        split = AC_PRECISION == "f16x2"  # weight gradients in the split-fp16 form too (exact fp32 with DIAMOND_AC_PRECISION=f32)
        blk_last, _ = plan.blocks[-1]
        cl = blk_last.f[2].out_channels
        hb, wb = ctx.out_buf
        hl, wl = ctx.out_valid if ctx.out_valid is not None else (hb, wb)
        n = dfeat.shape[0]
        # the whole backward runs on dfeat * 2^k, the parameter gradients are scaled back by 2^-k at its end (grad_ops.pow2_scaled)
        dfeat, inv_scale = G.pow2_scaled(dfeat)
        dfeat, _ = E.pad_to_extent(dfeat.reshape(n, cl, hl, wl), hb, wb)  # zero gradient outside the valid extent of the last buffer
        dcur = E.nchw_to_nhwc(dfeat.contiguous())
        # (the reductions of this backward's weight gradients as ONE launch at its end instead of two per gradient: same sums;
        #  the launch multiplies by 2^-k as it writes: bitwise the multiplication pass it replaces)
        batch = G.wgrad_batch(inv_scale.reshape(1))
        flat = torch.empty(plan.numel, device=dfeat.device, dtype=torch.float32)
        # out[i] = the gradient of plan.params[i]: ONE split call (a view per parameter costs host time on a host-paced stretch);
        # the kernels take the 1-D pieces, only a convolution weight's is viewed in its OIHW shape (the reduction's row length)
        out = list(flat.split_with_sizes(plan.sizes))

        def wgrad(src, prologue, spec_, dy_, taps, cin, i):
            """dW, db into out[i], out[i + 1]"""
            out[i] = out[i].view(plan.params[i].shape)
            if batch is None:
                dw_, db_ = G.wgrad(src, prologue, spec_, dy_, taps, cin, split=split)
                torch.mul(dw_, inv_scale, out=out[i])
                torch.mul(db_, inv_scale, out=out[i + 1])
                return
            G.wgrad(src, prologue, spec_, dy_, taps, cin, split=split, batch=batch, dw_out=out[i], db_out=out[i + 1])
            if not G._wgrad_instance(dy_.shape[-1], src.C, taps):
                # (a width the kernel has no instance for is reduced tile by tile at once, not by the batch: scaled here)
                out[i].mul_(inv_scale)
                out[i + 1].mul_(inv_scale)

        for (blk, pool), (x, arg), i0 in zip(reversed(plan.blocks), reversed(ctx.saved), reversed(plan.block_first)):
            # out[i0 ...] = [gn.weight, gn.bias, conv.weight, conv.bias, (skip.weight, skip.bias)]
            gn, conv = blk.f[0].norm, blk.f[2]
            spec = NormSpec(mul=cache.f32(gn.weight), add=cache.f32(gn.bias))
            dy = G.maxpool_bwd(dcur, arg) if pool else dcur
            wgrad(x, nv.PROLOGUE_NORM_SILU, spec, dy, 9, conv.in_channels, i0 + 2)
            vy = x.valid  # (a stride-1 block: its output exists where its input does; dy is zero elsewhere, and is treated so)
            # (split-fp16 pieces of the transposed weight: asked for the 3x3 stride-1 convolutions only, none for the 1x1 projection)
            wt, wt16 = G.dgrad_weights(cache, conv, 0, conv.in_channels, f16x2=split and conv.kernel_size == (3, 3) and conv.stride == (1, 1))
            da = E.conv2d([(Act(dy, valid=vy), nv.PROLOGUE_NONE, None)], wt, None, conv.in_channels, want_stats=False, w_f16=wt16).t
            sp = blk.skip_projection
            if isinstance(sp, nn.Identity):
                dskip = dy
            else:
                wgrad(x, nv.PROLOGUE_NONE, None, dy, 1, sp.in_channels, i0 + 4)
                dskip = E.conv2d([(Act(dy, valid=vy), nv.PROLOGUE_NONE, None)], G.dgrad_weights(cache, sp, 0, sp.in_channels)[0], None,
                                 sp.in_channels, taps=1, want_stats=False).t
            dx, dma = G.gn_bwd(x, spec, da, dskip)
            # dgamma, dbeta = the sums of dma (2, N, C) over the batch: a job of the same launch (ascending n, fp64 accumulation);
            # with DIAMOND_WGRAD_DEFER=0 a launch of its own, the same kernel: the same bits
            gn_batch = batch if batch is not None else G.WgradBatch(inv_scale.reshape(1))
            gn_batch.add_colsum(dma, out[i0], out[i0 + 1])
            if batch is None:
                gn_batch.flush()
            dcur = dx
        wgrad(ctx.x16, nv.PROLOGUE_NONE, None, dcur, 9, ctx.cimg, 0)
        # the image gradient, only where autograd asks for it (saliency of the policy / value): conv_in's data gradient from the
        # same dcur, unscaled by the launch (one launch; none when obs requires no gradient: the imagined window's launches stay)
        d_obs = None
        if ctx.needs_input_grad[2]:
            d_obs, _ = G.dgrad_input(Act(dcur, valid=ctx.x16.valid), plan.conv_in, ctx.cimg, want_b=False, post=inv_scale.reshape(1))
        if batch is not None:
            batch.flush()
        if ctx.bundled:
            return (None, None, d_obs, flat)
        return (None, None, d_obs, *[g.view(p.shape) for g, p in zip(out, plan.params)])


class _ParamBundleFn(torch.autograd.Function):
    """The autograd edge between the encoder's parameters and the _EncoderFn nodes of ONE recorded graph: its output stands for
    all of plan.params (a flat fp32 buffer of their total size whose VALUES nobody reads: _EncoderFn.forward takes the weights
    from the pack cache), its backward splits the flat gradient into per-parameter views.  Every _EncoderFn.backward of the graph
    returns one flat gradient; autograd sums the 15 steps' with one add per step instead of one per parameter and step, and
    AccumulateGrad -- and any post-accumulate hook (dist.GradAllReducer) -- runs once per parameter and backward.

    Summation order across the steps of a window: autograd adds the gradients that reach a node in that node's input buffer as
    their producers run, last step first, and runs the node once: S = ((g14 + g13) + ...) + g0 elementwise, then AccumulateGrad
    forms .grad = G + S for a .grad G that exists already (S itself where .grad is None).  That is the order with and without
    the bundle -- without it the sum S is formed per parameter in that parameter's AccumulateGrad input buffer, with it once on
    the flat buffer in this node's -- so every .grad is bitwise the same either way, also on top of a non-zero G carried over
    from gradient accumulation."""

    @staticmethod
    def forward(ctx, owner_ref, plan: _Plan, *params: Tensor) -> Tensor:
        ctx.owner_ref, ctx.plan = owner_ref, plan
        return torch.empty(plan.numel, device=params[0].device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, g: Tensor):
        owner = ctx.owner_ref()
        if owner is not None:
            owner._bundle = None  # the graph is consumed: the next recorded graph gets its own node
        plan = ctx.plan
        return (None, None, *[piece.view(p.shape) for piece, p in zip(g.split_with_sizes(plan.sizes), plan.params)])


def grad_bundle_enabled() -> bool:
    """DIAMOND_AC_GRAD_BUNDLE=0: one gradient per encoder parameter and _EncoderFn node, accumulated by autograd parameter by
    parameter (the A/B arm; same bits from a zero or absent .grad)."""
    return os.environ.get("DIAMOND_AC_GRAD_BUNDLE", "1") != "0"


class NativeEncoder:
    """Host-side launcher bound to one ActorCritic module (packed-weight cache + plan)."""

    def __init__(self, encoder_seq: nn.Sequential) -> None:
        self.plan = _Plan(encoder_seq)
        self.cache = E.PackCache()
        self._bundle: Optional[Tensor] = None  # the _ParamBundleFn output of the graph being recorded (reset by its backward)
        self._bundle_key = None

    def __call__(self, obs: Tensor) -> Tensor:
        nv.require_gpu(obs)
        params = self.plan.params
        if grad_bundle_enabled() and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            key = tuple(p.requires_grad for p in params) + (params[0].device,)
            if self._bundle is None or self._bundle_key != key:
                self._bundle, self._bundle_key = _ParamBundleFn.apply(weakref.ref(self), self.plan, *params), key
            return _EncoderFn.apply(self.plan, self.cache, obs.contiguous(), self._bundle)
        return _EncoderFn.apply(self.plan, self.cache, obs.contiguous(), *params)
