"""Training backward of the denoiser's U-Net on the hand-written HIP kernels (the
`loss.backward()` of `Denoiser.forward`, reference denoiser.py:93-122 / trainer.py:363-366, where ATen autograd
differentiates blocks.py / inner_model.py).

Design: the inference forward (`InnerModel.run`) is executed unchanged while `engine.TAPE` records every conv /
attention launch; ONE `torch.autograd.Function` spans the whole network and its backward walks the tape in reverse.
Per recorded convolution, with dOut the gradient of its output (the launches themselves: grad_ops.py):
  * bias / weight gradient  -> `dmd_conv2d_wgrad` per source (the activated input SiLU(GN(x)*..) is recomputed from x and
    its statistics while staging: nothing but the layer inputs was saved);
  * data gradient           -> `dmd_conv2d` on the flipped / transposed weight slice of that source (split-fp16 MFMA
    where the shape is covered); a stride-2 convolution runs both on the zero-stuffed dOut, an upsampling one on the
    materialised nearest-x2 input followed by a 2x2 sum;
  * fused prologue          -> `dmd_gn_silu_bwd` (GroupNorm + FiLM/affine + SiLU or identity): dx plus per-(sample,
    channel) gradients of the multiplicative / additive terms, which are columns of the batched FiLM table
    (AdaGroupNorm) or the affine parameters of an nn.GroupNorm;
  * residual                -> accumulated into the gradient of the residual tensor (through the GroupNorm affine for
    the attention block's `x_normed + out_proj(y)`, blocks.py:72).
Attention core: grad_ops.attention_bwd (`dmd_attention_bwd`, from ATTN_BWD_MFMA_MIN_T valid tokens on `dmd_attention_bwd_mfma`).
The FiLM table itself (`cond @ W_cat^T + b_cat`), the 256-wide cond MLP and the
action embedding are a handful of tiny GEMMs: they run as torch ops under ordinary autograd, so the table gradient
returned here flows on into the 44 AdaGroupNorm linears, `cond_proj` and `act_emb`.
Image gradients: where autograd asks for one, conv_in's data gradient goes to the caller's images through grad_ops.dgrad_input
(`dmd_conv2d_dgrad_input`, one launch; UNetTrainFn / EncoderTrainFn take the images as inputs of their own only then).
Image sizes off the kernels' tile grid record on the VALID EXTENT of a padded buffer (engine.padded_extent): the gradient
tensors' margins are then unspecified, and every kernel of the walk reads only the extent it is given (data gradients: dy's,
weight gradients / GroupNorm backward: their source's, attention: `dmd_attention_bwd_valid`).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import engine as E
from . import grad_ops as G
from . import native as nv
from .engine import Act, AttnRecord, CatRecord, ConvRecord, NormSpec
from .grad_ops import ATTN_BWD_MFMA_MIN_T, attn_bwd_mfma_min_t  # noqa: F401  (read-only here: tools and tests read the default; DIAMOND_ATTN_BWD_MIN_T overrides it)

TRAIN_PRECISION = "f16x2"  # arithmetic of the forward, dgrad and wgrad convolutions (split-fp16 operands, fp32 accumulate); "f32" = exact


def _key(t: Tensor) -> int:
    return t.data_ptr()


class _Grads:
    """Gradient accumulator keyed by activation storage."""

    def __init__(self) -> None:
        self.g: Dict[int, Tensor] = {}

    def add(self, t: Tensor, g: Tensor) -> None:
        k = _key(t)
        if k in self.g:
            self.g[k] = self.g[k] + g
        else:
            self.g[k] = g

    def pop(self, t: Tensor) -> Optional[Tensor]:
        return self.g.pop(_key(t), None)

    def peek(self, t: Tensor) -> Optional[Tensor]:
        return self.g.get(_key(t))


def _twice(valid: Optional[Tuple[int, int]]) -> Optional[Tuple[int, int]]:
    return None if valid is None else (2 * valid[0], 2 * valid[1])


def _zero_stuff(dy: Tensor) -> Tensor:
    """(N, H, W, C) -> (N, 2H, 2W, C) with dy at the even positions: the transposed stride-2 convolution and its weight
    gradient are the stride-1 ones of this tensor."""
    n, h, w, c = dy.shape
    z = torch.zeros(n, 2 * h, 2 * w, c, device=dy.device, dtype=dy.dtype)
    z[:, ::2, ::2] = dy
    return z


def _upsample_nearest(x: Tensor) -> Tensor:
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()


def _sum_pool2(g: Tensor) -> Tensor:
    n, h, w, c = g.shape
    return g.reshape(n, h // 2, 2, w // 2, 2, c).sum(dim=(2, 4)).contiguous()


class _ParamGrads:
    def __init__(self, table: Tensor) -> None:
        self._table = table
        self._pieces: Dict[int, Tensor] = {}  # first column -> (N, c) gradient block of the FiLM table
        self._dtable: Optional[Tensor] = None
        self.by_param: Dict[int, Tensor] = {}

    def add_param(self, p: nn.Parameter, g: Tensor) -> None:
        k = id(p)
        self.by_param[k] = self.by_param[k] + g if k in self.by_param else g

    def norm_terms(self, spec: NormSpec, dmul: Tensor, dadd: Tensor) -> None:
        c = dmul.shape[1]
        if spec.film_cols is not None:  # AdaGroupNorm: y = xn * (1 + scale) + shift -> d scale = dmul, d shift = dadd
            mc, ac = spec.film_cols
            # every column block of the table belongs to ONE normalised source: the blocks are collected and the table
            # is assembled once (dtable) -- not 2 strided `+=` launches per normalisation
            for col, g in ((mc, dmul), (ac, dadd)):
                self._pieces[col] = self._pieces[col] + g if col in self._pieces else g
        elif spec.gn_module is not None:
            self.add_param(spec.gn_module.weight, dmul.sum(0))
            self.add_param(spec.gn_module.bias, dadd.sum(0))

    @property
    def dtable(self) -> Tensor:
        """Gradient of the batched FiLM table (N, total): the collected column blocks, zeros where no block was produced."""
        if self._dtable is None:
            n, total = self._table.shape
            parts, at = [], 0
            for col in sorted(self._pieces):
                g = self._pieces[col]
                assert col >= at, "overlapping FiLM column blocks"
                if col > at:
                    parts.append(torch.zeros(n, col - at, device=g.device, dtype=g.dtype))
                parts.append(g)
                at = col + g.shape[1]
            if at < total or not parts:
                parts.append(torch.zeros(n, total - at, device=self._table.device, dtype=self._table.dtype))
            self._dtable = torch.cat(parts, dim=1)
        return self._dtable


def backward_tape(tape: List, cache: E.PackCache, d_out: Tensor, table: Tensor, use_f16: bool,
                  out_nhwc: Optional[Tensor] = None, image_grad: Optional[Callable[[Act, nn.Conv2d], None]] = None) -> _ParamGrads:
    """Walk the recorded launches in reverse; returns the parameter / FiLM-table gradients.
    `out_nhwc` None: the tape ends with the NCHW head convolution (U-Net) and `d_out` is (N, 3, H, W); otherwise
    `out_nhwc` is the recorded NHWC activation the network returned (an encoder) and `d_out` its gradient.
    `image_grad` (set only where autograd asks for an image gradient): the network input -- the one source recorded with
    needs_grad=False, conv_in's -- then carries a gradient: image_grad(dy, conv_in) is called with the gradient of conv_in's
    output on the extent of its source (one grad_ops.dgrad_input launch, the caller's; nothing is launched without it)."""
    grads = _Grads()
    pg = _ParamGrads(table)
    pending_norm: Dict[int, Tensor] = {}  # gradient w.r.t. GN_affine(x) handed over by a residual_norm consumer
    # the reductions of ALL weight gradients as one launch per 32 at the end (bit-identical sums), every source / 64-channel piece
    # of a convolution writing its slice of ONE OIHW tensor; DIAMOND_WGRAD_DEFER=0: reduced per call and concatenated, as before
    batch = G.wgrad_batch()
    if out_nhwc is None:
        last = tape[-1]
        assert isinstance(last, ConvRecord) and last.out_nchw, "the tape must end with the NCHW head convolution"
        # dF (N, 3, H, W) -> NHWC with the channels zero-padded to 16 (wgrad / dgrad work on 16-channel groups)
        grads.add(last.out.t, E.nchw_to_nhwc(d_out.contiguous().float(), 16))
    else:
        grads.add(out_nhwc, d_out.contiguous().float())
    for rec in reversed(tape):
        if isinstance(rec, AttnRecord):
            dy = grads.pop(rec.out)
            if dy is None:
                continue
            grads.add(rec.qkv.t, G.attention_bwd(rec, dy))
            continue
        if isinstance(rec, CatRecord):  # a materialised channel concatenation (engine.concat): the gradient split by channels
            dy = grads.pop(rec.out.t)
            if dy is None:
                continue
            c0 = 0
            for a in rec.srcs:
                if a.needs_grad:
                    grads.add(a.t, dy[..., c0:c0 + a.C].contiguous())
                c0 += a.C
            continue
        dout = grads.pop(rec.out.t)
        if dout is None:
            continue
        conv = rec.module
        cout = conv.out_channels
        head = rec.out_nchw  # conv_out: dout carries 16 channels (3 real)
        cpad = 16 if head else None
        # ---- residual branch
        if rec.residual is not None:
            if rec.residual_norm is not None:  # x_normed + out_proj(y): goes through GN_affine(x) with the qkv branch
                pending_norm[_key(rec.residual.t)] = dout
            else:
                grads.add(rec.residual.t, dout)
        # ---- geometry of the gradient the weight / data kernels consume.  Under a VALID EXTENT the gradient tensors' margins
        # are unspecified (a data gradient writes the whole buffer): the data gradient reads dy as the extent of the output it is
        # the gradient of (zero-stuffed: twice that), the weight gradient masks dy by its source's extent
        dy_k = _zero_stuff(dout) if rec.stride == 2 else dout
        dy_valid = _twice(rec.out.valid) if rec.stride == 2 else rec.out.valid
        k = conv.kernel_size[0]
        dws: List[Tensor] = []
        db: Optional[Tensor] = None
        c0 = 0
        if batch is not None:  # (rows: the channel count dy carries -- the head's 3 output channels travel padded to 16)
            dw_all = torch.empty(dy_k.shape[-1], conv.in_channels, k, k, device=dy_k.device, dtype=torch.float32)
            db = torch.empty(dy_k.shape[-1], device=dy_k.device, dtype=torch.float32)
        for si, (a, prologue, spec) in enumerate(rec.srcs):
            ci_pad = a.C
            ci_real = min(ci_pad, conv.in_channels - c0)
            src = Act(_upsample_nearest(a.t), valid=_twice(a.valid)) if rec.upsample else a
            assert not (rec.upsample and prologue != nv.PROLOGUE_NONE)
            step = 64 if cout > 64 and not head else dy_k.shape[-1]  # (the wgrad instances take at most 64 output channels: qkv)
            parts = []
            for o in range(0, dy_k.shape[-1], step):
                dy_o = dy_k if step == dy_k.shape[-1] else dy_k[..., o:o + step].contiguous()
                if batch is not None:
                    G.wgrad(src, prologue, spec, dy_o, rec.taps, ci_real, split=use_f16, batch=batch, dw_out=dw_all[o:o + step], c0=c0,
                            db_out=db[o:o + step] if si == 0 else None)
                else:
                    parts.append(G.wgrad(src, prologue, spec, dy_o, rec.taps, ci_real, split=use_f16))
            if batch is None:  # (reduced per call; the 64-row pieces of a gradient concatenated)
                dw_i, db_i = parts[0] if len(parts) == 1 else (torch.cat([p_[i] for p_ in parts], dim=0) for i in (0, 1))
                dws.append(dw_i[:cout])
                if si == 0:
                    db = db_i[:cout]
            if a.needs_grad:
                wp, w16 = G.dgrad_weights(cache, conv, c0, c0 + ci_real, cpad or 0, f16x2=use_f16)
                da = E.conv2d([(Act(dy_k, valid=dy_valid), nv.PROLOGUE_NONE, None)], wp, None, ci_real, taps=rec.taps, want_stats=False,
                              w_f16=w16, fast_math=use_f16).t
                if rec.upsample:
                    da = _sum_pool2(da)
                if prologue == nv.PROLOGUE_NONE:
                    grads.add(a.t, da)
                else:
                    identity = prologue == nv.PROLOGUE_NORM
                    if identity and _key(a.t) in pending_norm:
                        da = da + pending_norm.pop(_key(a.t))
                    dx, (dmul, dadd) = G.gn_bwd(a, spec, da, grads.pop(a.t), identity)
                    grads.g[_key(a.t)] = dx  # dx already contains the gradient accumulated so far (dskip)
                    pg.norm_terms(spec, dmul, dadd)
            elif image_grad is not None:  # the network input: the first convolution's data gradient goes to the caller's images
                assert prologue == nv.PROLOGUE_NONE and rec.stride == 1 and rec.taps == 9 and not rec.upsample and len(rec.srcs) == 1
                # (a stride-1 convolution's output exists where its source does: what InnerModel.run zero-fills behind it carries none)
                image_grad(Act(dy_k, valid=a.valid), conv)
            c0 += ci_real
        if batch is not None:
            if id(conv.weight) in pg.by_param:  # a convolution recorded twice: its gradients are ADDED, so they have to exist
                batch.flush()
            pg.add_param(conv.weight, dw_all[:cout])
            db = db[:cout]
        else:
            pg.add_param(conv.weight, torch.cat(dws, dim=1) if len(dws) > 1 else dws[0])
        if conv.bias is not None and db is not None:
            pg.add_param(conv.bias, db)
    if batch is not None:
        batch.flush()
    assert not pending_norm, "a normalised residual was never matched with its pre-norm consumer"
    return pg


class UNetTrainFn(torch.autograd.Function):
    """F = InnerModel.run(packed_in, table) with a hand-written backward.  Inputs that carry gradients: the FiLM
    table and every parameter in `params` (the convolutions, nn.GroupNorm affines and attention projections of
    conv_in / unet / norm_out / conv_out).  valid = (h, w): the image is that part of the zero-padded packed_in
    (InnerModel.run); F is meaningful in [:h, :w] only and the caller crops it (its gradient is zero outside)."""

    IMAGE_ARGS = 6  # position of (noisy, obs) among forward's arguments

    @staticmethod
    def forward(ctx, inner, packed_in: Tensor, table: Tensor, precision: str, valid: Optional[Tuple[int, int]],
                attn_precision: Optional[str], noisy: Optional[Tensor], obs: Optional[Tensor],
                image_scales: Optional[Tuple[Tensor, float]], *params: Tensor) -> Tensor:
        """noisy, obs: the images packed_in was built from (Denoiser.model_output_with_grad), handed over ONLY when one of them
        requires a gradient -- they are then differentiable inputs (their values are not read: packed_in holds them);
        image_scales = (c_in (N,) device, 1 / sigma_data): d noisy = c_in[n] * d packed[:, cobs:], d obs = d packed[:, :cobs] / sigma_data
        (dmd_edm_pack_input packs obs first).  None, None, None otherwise: the backward is what it was, launch for launch."""
        assert E.TAPE is None, "nested recording"
        E.TAPE = []
        try:
            out = inner.run(packed_in, None, precision=precision, table=table.detach(), valid=valid, attn_precision=attn_precision)
            tape = E.TAPE
        finally:
            E.TAPE = None
        ctx.inner, ctx.tape, ctx.table, ctx.precision = inner, tape, table.detach(), precision
        ctx.params = params
        ctx.image_scales, ctx.cx = image_scales, (0 if noisy is None else noisy.shape[1])
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        need_noisy, need_obs = ctx.needs_input_grad[UNetTrainFn.IMAGE_ARGS:UNetTrainFn.IMAGE_ARGS + 2]
        images = {}
        image_grad = None
        if need_noisy or need_obs:
            c_in, inv_sd = ctx.image_scales

            def image_grad(dy: Act, conv: nn.Conv2d, inv: Tensor) -> None:
                # channels [0, cobs) are obs / sigma_data (a host scalar), [cobs, cobs + cx) noisy * c_in[n]: swap_scales
                images["obs"], images["noisy"] = G.dgrad_input(dy, conv, conv.in_channels - ctx.cx, want_a=need_obs, want_b=need_noisy,
                                                               scale_a=c_in, scale_b=inv_sd, post=inv.reshape(1), swap_scales=True)

        pg, inv = scaled_backward(ctx.tape, ctx.inner._cache, d_out, ctx.table, use_f16=ctx.precision == "f16x2", image_grad=image_grad)
        ctx.tape = None  # free the saved activations
        grads = _unscale(pg, ctx.params, inv)
        return (None, None, pg.dtable * inv, None, None, None, images.get("noisy"), images.get("obs"), None, *grads)


def _unscale(pg: "_ParamGrads", params, inv: Tensor):
    """Gradients of the scaled problem times 2^-k.  One multiply per parameter would be 236 launches of 4 us for the
    denoiser (torch._foreach_mul with a device scalar falls back to exactly that): the gradients are gathered into one flat
    buffer (torch.cat: two launches), scaled there, and handed out as views of it."""
    have = [pg.by_param[id(p)] for p in params if pg.by_param.get(id(p)) is not None]
    if not have:
        return tuple(None for _ in params)
    flat = torch.cat([g.reshape(-1) for g in have])
    flat *= inv
    out, off = [], 0
    for g in have:
        out.append(flat[off:off + g.numel()].view(g.shape))
        off += g.numel()
    scaled = iter(out)
    return tuple(None if pg.by_param.get(id(p)) is None else next(scaled) for p in params)


def scaled_backward(tape: List, cache: E.PackCache, d_out: Tensor, table: Tensor, use_f16: bool,
                    out_nhwc: Optional[Tensor] = None, image_grad=None) -> Tuple[_ParamGrads, Tensor]:
    """backward_tape on d_out * 2^k with the largest entry O(1) (grad_ops.pow2_scaled); returns (gradients of the scaled
    problem, 2^-k).  image_grad(dy, conv_in, 2^-k), or None: backward_tape's, with the factor that unscales its result."""
    d_scaled, inv = G.pow2_scaled(d_out)
    if image_grad is None:
        return backward_tape(tape, cache, d_scaled, table, use_f16, out_nhwc), inv
    return backward_tape(tape, cache, d_scaled, table, use_f16, out_nhwc, image_grad=lambda dy, conv: image_grad(dy, conv, inv)), inv


class EncoderTrainFn(torch.autograd.Function):
    """feat = encoder.run(x, table) (an AdaGN-ResBlock encoder returning an NHWC activation: RewEndEncoder) with the
    same recorded-tape backward as the U-Net.  `run(table) -> Tensor` executes the forward."""

    IMAGE_ARGS = 4  # position of (frames_a, frames_b) among forward's arguments

    @staticmethod
    def forward(ctx, run, cache: E.PackCache, table: Tensor, precision: str, frames_a: Optional[Tensor], frames_b: Optional[Tensor],
                *params: Tensor) -> Tensor:
        """frames_a, frames_b: the images whose channel concatenation `run` feeds to conv_in (RewEndModel: obs, next_obs), handed over
        ONLY when one of them requires a gradient (differentiable inputs whose values are not read); None, None otherwise."""
        assert E.TAPE is None, "nested recording"
        E.TAPE = []
        try:
            out = run(table.detach())
            tape = E.TAPE
        finally:
            E.TAPE = None
        ctx.cache, ctx.tape, ctx.table, ctx.precision, ctx.out, ctx.params = cache, tape, table.detach(), precision, out, params
        ctx.frame_shapes = tuple(None if f is None else tuple(f.shape) for f in (frames_a, frames_b))
        return out

    @staticmethod
    def backward(ctx, d_out: Tensor):
        need_a, need_b = ctx.needs_input_grad[EncoderTrainFn.IMAGE_ARGS:EncoderTrainFn.IMAGE_ARGS + 2]
        images = {}
        image_grad = None
        if need_a or need_b:
            sa, sb = ctx.frame_shapes

            def image_grad(dy: Act, conv: nn.Conv2d, inv: Tensor) -> None:
                da, db = G.dgrad_input(dy, conv, sa[-3], want_a=need_a, want_b=need_b, post=inv.reshape(1))
                images["a"], images["b"] = (None if da is None else da.view(sa)), (None if db is None else db.view(sb))

        pg, inv = scaled_backward(ctx.tape, ctx.cache, d_out, ctx.table, ctx.precision == "f16x2", out_nhwc=ctx.out, image_grad=image_grad)
        ctx.tape = ctx.out = None
        grads = _unscale(pg, ctx.params, inv)
        return (None, None, pg.dtable * inv, None, images.get("a"), images.get("b"), *grads)


def trainable_unet_params(inner) -> List[nn.Parameter]:
    """Parameters whose gradients come out of UNetTrainFn (everything the recorded launches touch directly; the
    AdaGroupNorm linears, cond_proj and act_emb get theirs through the FiLM table under torch autograd)."""
    from .blocks import AdaGroupNorm

    skip = set()
    for m in inner.modules():
        if isinstance(m, AdaGroupNorm):
            skip.update(id(p) for p in m.parameters())
    skip.update(id(p) for p in inner.cond_proj.parameters())
    skip.update(id(p) for p in inner.act_emb.parameters())
    return [p for p in inner.parameters() if id(p) not in skip]
