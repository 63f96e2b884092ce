"""TEST INFRASTRUCTURE: one entry point of the C ABI (include/diamond_hip.h) on the SIMT interpreter and on the device, through the
same launch, the same inputs and the same assertions -- what every *_precision test of a kernel is written against.

A RUNNER knows how an array gets to its machine and back, nothing else:

    run.name        "simt" / "gpu"
    run.lib()       the library (tests/simt's interpreter build / diamond_amd.native's), loaded at the first call
    run.put(a)      a numpy array or CPU tensor -> a handle that owns a contiguous copy; put(None) is None
    run.ptr(h)      the handle's address for the C ABI; ptr(None) is None
    run.get(h)      the handle's content as a fresh numpy array (on the device: .cpu(), which synchronises)
    run.stream()    the stream argument (None / native.stream())

Simt.put FENCES every array (tests/simt/fence.py: the copy ends at an inaccessible page, so a kernel that reads or writes past a
tensor faults instead of touching a neighbour); Simt.get copies out of the fence.  Gpu.put makes a contiguous device tensor.
Importing this file loads no library and touches no GPU: diamond_amd.native is here for struct layouts and the signature table.

A LAUNCHER is one entry point written once against a runner.  Every output and every workspace starts as NaN (`nan_like`) on
both runners, so an element a kernel does not write shows; inputs go through run.put and nothing else.  Launchers return NUMPY
arrays (what run.get gives); a caller that works in torch wraps them in torch.from_numpy.  With status=True a launcher returns
(rc, dmd_last_error() text, outputs) instead of raising on a nonzero status: the refused-argument tests.

`arms(simt, gpu, cases)` builds the pytest parameters: for each case (a tuple of values, or one value) `simt-<tag>` and
`gpu-<tag>`, the latter marked pytest.mark.gpu, the tag the case's values joined by "-" (a tuple among them by "x"); with no cases
the ids are `simt` and `gpu` (RUNNERS is that list for the plain runners).  `simt_if(*case)` leaves cases off the interpreter
arm (long token counts, device-only extents).  `simt` and `gpu` are the runners or namespaces around them that carry a module's
per-arm data (a channel count, shapes): the cases a kernel is measured on stay with its tests.

    from tests import abi

    @pytest.mark.parametrize("run,t", abi.arms(abi.Simt, abi.Gpu, [64, 320, 1024], simt_if=lambda t: t <= 512))  # 5 cases
    def test_attention_is_finite(run, t):
        qkv = torch.randn(2, t, 48, generator=torch.Generator().manual_seed(t))
        assert np.isfinite(abi.attention(run, qkv, 16)).all()
"""
import ctypes as C

import numpy as np
import pytest
import torch

from diamond_amd import native as nv  # struct layouts and the signature table only
from tests import groupnorm_cases as GC


# ---- the two runners: the same C ABI, on fenced host arrays (interpreter build) and on device tensors --------------------------------
def _array(a):
    return a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class Simt:
    """the kernels' own source on the interpreter, arrays fenced"""
    name = "simt"

    @staticmethod
    def lib():
        from tests.simt import loader as S
        return S.lib()

    @staticmethod
    def put(a):
        from tests.simt.fence import fenced
        return None if a is None else fenced(np.ascontiguousarray(_array(a)))

    @staticmethod
    def ptr(h):
        return None if h is None else h.ctypes.data

    @staticmethod
    def get(h):
        return np.array(h)

    @staticmethod
    def stream():
        return None


class Gpu:
    name = "gpu"

    @staticmethod
    def lib():
        return nv.lib()

    @staticmethod
    def put(a):
        return None if a is None else torch.tensor(_array(a)).cuda().contiguous()

    @staticmethod
    def ptr(h):
        return None if h is None else h.data_ptr()

    @staticmethod
    def get(h):
        return h.cpu().numpy()

    @staticmethod
    def stream():
        return nv.stream()


def arms(simt, gpu, cases=None, simt_if=None, tag=None, values=None):
    """pytest parameters (arm, *case) with the ids simt-<tag> / gpu-<tag> (the module docstring has the rule).  tag(*case): another
    spelling of the tag; values(arm, *case): the parameters of a case where they depend on the arm"""
    if cases is None:
        return [pytest.param(simt, id="simt"), pytest.param(gpu, marks=pytest.mark.gpu, id="gpu")]
    tag = tag or (lambda *case: "-".join("x".join(str(v) for v in x) if isinstance(x, tuple) else str(x) for x in case))
    values = values or (lambda arm, *case: case)
    out = []
    for case in cases:
        case = case if isinstance(case, tuple) else (case,)
        if simt_if is None or simt_if(*case):
            out.append(pytest.param(simt, *values(simt, *case), id=f"simt-{tag(*case)}"))
        out.append(pytest.param(gpu, *values(gpu, *case), marks=pytest.mark.gpu, id=f"gpu-{tag(*case)}"))
    return out


def joined_by_x(*case):
    """a tag for arms(): 16x16x9x9"""
    return "x".join(str(v) for v in case)


def arms_by_token_count(simt, gpu, ts, *more, simt_max_t=512):
    """arms() of the cases (t, *extra) of every t and every extra (a value or a tuple), t outermost: the interpreter arm gets
    T <= simt_max_t only, the device arm every T"""
    cases = [(t,) + (e if isinstance(e, tuple) else (e,)) for t in ts for e in (more or [()])]
    return arms(simt, gpu, cases, simt_if=lambda t, *_: t <= simt_max_t)


RUNNERS = arms(Simt, Gpu)


def check(run, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {run.lib().dmd_last_error().decode()}")


def nan_like(shape, dtype=np.float32):
    return np.full(shape, np.nan, dtype=dtype)


def _finish(run, rc, what, status, outs):
    """what a launcher returns: its outputs, or with status=True (rc, the library's message, outputs) without raising"""
    if status:
        return rc, run.lib().dmd_last_error().decode(), outs()
    check(run, rc, what)
    return outs()


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def attention(run, qkv, c, entry="dmd_attention", extent=None, head_dim=8, status=False):
    """qkv (N, ..., 3C) -> out (N, ..., C).  dmd_attention takes the tokens flat; dmd_attention_valid / _f16x2 / _f32 take
    extent = (H, W, valid_h, valid_w), by default one row of all the tokens, (1, T, 1, T)"""
    n, t = qkv.shape[0], int(np.prod(qkv.shape[1:-1]))
    a, out = run.put(qkv), run.put(nan_like(tuple(qkv.shape[:-1]) + (c,)))
    grid = (t,) if entry == "dmd_attention" else tuple(extent or (1, t, 1, t))
    rc = getattr(run.lib(), entry)(run.ptr(a), run.ptr(out), n, *grid, c, head_dim, run.stream())
    return _finish(run, rc, entry, status, lambda: run.get(out))


def attention_default(run, qkv, c, exact=False):
    """dmd_attention on (N, T, 3C); exact=True: dmd_attention_valid over the whole (T / 16, 16) grid, attention_kernel at any T"""
    t = qkv.shape[1]
    return attention(run, qkv, c, "dmd_attention_valid", (t // 16, 16, t // 16, 16)) if exact else attention(run, qkv, c)


def attention_bwd(run, qkv, y, dy, c, entry="dmd_attention_bwd", extent=None, status=False):
    """qkv / y / dy (N, ..., 3C | C | C) -> dqkv.  dmd_attention_bwd takes the tokens flat; dmd_attention_bwd_valid / _mfma take
    extent = (H, W, valid_h, valid_w), by default (1, T, 1, T).  The workspace is dmd_attention_bwd_workspace_floats of the grid"""
    L = run.lib()
    n, t = qkv.shape[0], int(np.prod(qkv.shape[1:-1]))
    a = [run.put(x) for x in (qkv, y, dy)]
    ws = run.put(nan_like(int(L.dmd_attention_bwd_workspace_floats(n, t, c))))
    dqkv = run.put(nan_like(tuple(qkv.shape)))
    grid = (t,) if entry == "dmd_attention_bwd" else tuple(extent or (1, t, 1, t))
    rc = getattr(L, entry)(*(run.ptr(x) for x in a), run.ptr(dqkv), run.ptr(ws), n, *grid, c, 8, run.stream())
    return _finish(run, rc, entry, status, lambda: run.get(dqkv))


# ---- dmd_conv2d_dgrad_input ----------------------------------------------------------------------------------------------------------
def dgrad_input(run, dy, wt, cin, c_split, valid=None, scale_a=None, scale_b=1.0, post=None, swap=False, want_a=True, want_b=True,
                status=False):
    """dy (N, H, W, Cout), wt (Cout, cin, 3, 3) -> (dx_a, dx_b), NCHW cropped to the valid extent, None where not wanted or empty"""
    n, h, w, cout = dy.shape
    vh, vw = valid or (h, w)
    vh, vw = min(vh, h), min(vw, w)  # (the refused-argument test asks for more than the buffer: the outputs stay inside it)
    keep = [run.put(dy), run.put(wt)]
    dx_a = run.put(nan_like((n, c_split, vh, vw))) if want_a and c_split > 0 else None
    dx_b = run.put(nan_like((n, max(cin - c_split, 0), vh, vw))) if want_b and cin > c_split else None
    p = nv.DgradInputParams()
    p.N, p.H, p.W, p.Cout, p.cin, p.c_split = n, h, w, cout, cin, c_split
    if valid is not None:
        p.valid_h, p.valid_w = valid
    p.stride_a, p.scale_b, p.swap_scales = 0, scale_b, int(swap)
    p.dy, p.w, p.dx_a, p.dx_b = run.ptr(keep[0]), run.ptr(keep[1]), run.ptr(dx_a), run.ptr(dx_b)
    if scale_a is not None:
        keep.append(run.put(scale_a))
        p.scale_a, p.stride_a = run.ptr(keep[-1]), int(_array(scale_a).size > 1)
    if post is not None:
        keep.append(run.put(np.array([post], dtype=np.float32)))
        p.post = run.ptr(keep[-1])
    rc = run.lib().dmd_conv2d_dgrad_input(C.byref(p), run.stream())
    return _finish(run, rc, "dmd_conv2d_dgrad_input", status, lambda: tuple(None if a is None else run.get(a) for a in (dx_a, dx_b)))


# ---- GroupNorm statistics, dmd_norm, weight packs, dmd_conv2d --------------------------------------------------------------------------
def kernel_sums(run, x, hv=None, wv=None):
    """(N, G, 1, 2) sums of dmd_gn_stats / dmd_gn_stats_valid (gn_stats_kernel; gn_stats_any_kernel for the general groups)"""
    n, h, w, c = x.shape
    xd, st = run.put(x), run.put(nan_like((n, GC.groups_of(c), 1, 2), np.float64))
    if hv is None:
        check(run, run.lib().dmd_gn_stats(run.ptr(xd), run.ptr(st), n, h * w, c, run.stream()), "dmd_gn_stats")
    else:
        check(run, run.lib().dmd_gn_stats_valid(run.ptr(xd), run.ptr(st), n, h, w, hv, wv, c, run.stream()), "dmd_gn_stats_valid")
    return run.get(st)


def norm_struct(run, keep, stats, mul, add, plus_one):
    hs = [run.put(a) for a in (stats, mul, add)]
    keep += hs
    n = nv.Norm()
    n.stats, n.stat_tiles, n.mul_plus_one = run.ptr(hs[0]), stats.shape[2], int(plus_one)
    n.mul, n.add = run.ptr(hs[1]), run.ptr(hs[2])
    n.mul_stride = 0 if mul is None else mul.shape[-1]
    n.add_stride = 0 if add is None else add.shape[-1]
    return n


def act_norm(run, keep, a, stats=None):
    """the dmd_norm of an activation of the cases file, statistics from the statistics kernel unless given"""
    if stats is None:
        stats = kernel_sums(run, a.x, *((a.hv, a.wv) if (a.hv, a.wv) != (a.h, a.w) else ()))
    return norm_struct(run, keep, stats, a.mul, a.add, a.plus_one)


def pack_f32(run, keep, w, cout_pad):
    cout, cin, k, _ = w.shape
    src, dst = run.put(w), run.put(nan_like((cin // 16) * k * k * cout_pad * 16))
    keep += [src, dst]
    check(run, run.lib().dmd_pack_conv_weight(run.ptr(src), run.ptr(dst), cout, cin, k, cout_pad, cin, run.stream()), "dmd_pack_conv_weight")
    return dst


def pack_f16(run, keep, w):
    cout, cin, k, _ = w.shape
    src, dst = run.put(w), run.put(np.zeros((cin // 16) * k * k * 2 * cout * 16, dtype=np.float16))
    keep += [src, dst]
    check(run, run.lib().dmd_pack_conv_weight_f16x2(run.ptr(src), run.ptr(dst), cout, cin, k, cin, run.stream()), "dmd_pack_conv_weight_f16x2")
    return dst


def launch_conv(run, srcs, w, bias, *, precision=0, w16=False, residual=None, residual_norm=None, want_stats=False, proj=None,
                expect=None):
    """dmd_conv2d.  srcs: [(x NHWC float32, prologue, dmd_norm builder or None)]; residual_norm: an Act whose x is the residual;
    proj: (j0, j1, wp, bp).  Returns (out NHWC, out_stats or None)."""
    L, keep = run.lib(), []
    n, h, wd, _ = srcs[0][0].shape
    cout, cin, k, _ = w.shape
    p = nv.ConvParams()
    p.N, p.H, p.W, p.Cout, p.CoutPad, p.taps, p.stride, p.upsample, p.nsrc, p.precision = n, h, wd, cout, cout, k * k, 1, 0, len(srcs), precision
    for i, (x, prologue, norm) in enumerate(srcs):
        xd = run.put(x)
        keep.append(xd)
        p.src[i].x, p.src[i].C, p.src[i].prologue = run.ptr(xd), x.shape[-1], prologue
        if prologue:
            p.src[i].norm = norm(run, keep)
    bd = run.put(bias)
    keep.append(bd)
    p.w, p.bias = run.ptr(pack_f32(run, keep, w, cout)), run.ptr(bd)
    if w16:
        p.w_f16 = run.ptr(pack_f16(run, keep, w))
    if residual is not None:
        rd = run.put(residual)
        keep.append(rd)
        p.residual = run.ptr(rd)
    if residual_norm is not None:
        rd = run.put(residual_norm.x)
        keep.append(rd)
        p.residual = run.ptr(rd)
        p.residual_norm = act_norm(run, keep, residual_norm)
    if proj is not None:
        j0, j1, wp, bp = proj
        hs = [run.put(j0), run.put(j1), run.put(bp)]
        keep += hs
        p.proj_nsrc, p.proj_C[0], p.proj_C[1] = 2, 64, 64
        p.proj_x[0], p.proj_x[1], p.proj_w_f16, p.proj_bias = run.ptr(hs[0]), run.ptr(hs[1]), run.ptr(pack_f16(run, keep, wp)), run.ptr(hs[2])
    out = run.put(nan_like((n, h, wd, cout)))
    st = run.put(nan_like((n, cout // 32, L.dmd_conv_stat_tiles(h, wd), 2), np.float64)) if want_stats else None
    p.out, p.out_stats = run.ptr(out), run.ptr(st)
    if expect is not None:
        buf = (C.c_char * 96)()
        check(run, L.dmd_conv2d_kernel_name(p, buf, 96), "dmd_conv2d_kernel_name")
        assert buf.value.decode() == expect, buf.value
    check(run, L.dmd_conv2d(p, run.stream()), "dmd_conv2d")
    return run.get(out), (run.get(st) if want_stats else None)


# ---- dmd_conv2d_wgrad ----------------------------------------------------------------------------------------------------------------
def launch_wgrad(run, c, cout, taps, precision, prologue=0, norm=None, defer_into=None):
    """dmd_conv2d_wgrad on a wgrad_cases.Case -> (dw, db); defer_into = (job, dw handle, db handle or None): defer_reduce = 1, the
    job filled by dmd_wgrad_job, its partials kept alive by the returned handle"""
    L, keep = run.lib(), []
    n, h, w, cin = c.x.shape
    p = nv.WgradParams()
    p.N, p.H, p.W, p.Cout, p.taps, p.cin_real, p.precision = n, h, w, cout, taps, c.cin_real, precision
    if c.valid is not None:
        p.valid_h, p.valid_w = c.valid
    hx, hdy = run.put(c.x), run.put(c.dy)
    p.src.x, p.src.C, p.src.prologue, p.dy = run.ptr(hx), cin, prologue, run.ptr(hdy)
    if prologue:
        p.src.norm = norm(run, keep)
    if defer_into is not None:
        job, hdw, hdb = defer_into
        p.dw, p.dbias, p.defer_reduce = run.ptr(hdw), run.ptr(hdb), 1
        check(run, L.dmd_wgrad_job(p, job), "dmd_wgrad_job")
        ws = run.put(nan_like(job.num_wg * (job.NB * job.NCO * 256 + job.NCO * 16)))
        p.workspace = job.partials = run.ptr(ws)
        check(run, L.dmd_conv2d_wgrad(p, run.stream()), "dmd_conv2d_wgrad")
        return ws, (hx, hdy, keep)
    hdw, hdb = run.put(nan_like((cout, c.cin_real, c.k, c.k))), run.put(nan_like(cout))
    ws = run.put(nan_like(int(L.dmd_wgrad_workspace_floats(p))))
    p.workspace, p.dw, p.dbias = run.ptr(ws), run.ptr(hdw), run.ptr(hdb)
    check(run, L.dmd_conv2d_wgrad(p, run.stream()), "dmd_conv2d_wgrad")
    return run.get(hdw), run.get(hdb)


# ---- dmd_gn_silu_bwd -----------------------------------------------------------------------------------------------------------------
def launch_gn_silu_bwd(run, a, da, dskip=None, valid=False):
    """dmd_gn_silu_bwd on an activation of the cases file (valid: with its W / valid_h / valid_w) -> (dx, dmul, dadd)"""
    L, keep = run.lib(), []
    n, hw, c = a.n, a.h * a.w, a.c
    p = nv.GnBwdParams()
    p.N, p.HW, p.C, p.identity_activation = n, hw, c, 0
    if valid:
        p.W, p.valid_h, p.valid_w = a.w, a.hv, a.wv
    hs = [run.put(t) for t in (a.x, da, dskip)]
    outs = [run.put(nan_like(a.x.shape)), run.put(nan_like((n, c))), run.put(nan_like((n, c)))]
    ws = run.put(np.zeros(int(L.dmd_gn_bwd_workspace_bytes(n, hw, c)), dtype=np.uint8))
    p.x, p.norm, p.da, p.dskip = run.ptr(hs[0]), act_norm(run, keep, a), run.ptr(hs[1]), run.ptr(hs[2])
    p.dx, p.workspace, p.dmul, p.dadd = run.ptr(outs[0]), run.ptr(ws), run.ptr(outs[1]), run.ptr(outs[2])
    check(run, L.dmd_gn_silu_bwd(p, run.stream()), "dmd_gn_silu_bwd")
    return tuple(run.get(o) for o in outs)


# ---- dmd_lowres_chain / dmd_lowres_chain32 -------------------------------------------------------------------------------------------
def launch_lowres_chain(run, x, blocks, pack=pack_f16):
    """The 8x8 chain of `blocks` on x (N, 8, 8, C), C = 64 (dmd_lowres_chain: the input kept in slot 0) or 32 (dmd_lowres_chain32:
    no slots).  A block is a dict: cat (its input is cat(x, slot 1), with the projection wp / bp), attn (wqkv / bqkv / wo / bo /
    gam / bet), save (slot or -1), OIHW weights w1 / w2, biases b1 / b2 and FiLM rows f1 / f2 = (mul, add), each (N, channels);
    the rows become the columns of one table in block order.  pack(run, keep, w): an OIHW weight -> the handle of its split-fp16
    pack"""
    n, c, keep = x.shape[0], x.shape[-1], []
    cols, table = [], []

    def column(v):  # (N, m) -> its first column in the FiLM table
        cols.append(sum(t.shape[1] for t in table))
        table.append(v)
        return cols[-1]

    p = nv.LowresChainParams()
    p.N, p.nblocks, p.input_save_slot = n, len(blocks), (0 if c == 64 else -1)
    for i, b in enumerate(blocks):
        cb = p.blocks[i]
        cb.skip_slot, cb.save_slot, cb.has_attn = (1 if b["cat"] else -1), b["save"], int(b["attn"])
        o_mul, o_add = column(b["f1"][0]), column(b["f1"][1])
        cb.film1_mul[0], cb.film1_add[0], cb.film1_mul[1], cb.film1_add[1] = o_mul, o_add, o_mul + c, o_add + c
        cb.film2_mul, cb.film2_add = column(b["f2"][0]), column(b["f2"][1])
        hb = {key: run.put(b[key]) for key in ("b1", "b2", "bp", "gam", "bet", "bqkv", "bo") if key in b}
        keep.append(hb)
        cb.w1, cb.w2, cb.b1, cb.b2 = run.ptr(pack(run, keep, b["w1"])), run.ptr(pack(run, keep, b["w2"])), run.ptr(hb["b1"]), run.ptr(hb["b2"])
        if b["cat"]:
            cb.wproj, cb.bproj = run.ptr(pack(run, keep, b["wp"])), run.ptr(hb["bp"])
        if b["attn"]:
            cb.wq, cb.wk, cb.wv = (run.ptr(pack(run, keep, np.ascontiguousarray(b["wqkv"][j * c:(j + 1) * c]))) for j in range(3))
            cb.wo = run.ptr(pack(run, keep, b["wo"]))
            cb.gn_gamma, cb.gn_beta, cb.bqkv, cb.bo = run.ptr(hb["gam"]), run.ptr(hb["bet"]), run.ptr(hb["bqkv"]), run.ptr(hb["bo"])
    tab = np.ascontiguousarray(np.concatenate(table, axis=1))
    hx, ht, out = run.put(x), run.put(tab), run.put(nan_like(x.shape))
    p.x, p.out, p.table, p.table_stride = run.ptr(hx), run.ptr(out), run.ptr(ht), tab.shape[1]
    check(run, (run.lib().dmd_lowres_chain if c == 64 else run.lib().dmd_lowres_chain32)(p, run.stream()), "dmd_lowres_chain")
    return run.get(out)


# ---- dmd_linear ----------------------------------------------------------------------------------------------------------------------
def _aligned(run, storage, offset):
    """(handle, address of storage[0]): a flat copy of `storage` behind `offset` floats of NaN in a buffer that begins on a 16-byte
    boundary (its length rounded up to 4 floats, NaN as well, so that both runners place it so: at most 3 floats of slack before
    the interpreter's fence)"""
    flat = storage.reshape(-1)
    buf = nan_like(-(-(offset + flat.size) // 4) * 4)
    buf[offset:offset + flat.size] = flat
    h = run.put(buf)
    assert run.ptr(h) % 16 == 0
    return h, run.ptr(h) + 4 * offset


def linear(run, a, w, bias=None, c0=None, silu=False, trans_a=False, trans_w=False, pad=(0, 0, 0), offset=(0, 0), status=False):
    """dmd_linear on the LOGICAL operands a (M, K), w (N, K) -> (C (M, N), the storage of C (M, N + pad[2])).  An operand is laid
    out K-contiguous as (rows, K + pad) or, transposed, as (K, rows + pad) -- with a pad also one more row beyond K --, the pad
    floats of lda / ldw / ldc NaN: no instance may read them.  offset = (floats of A, of W) past a 16-byte boundary at which the
    operand's first element sits.  c0 (M, N): C starts as it and the call accumulates; otherwise C starts as NaN."""
    a, w = np.asarray(_array(a), dtype=np.float32), np.asarray(_array(w), dtype=np.float32)
    (m, k), n = a.shape, w.shape[0]
    assert w.shape[1] == k

    def lay(x, trans, extra):
        st = nan_like((k + (extra > 0), x.shape[0] + extra) if trans else (x.shape[0], k + extra))
        if trans:
            st[:k, :x.shape[0]] = x.T
        else:
            st[:, :k] = x
        return st, st.shape[1]

    (sa, lda), (sw, ldw) = lay(a, trans_a, pad[0]), lay(w, trans_w, pad[1])
    (ha, pa), (hw, pw) = _aligned(run, sa, offset[0]), _aligned(run, sw, offset[1])
    sc = nan_like((m, n + pad[2]))
    if c0 is not None:
        sc[:, :n] = _array(c0)
    hb, hc = run.put(None if bias is None else np.asarray(_array(bias), dtype=np.float32)), run.put(sc)
    p = nv.LinearParams()
    p.M, p.N, p.K, p.A, p.lda, p.W, p.ldw, p.bias, p.C, p.ldc = m, n, k, pa, lda, pw, ldw, run.ptr(hb), run.ptr(hc), n + pad[2]
    p.accumulate, p.silu, p.trans_a, p.trans_w = int(c0 is not None), int(silu), int(trans_a), int(trans_w)
    rc = run.lib().dmd_linear(C.byref(p), run.stream())

    def outs(keep=(ha, hw, hb)):  # (the operands stay alive until the result is back)
        st = run.get(hc)
        return np.ascontiguousarray(st[:, :n]), st

    return _finish(run, rc, "dmd_linear", status, outs)


# ---- dmd_lstm_pointwise / dmd_lstm_pointwise_bwd -------------------------------------------------------------------------------------
def lstm_pointwise(run, gates, c_prev):
    """gates (N, 4 Hd) in i, f, g, o order, c_prev (N, Hd) -> (h, c)"""
    n, hd = c_prev.shape
    hg, hc = run.put(np.asarray(_array(gates), dtype=np.float32)), run.put(np.asarray(_array(c_prev), dtype=np.float32))
    h, c = run.put(nan_like((n, hd))), run.put(nan_like((n, hd)))
    check(run, run.lib().dmd_lstm_pointwise(run.ptr(hg), run.ptr(hc), run.ptr(h), run.ptr(c), n, hd, run.stream()), "dmd_lstm_pointwise")
    return run.get(h), run.get(c)


def lstm_pointwise_bwd(run, gates, c_prev, c_new, dh, dc):
    """-> (dgates (N, 4 Hd), dc_prev (N, Hd)); dh / dc may be None (the kernel's NULL: a zero gradient)"""
    n, hd = c_prev.shape
    hs = [run.put(None if x is None else np.asarray(_array(x), dtype=np.float32)) for x in (gates, c_prev, c_new, dh, dc)]
    dg, dcp = run.put(nan_like((n, 4 * hd))), run.put(nan_like((n, hd)))
    check(run, run.lib().dmd_lstm_pointwise_bwd(*(run.ptr(x) for x in hs), run.ptr(dg), run.ptr(dcp), n, hd, run.stream()),
          "dmd_lstm_pointwise_bwd")
    return run.get(dg), run.get(dcp)
