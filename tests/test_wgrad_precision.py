"""The weight-gradient kernels' numerics away from benign N(0, 1) dy: dmd_conv2d_wgrad's nine instances on its three routes --
exact (wgrad_kernel<G, false>), split-fp16 on the producer / consumer kernel (wgrad_ps_kernel) and on the single-role kernel
(wgrad_kernel<G, true>, DIAMOND_WGRAD_PS=0) --, the reductions (wgrad_reduce1/2_kernel, wgrad_reduce_jobs_kernel with its per-job
scale) and the host's grad_ops.pow2_scaled, on the SIMT interpreter and on the device (-m gpu), through the same C ABI, the same
inputs and the same assertions.  Outputs start as NaN.

Inputs (tests/wgrad_cases.py): a family per 16-channel block of dy and per 16-channel block of the source, see there.
Truth: the sum in float64 over the float32 inputs.  Stick: float32 F.conv2d autograd on the CPU.
Error: max |got - truth| / max |truth| per (output channel, 16-channel source block) ROW of dw -- a whole-tensor maximum hides a
small output channel behind the launch's largest one.  db: per channel, against max(|truth|, sqrt(sum dy^2)): LOOSER than the
channel's own |truth| exactly where a zero-mean sum happens to cancel (a single element has no row to take a maximum over), the
same thing for a coherent sum.  The stick runs on one thread: torch's order of summation moves with the thread count.

Bounds
  exact route   err <= K_BWD max(err_fp32, 2^-24) on every row of every family.
  split routes  the same plus the operand contract's allowance (include/diamond_hip.h, dmd_wgrad_params.precision), derived, not
                measured: A = sum_pixels e(dy) |a| + |dy| e(a) + e(dy) e(a), e(x) = max(2^-22 |x|, 2^-25), largest element of the
                row over the row's max |truth|.  Rows whose dy channel is at >= 2^-3 of O(1) meet the plain bound WITHOUT it
                (test_split_floor_begins_below_2_to_minus_3 pins that edge from the arithmetic alone, no kernel).
  exact values  wherever no product reaches an element (a tap that looks into the zero padding, nothing an impulse meets, anything
                beyond the valid extent) both routes return exactly 0 (either sign); where ONE product reaches it the exact route
                returns float32(dy a) bitwise, the split routes that product within its two operands' contract -- 2^-21 |dy a|
                where both are in the contract's relative range, |x| >= 2^-3.
  non-finite    exact: finite exactly where the truth is.  split: a finite operand beyond fp16 (1e5) splits into h = inf, l = -inf:
                a dy entry makes its whole ROW co of dw NaN, a source entry its whole COLUMN ci, every other row and column is
                finite and inside the bound, db is the finite raw sum -- never a finite wrong number.  NaN / Inf operands: non-finite
                on the rows and columns where the truth is, nowhere else.

What the interpreter cannot reproduce: the order of the sums inside an MFMA is its own, so the split rows differ between the
runners by small factors (profiles/wgrad_precision.txt has both)."""
import functools
import math

import numpy as np
import pytest
import torch

from diamond_amd import native as nv  # struct layouts only
from tests import groupnorm_cases as GC
from tests import wgrad_cases as WC
from tests.abi import RUNNERS, check, kernel_sums, launch_wgrad, nan_like, norm_struct
from tests.groupnorm_cases import FLOOR_EXACT, K_BWD, rows_errors

SITES = [(2, 1, 9), (4, 1, 9), (1, 4, 9), (2, 2, 9), (4, 2, 9), (4, 4, 9), (4, 2, 1), (2, 2, 1), (4, 4, 1)]
SITE_IDS = ["%d-%d-%d" % s for s in SITES]
# route -> (dmd_wgrad_params.precision, DIAMOND_WGRAD_PS)
ROUTES = {"exact": (0, None), "ps": (1, None), "split": (1, 0)}
SHAPES = [(3, 8, 8), (3, 8, 16)]  # 3 sub-tiles (the last tile half empty, its first half shared by two images) / 6 sub-tiles


def T(a):
    """a tensor copy of a (possibly read-only) array"""
    return torch.tensor(np.asarray(a))


def check_case(run, tag, c, nci, dw, db, route, plain_rows=None):
    """print the figures of the worst row of every (dy block, source block) pair, then assert everything the module's docstring
    states.  plain_rows: a mask over the output channels whose rows must meet the bound without the split allowance."""
    split = route != "exact"
    truth, stick = T(c.truth), c.stick
    got = torch.from_numpy(np.ascontiguousarray(dw))
    rows = functools.partial(WC.block_rows, nci=nci)
    e, e32 = rows_errors(rows(got), rows(truth)), rows_errors(rows(stick), rows(truth))
    scale = torch.where(torch.isfinite(rows(truth)), rows(truth).abs(), torch.zeros_like(rows(truth))).amax(dim=1)
    rel = lambda t: torch.where(scale > 0, rows(T(t)).amax(dim=1) / scale.clamp_min(1e-300), torch.zeros_like(scale))
    allow, rss = rel(c.allow), rel(c.rss)
    plain = K_BWD * torch.clamp(e32, min=FLOOR_EXACT)
    limit = plain + allow if split else plain
    if plain_rows is not None:
        limit = torch.where(T(np.repeat(plain_rows, nci)), plain, limit)
    used = e / limit
    cout = dw.shape[0]
    per = used.reshape(cout // 16, 16, nci).permute(0, 2, 1).reshape(-1, 16)
    for b in range(per.shape[0]):
        j = ((b // nci) * 16 + int(per[b].argmax())) * nci + b % nci
        print(f"WGPREC {run.name} {tag} {route} dy={c.dy_kinds[b // nci] if c.dy_kinds else '-'} src={c.src_kinds[b % nci] if c.src_kinds else '-'}: "
              f"err {float(e[j]):.3e} fp32 {float(e32[j]):.3e} ratio {float(e[j] / max(float(e32[j]), FLOOR_EXACT)):.2f} limit {float(limit[j]):.3e} "
              f"of-A {float(e[j] / allow[j]) if float(allow[j]) > 0 else 0.0:.3f} of-rss {float(e[j] / rss[j]) if float(rss[j]) > 0 else 0.0:.2f}")
    # finiteness
    bad = ~torch.isfinite(truth)
    if split:
        bad = bad | T(c.big_rows)[:, None, None, None] | T(c.big_cols)[None, :, None, None]
    wrong = torch.isfinite(got) == bad
    assert not bool(wrong.any()), f"{int(wrong.sum())} elements of dw are finite where they must not be, or the reverse: rows {sorted(set(torch.nonzero(wrong)[:, 0].tolist()))}"
    assert float(used.max()) <= 1.0, (float(used.max()), int(used.argmax()) // nci, int(used.argmax()) % nci)
    # exact values
    clean = ~(T(c.bad_rows | (c.big_rows if split else False))[:, None, None, None] |
              T(c.bad_cols | (c.big_cols if split else False))[None, :, None, None])
    none, one = clean & T(c.count == 0), clean & T(c.count == 1)
    assert bool((got[none] == 0).all()), f"{int((got[none] != 0).sum())} elements no product reaches are not zero"
    if split:
        # the product of two split operands as the kernels form it, l l + h l + l h + h h: each operand's contract, and four fp32
        # roundings of the accumulator
        d = (got[one].double() - truth[one]).abs()
        assert bool((d <= T(c.allow)[one] + 4 * 2.0 ** -24 * truth[one].abs()).all())
        print(f"WGPREC {run.name} {tag} {route} single products: {int(one.sum())}, worst {single_product_ratio(c, got, split):.3f} x 2^-21 |dy a|")
    else:
        assert bool((got[one] == truth[one].float()).all()), "a single product is not float32(dy * a)"
    # db: the raw dy, fp32, on every route.  Per channel, against max(|truth|, sqrt(sum dy^2)): a sum of N(0, 1) values that
    # happens to cancel (|truth| far below the root-sum-square its terms make) is held to the accuracy of that scale, as any order
    # of fp32 additions is; a coherent sum (family 4: |truth| = sum |dy|) is held to its own value.
    gdb, tdb, sdb = T(db).double(), T(c.truth_db), T(c.scale_db)
    err_of = lambda v: torch.where(torch.isfinite(v - tdb), (v - tdb).abs(), torch.zeros_like(tdb)) / sdb.clamp_min(1e-300)
    eb, eb32 = err_of(gdb), err_of(c.stick_db.double())
    lim = K_BWD * torch.clamp(eb32, min=FLOOR_EXACT)
    j = int((eb / lim).argmax())
    print(f"WGPREC {run.name} {tag} {route} db: err {float(eb[j]):.3e} fp32 {float(eb32[j]):.3e} limit {float(lim[j]):.3e} (channel {j})")
    assert bool((torch.isfinite(gdb) == torch.isfinite(tdb)).all()), "db is not finite exactly where the raw sum is"
    assert float((eb / lim).max()) <= 1.0, (j, float(eb[j]), float(lim[j]))
    assert bool((gdb[sdb == 0] == 0).all())
    gdb, tdb = gdb[:, None], tdb[:, None]
    lone = T(c.count_db == 1)  # a channel whose dy is one impulse: db is that value
    assert bool((gdb[lone, 0] == tdb[lone, 0].float()).all())
    return e, limit


def single_product_ratio(c, got, split):
    """largest |got - dy a| / (2^-21 |dy a|) over the elements of dw that ONE product reaches, both operands in the contract's
    relative range (2^-3 <= |x| < 65520) and their row and column free of non-finite operands"""
    clean = ~(T(c.bad_rows | (c.big_rows if split else False))[:, None, None, None] | T(c.bad_cols | (c.big_cols if split else False))[None, :, None, None])
    both = clean & T(c.count == 1) & T(c.count_rel == 1)
    truth = T(c.truth)
    if not bool(both.any()):
        return 0.0
    return float(((got[both].double() - truth[both]).abs() / (2.0 ** -21 * truth[both].abs())).max())


def floor_free_rows(c):
    """output channels of the channel-scale families at >= 2^-3 of O(1), and every channel of a benign block"""
    m = np.zeros(16 * len(c.dy_kinds), dtype=bool)
    for b, kind in enumerate(c.dy_kinds):
        if kind in WC.CHAN_SCALE:
            m[16 * b:16 * b + 16] = WC.CHAN_SCALE[kind](np.arange(16)) >= 0.125
        elif kind == "benign":
            m[16 * b:16 * b + 16] = True
    return m


# ---- the nine instances, raw source --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", WC.ARMS)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("site", SITES, ids=SITE_IDS)
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_families(run, site, route, arm, dmd_env):
    """every family through every instance and route, N = 3 at 8x8 and 8x16, the default plan"""
    nco, nci, taps = site
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=None)
    for n, h, w in SHAPES:
        for r in range(WC.launches(arm, nco, nci)):
            c = WC.case(arm, nco, nci, taps, n, h, w, r)
            dw, db = launch_wgrad(run, c, 16 * nco, taps, precision)
            e, _ = check_case(run, f"<{nco},{nci},{taps}> {h}x{w} arm={arm}/{r}", c, nci, dw, db, route,
                              plain_rows=floor_free_rows(c) if arm == "scales" else None)
            for b, kind in enumerate(c.dy_kinds):  # the table of include/diamond_hip.h: error per channel scale, source block 0
                if kind in WC.CHAN_SCALE and c.src_kinds[0] == "benign":
                    per = " ".join(f"{float(e[(16 * b + ch) * nci]):.1e}" for ch in range(16))
                    print(f"WGPREC {run.name} <{nco},{nci},{taps}> {h}x{w} {route} per-scale {kind} c=0..15: {per}")


PLAN_SITES = [(2, 1, 9), (2, 2, 9), (4, 4, 9), (4, 2, 1)]


@pytest.mark.parametrize("max_wg", [1, 2])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("site", PLAN_SITES, ids=["%d-%d-%d" % s for s in PLAN_SITES])
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_plans(run, site, route, max_wg, dmd_env):
    """DIAMOND_WGRAD_MAX_WG = 1 (one accumulator chain over the three tiles of N = 3 at 8x16) and 2 (two tiles + one); the default
    plan -- one tile per workgroup -- is test_wgrad_families'"""
    nco, nci, taps = site
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=max_wg)
    for arm in ("scales", "sparse", "checker", "coherent"):
        c = WC.case(arm, nco, nci, taps, 3, 8, 16, 0)
        dw, db = launch_wgrad(run, c, 16 * nco, taps, precision)
        check_case(run, f"<{nco},{nci},{taps}> 8x16 max_wg={max_wg} arm={arm}/0", c, nci, dw, db, route,
                   plain_rows=floor_free_rows(c) if arm == "scales" else None)


# ---- impulses and the valid extent --------------------------------------------------------------------------------------------------
EXTENT_SITES = [(2, 1, 9), (2, 2, 9), (4, 4, 9)]


@pytest.mark.parametrize("valid", [None, (15, 13)], ids=["full", "valid15x13"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("site", EXTENT_SITES, ids=["%d-%d-%d" % s for s in EXTENT_SITES])
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_impulses_and_valid_extent(run, site, route, valid, dmd_env):
    """N = 3 at 16x16 (the seam impulses of image 2 exist): every element of dw an impulse reaches is ONE product, every other an exact
    zero.  With valid_h, valid_w = 15, 13 the margins of x and dy are NaN and hold impulses just outside the extent: they contribute
    nothing (a margin that leaked would be a NaN, or the product of an outside impulse where an exact zero belongs)."""
    nco, nci, taps = site
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=None)
    for arm in ("sparse", "checker", "frames3"):
        for r in range(WC.launches(arm, nco, nci)):
            c = WC.case(arm, nco, nci, taps, 3, 16, 16, r, valid, valid is not None)
            assert "impulse" not in c.dy_kinds or int((c.count == 1).sum()) > 0
            dw, db = launch_wgrad(run, c, 16 * nco, taps, precision)
            check_case(run, f"<{nco},{nci},{taps}> 16x16 {'valid15x13' if valid else 'full'} arm={arm}/{r}", c, nci, dw, db, route)


@pytest.mark.parametrize("route", ["ps", "split"])
@pytest.mark.parametrize("site", SITES, ids=SITE_IDS)
@pytest.mark.parametrize("run", RUNNERS)
def test_split_single_product_within_2_to_minus_21(run, site, route, dmd_env):
    """On the split routes an element of dw that a single product reaches is within 2^-21 |dy a| of it (both operands in the
    contract's relative range): every arm with an impulse block, N = 3 at 8x8 and 8x16.

    The bound is the sum of the two operands' contracts, 2 x 2^-22, so it holds only because the kernels sum all four partial
    products: l l alone is up to 2^-11 |dy| x 2^-11 |a| = 2^-22 |dy a| when both operands sit just above a power of two, and a
    kernel that leaves it out measures 1.03 x 2^-21 on <4,2,9> (profiles/wgrad_precision.txt)."""
    nco, nci, taps = site
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=None)
    worst = 0.0
    for arm in ("sparse", "checker", "frames3"):
        for n, h, w in SHAPES:
            for r in range(WC.launches(arm, nco, nci)):
                c = WC.case(arm, nco, nci, taps, n, h, w, r)
                if "impulse" not in c.dy_kinds:
                    continue
                dw, _ = launch_wgrad(run, c, 16 * nco, taps, precision)
                ratio = single_product_ratio(c, torch.from_numpy(np.ascontiguousarray(dw)), True)
                print(f"WGPREC {run.name} <{nco},{nci},{taps}> {h}x{w} arm={arm}/{r} {route} single products: worst {ratio:.3f} x 2^-21 |dy a|")
                worst = max(worst, ratio)
    assert worst <= 1.0, worst


# ---- normalised sources ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normed_case(nco, c_real, c_pad, h, w):
    """a benign activation (N(0.3, 1.5^2), FiLM rows N(0, 0.3^2)) under NORM_SILU, every dy family that needs no partner"""
    rng = np.random.default_rng([7, nco, c_real, h, w])
    n = 3
    x = (rng.standard_normal((n, h, w, c_real)) * 1.5 + 0.3).astype(np.float32)
    mul, add = (rng.standard_normal((n, c_real)) * 0.3).astype(np.float32), (rng.standard_normal((n, c_real)) * 0.3).astype(np.float32)
    kinds = ("chan2", "benign", "pooled", "offset")[:nco]
    dy = np.concatenate([WC.dy_block(kind, rng, n, h, w, h, w) for kind in kinds], axis=-1).astype(np.float32)
    act = lambda dtype: GC.nhwc(GC.norm_act(GC.tt(x, dtype).permute(0, 3, 1, 2), GC.tt(mul, dtype), GC.tt(add, dtype), True, True)).numpy()
    xp = np.zeros((n, h, w, c_pad), dtype=np.float32)
    xp[..., :c_real] = x
    pad = lambda v: np.ascontiguousarray(np.pad(v, ((0, 0), (0, c_pad - c_real))))
    case = WC.Case(xp, dy, 3, c_real, a64=act(torch.float64), a32=act(torch.float32), dy_kinds=kinds, src_kinds=("normed",) * (c_pad // 16))
    return case, np.ascontiguousarray(x), pad(mul), pad(add)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("geom", [(2, 32, 32), (4, 64, 64), (4, 48, 64)], ids=["2-2-9", "4-4-9", "GN-4-4-9-c48"])
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_normalised_source(run, geom, route, dmd_env):
    """NORM_SILU + FiLM on <2,2,9> (the two-workgroups-per-CU shape), <4,4,9> and WgradGeomGN<4,4,9> at 48 real channels (one group of
    48, the source zero-padded to 64).  wgrad_ps_kernel's v_exp / v_rcp SiLU differs from expf in the last bit of an activation: far
    inside the split allowance."""
    nco, c_real, c_pad = geom
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=None)
    c, x, mul, add = normed_case(nco, c_real, c_pad, 8, 16)
    norm = lambda r, keep: norm_struct(r, keep, kernel_sums(r, x), mul, add, True)
    dw, db = launch_wgrad(run, c, 16 * nco, 9, precision, prologue=1, norm=norm)
    check_case(run, f"norm-silu <{nco},{c_pad // 16},9> c={c_real} 8x16", c, c_pad // 16, dw, db, route, plain_rows=floor_free_rows(c))


# ---- where the floor begins: the arithmetic alone ------------------------------------------------------------------------------------
def test_split_floor_begins_below_2_to_minus_3():
    """No kernel: both operands split as wg_pack_hl does, h h + l h + h l + l l summed in float64.  N = 3, 8x16, 32 source channels at
    1.3 N(0, 1) + 0.2, dy channel c at 2^-2c.  Per output channel, against that channel's own max |truth|: rows at >= 2^-3 are
    fp32-class (below K_BWD 2^-24 -- l is a NORMAL fp16 there, the operand error relative), rows at <= 2^-14 are not (l is a
    subnormal, the operand error an absolute 2^-25), and every row stays inside the allowance A of the operand contract."""
    rng = np.random.default_rng(3)
    n, h, w = 3, 8, 16
    x = (1.3 * rng.standard_normal((n, h, w, 32)) + 0.2).astype(np.float32)
    dy = (rng.standard_normal((n, h, w, 16)) * WC.CHAN_SCALE["chan4"](np.arange(16))).astype(np.float32)
    c = WC.Case(x, dy, 3, 32)
    (gh, gl), (ah, al) = WC.split_hl(dy), WC.split_hl(x)
    emu = WC.tap_sums(gh, ah, 3) + WC.tap_sums(gl, ah, 3) + WC.tap_sums(gh, al, 3) + WC.tap_sums(gl, al, 3)
    rows = lambda t: T(t).reshape(16, -1)
    e = rows_errors(rows(emu), rows(c.truth))
    a = rows(c.allow).amax(dim=1) / rows(c.truth).abs().amax(dim=1)
    for ch in range(16):
        print(f"WGPREC emulation channel scale 2^-{2 * ch}: err {float(e[ch]):.3e} of-A {float(e[ch] / a[ch]):.3f}")
    assert bool((e <= a).all()), (e, a)
    assert bool((e[:2] <= K_BWD * FLOOR_EXACT).all()), e[:2]  # 2^0, 2^-2
    assert bool((e[7:13] > K_BWD * FLOOR_EXACT).all()), e[7:13]  # 2^-14 .. 2^-24
    assert float(e[13]) > 0.5  # 2^-26: below half the smallest fp16 subnormal times O(1) -- flushed


# ---- reductions and scaling ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0 ** -40, 2.0 ** 30, 0.3], ids=["2^-40", "2^30", "0.3"])
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_deferred_reduction_scale_slices_and_column_sums(run, scale, dmd_env):
    """defer_reduce = 1 -> dmd_wgrad_job -> dmd_wgrad_reduce_jobs with a device scale: two sources (32 channels on wgrad_ps_kernel,
    15 of 16 on the exact kernel) land in slices [0, 32) and [36, 51) of ONE (32, 56, 3, 3) tensor prefilled with NaN, bitwise the
    undeferred gradient times the scale, the rest of the tensor still NaN; a DMD_REDUCE_COLSUM job in the same launch whose partials
    span 1 .. 2^-30 over n is the float64 sum rounded once (2^-24 relative), times the scale."""
    L = run.lib()
    dmd_env(DIAMOND_WGRAD_PS=None, DIAMOND_WGRAD_MAX_WG=None)
    scale = np.float32(scale)
    hs = run.put(np.array([scale], dtype=np.float32))
    big, dbs = run.put(nan_like((32, 56, 3, 3))), run.put(nan_like(32))
    jobs, keep, want = [], [], []
    for (nci, arm, precision, c0, with_db) in ((2, "scales", 1, 0, True), (1, "frames15", 0, 36, False)):
        c = WC.case(arm, 2, nci, 9, 3, 8, 16, 0)
        dw, db = launch_wgrad(run, c, 32, 9, precision)
        job = nv.WgradReduceJob()
        keep.append(launch_wgrad(run, c, 32, 9, precision, defer_into=(job, big, dbs if with_db else None)))
        assert job.ld_cin == c.cin_real and job.c0 == 0 and job.scale is None and job.kind == nv.REDUCE_WGRAD
        job.ld_cin, job.c0, job.scale = 56, c0, run.ptr(hs)
        jobs.append(job)
        want.append((c0, c.cin_real, dw, db if with_db else None))
    rng = np.random.default_rng(8)
    n, ch = 16, 32
    parts = (rng.standard_normal((2, n, ch)) * (2.0 ** (-2.0 * np.arange(n)))[None, :, None]).astype(np.float32)
    hp, hg, hb = run.put(parts), run.put(nan_like(ch)), run.put(nan_like(ch))
    job = nv.WgradReduceJob()
    job.kind, job.partials, job.dw, job.dbias, job.num_wg, job.cin_real, job.scale = nv.REDUCE_COLSUM, run.ptr(hp), run.ptr(hg), run.ptr(hb), n, ch, run.ptr(hs)
    jobs.append(job)
    table = (nv.WgradReduceJob * len(jobs))(*jobs)
    check(run, L.dmd_wgrad_reduce_jobs(table, len(jobs), run.stream()), "dmd_wgrad_reduce_jobs")
    got, gdb = run.get(big), run.get(dbs)
    touched = np.zeros(56, dtype=bool)
    for c0, cr, dw, db in want:
        assert np.isfinite(dw).all()
        assert np.array_equal(got[:, c0:c0 + cr].view(np.uint32), (dw * scale).view(np.uint32)), "not bitwise (undeferred result) * scale"
        touched[c0:c0 + cr] = True
        if db is not None:
            assert np.array_equal(gdb.view(np.uint32), (db * scale).view(np.uint32))
    assert np.isnan(got[:, ~touched]).all() and int((~touched).sum()) == 9
    sums = np.zeros((2, ch))
    for i in range(n):
        sums += parts[:, i].astype(np.float64)
    for h, s in ((hg, sums[0]), (hb, sums[1])):
        v = run.get(h)
        assert np.array_equal(v.view(np.uint32), (s.astype(np.float32) * scale).view(np.uint32)), "not (float)(fp64 sum) * scale"
        assert bool((np.abs(v.astype(np.float64) / float(scale) - s) <= 2.0 ** -23 * np.abs(s)).all())
        if math.log2(float(scale)) == int(math.log2(float(scale))):  # (a power of two: the division is exact)
            assert bool((np.abs(v.astype(np.float64) / float(scale) - s) <= 2.0 ** -24 * np.abs(s)).all())


# ---- many workgroups, one long chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_two_pass_reduction(run, route, dmd_env):
    """N = 9 at 32x32 on <2,1,9>: 72 tiles, 72 workgroups -- more than the 64 partials one pass takes (wgrad_reduce1_kernel +
    wgrad_reduce2_kernel); offset family."""
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=None)
    c = WC.case("coherent", 2, 1, 9, 9, 32, 32, 0)
    assert c.dy_kinds == ("offset", "benign") and c.src_kinds == ("posit",)
    dw, db = launch_wgrad(run, c, 32, 9, precision)
    check_case(run, "<2,1,9> 9x32x32 two-pass arm=coherent/0", c, 1, dw, db, route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("run", RUNNERS)
def test_wgrad_one_accumulator_chain_of_16384_pixels(run, route, dmd_env):
    """DIAMOND_WGRAD_MAX_WG = 1 at N = 16, 32x32 on <2,1,9>: one workgroup walks all 128 tiles, 16,384 pixels of 1 + 1e-3 N(0, 1)
    against a positive source -- how the error of a coherent sum grows with the chain's length.  An fp32 accumulator collects one
    rounding per MFMA like a random walk, 2^-25 sqrt(n / 3) rms after n of them.  The exact route (one MFMA per 4 pixels) therefore
    moves its accumulators into the workgroup's partial every WGRAD_CHAIN_TILES = 16 tiles: chains of 512 roundings, eight of them
    added up; as ONE chain of 4,096 it measured 4.8e-6 on the MI355X.  The split routes round four times per 32 pixels, 2,048
    in this chain.  The stick runs on one thread (wgrad_cases.stick_f32), where torch's own sum over 16,384 pixels is a long
    chain too (1e-6 .. 2e-6): profiles/wgrad_precision.txt has the rows."""
    precision, ps = ROUTES[route]
    dmd_env(DIAMOND_WGRAD_PS=ps, DIAMOND_WGRAD_MAX_WG=1)
    c = WC.case("coherent", 2, 1, 9, 16, 32, 32, 0)
    dw, db = launch_wgrad(run, c, 32, 9, precision)
    check_case(run, "<2,1,9> 16x32x32 max_wg=1 arm=coherent/0", c, 1, dw, db, route)


# ---- the host: grad_ops.pow2_scaled (CPU, no kernel) ---------------------------------------------------------------------------------
AMAX = [0.0, 1e-45, 1e-40, 2.0 ** -126, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 3e38, math.inf, math.nan]


@pytest.mark.parametrize("amax", AMAX, ids=[repr(float(np.float32(a))) for a in AMAX])
def test_pow2_scaled_edges(amax):
    """(d 2^k, 2^-k): 2^-k is a finite normal number whatever d holds; d 2^k 2^-k is d bitwise wherever neither factor leaves
    the fp32 range; a NaN / Inf stays where it was; zeros stay zeros"""
    from diamond_amd.grad_ops import pow2_scaled

    rng = np.random.default_rng(2)
    d = torch.from_numpy(rng.uniform(-1.0, 1.0, 64).astype(np.float32)) * torch.tensor(amax if math.isfinite(amax) else 1.0, dtype=torch.float32)
    d[7] = torch.tensor(amax, dtype=torch.float32)
    d[9] = 0.0
    s, inv = pow2_scaled(d)
    inv = inv.float()
    assert s.dtype == torch.float32 and bool(torch.isfinite(inv)) and float(inv) >= 2.0 ** -126, float(inv)
    k = math.log2(float(inv))
    assert k == int(k)  # a power of two
    assert bool((torch.isnan(s) == torch.isnan(d)).all()) and bool((torch.isinf(s) == torch.isinf(d)).all())
    assert float(s[9]) == 0.0
    if amax == 0.0:
        assert not bool(s.any())
    back = s * inv
    exact = torch.isfinite(d) & ((s.abs() >= 2.0 ** -126) | (s == 0)) & ((d.abs() >= 2.0 ** -126) | (d == 0) | (s.abs() >= 2.0 ** -126))
    same = (back.view(torch.int32) == d.view(torch.int32)) | (d == 0)
    assert bool(same[exact].all()), (d[exact & ~same], back[exact & ~same])


def test_pow2_scaled_leaves_the_maximum_in_half_to_two():
    """every finite positive amax in [2^-120, 2^120] -- exact powers of two, their two neighbours, and values in between -- is
    scaled into [0.5, 2), and the round trip is bitwise"""
    from diamond_amd.grad_ops import pow2_scaled

    for e in range(-120, 121):
        for m in (1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -22, 1.2345678, 1.5):
            if e == 120 and m > 1.0:
                continue
            a = torch.tensor([m * 2.0 ** e, -0.3 * 2.0 ** e, 0.0], dtype=torch.float32)
            s, inv = pow2_scaled(a)
            assert 0.5 <= float(s.abs().max()) < 2.0, (e, m, float(s.abs().max()))
            assert bool(((s * inv).view(torch.int32) == a.view(torch.int32)).all()), (e, m)
