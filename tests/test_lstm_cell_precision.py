"""The LSTM cell's numerics away from benign gates: dmd_lstm_pointwise and dmd_lstm_pointwise_bwd (every step of LstmStepFn,
LstmHeadsFn, LstmBurnInFn and LstmSegmentFn), on the SIMT interpreter and on the device (-m gpu), through the same C ABI
(tests/abi.py), the same inputs and the same assertions; and one composed case, LstmSegmentFn against torch.nn.LSTM in float64.

Inputs, truth, stick and metric: tests/lstm_cases.py.  ratio = |got - float64 truth| / (2^-24 scale + 2^-126) per element, the
scale the UNCANCELLED one of its output.  Limit: 4 x the largest ratio of the float32 formula in numpy for that (arm, family,
output) over all shapes, never above 32.  The backward gets c as the float32 rounding of the float64 cell state.

Exact: dh = dc = 0 rows give dgates = dc_prev = 0; dh = NULL gives dg_o = 0; gates of +-200 give c = f c_prev + i g with f, i in
{0, 1} and g = +-1, h = +-o where |c| >= 20, dgates = 0 and dc_prev = f dc there; a NaN gate at (row, k) reaches the outputs of
(row, k) that depend on that gate and nothing else.
"""
import numpy as np
import pytest
import torch

from tests import abi
from tests import lstm_cases as LS


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check(run, tag, arm, fam, got, truth, scale):
    worst = LS.by_family(fam, {k: LS.ratio(got[k], truth[k], scale[k]) for k in got})
    failed = []
    for (kind, name), v in worst.items():
        lim = LS.limit(arm, kind, name)
        print(f"LSTMPREC {run.name} {tag} {arm} {kind} {name}: ratio {v:.2f} numpy-f32 {LS.stick_table(arm)[(kind, name)]:.2f} limit {lim:.2f}")
        if not v <= lim:
            failed.append((kind, name, v, lim))
    assert all(np.isfinite(v).all() for v in got.values())
    assert not failed, failed


@pytest.mark.parametrize("run,n,hd,arm", abi.arms(abi.Simt, abi.Gpu, [s + (arm,) for s in LS.SHAPES for arm in LS.ARMS]))
def test_cell_per_element(run, n, hd, arm):
    for r in range(LS.launches(n)):
        gates, cp, dh, dc, fam = LS.inputs(n, hd, r)
        tag = f"{n}x{hd} r{r}"
        truth, scale = LS.forward64(gates, cp)
        h, c = abi.lstm_pointwise(run, gates, cp)
        check(run, tag, arm, fam, dict(h=h, c=c), truth, scale)
        c_new = truth["c"].astype(np.float32)
        dh_, dc_ = LS.arm_grads(arm, dh, dc)
        dg, dcp = abi.lstm_pointwise_bwd(run, gates, cp, c_new, dh_, dc_)
        got = dict(LS.split_dgates(dg), dc_prev=dcp)
        check(run, tag, arm, fam, got, *LS.backward64(gates, cp, c_new, dh_, dc_))
        # exact values
        if arm == "dh-none":
            assert bool((got["dg_o"] == 0).all()), "dh = NULL: dg_o is not 0"
        g4 = gates.reshape(n, 4, hd)
        for j, kind in enumerate(fam):
            if kind == "zero":
                assert bool((dg[j] == 0).all()) and bool((dcp[j] == 0).all()), "dh = dc = 0: a gradient is not 0"
            if kind == "huge":
                i01, f01, o01 = ((g4[j, q] > 0).astype(np.float32) for q in (0, 1, 3))
                c_want = f01 * cp[j] + i01 * np.sign(g4[j, 2])  # 0, +-1, +-60, +-59, +-61: exact in float32
                assert bool((bits(c[j]) == bits(c_want)).all()), "gates of +-200: c is not f c_prev + i g of the exact limits"
                far = np.abs(c_want) >= 20
                assert bool((h[j][far] == (o01 * np.sign(c_want))[far]).all())
                assert bool((dg[j] == 0).all()), "gates of +-200: a gate gradient is not 0"
                dc_want = f01 * (np.zeros(hd, dtype=np.float32) if dc_ is None else dc_[j])
                assert bool((dcp[j][far] == dc_want[far]).all())


@pytest.mark.parametrize("run", abi.RUNNERS)
def test_nan_gate_reaches_its_own_element_only(run):
    n, hd = 5, 103
    gates, cp, dh, dc, _ = LS.inputs(n, hd, 0)
    truth, _ = LS.forward64(gates, cp)
    c_new = truth["c"].astype(np.float32)
    clean_f = abi.lstm_pointwise(run, gates, cp)
    clean_b = {arm: abi.lstm_pointwise_bwd(run, gates, cp, c_new, *LS.arm_grads(arm, dh, dc)) for arm in LS.ARMS}
    for gate, (row, k) in enumerate([(0, 0), (4, 102), (2, 51), (3, 7)]):
        g = gates.copy()
        g[row, gate * hd + k] = np.nan
        want, _ = LS.forward64(g, cp)
        for got, clean, name in zip(abi.lstm_pointwise(run, g, cp), clean_f, ("h", "c")):
            poisoned = np.isnan(want[name])
            assert poisoned.sum() == (0 if (gate == 3 and name == "c") else 1)
            assert bool((np.isnan(got) == poisoned).all()) and bool((bits(got)[~poisoned] == bits(clean)[~poisoned]).all()), (gate, name)
        for arm in LS.ARMS:
            dh_, dc_ = LS.arm_grads(arm, dh, dc)
            dg, dcp = abi.lstm_pointwise_bwd(run, g, cp, c_new, dh_, dc_)
            wb, _ = LS.backward64(g, cp, c_new, dh_, dc_)
            got, clean = dict(LS.split_dgates(dg), dc_prev=dcp), dict(LS.split_dgates(clean_b[arm][0]), dc_prev=clean_b[arm][1])
            for name in LS.BACKWARD:
                poisoned = np.isnan(wb[name])
                assert poisoned.sum() <= 1 and not poisoned[np.arange(n) != row].any()
                assert bool((np.isnan(got[name]) == poisoned).all()), (gate, arm, name)
                assert bool((bits(got[name])[~poisoned] == bits(clean[name])[~poisoned]).all()), (gate, arm, name)


# ---- composed: LstmSegmentFn forward and backward against torch.nn.LSTM in float64 -----------------------------------------------------
def _segment_case():
    t, b, hd = 6, 5, 16
    g = torch.Generator().manual_seed(23)
    gx = 1.5 * torch.randn(t, b, 4 * hd, generator=g)
    gx[1], gx[4] = 6.0 * torch.randn(b, 4 * hd, generator=g), 6.0 * torch.randn(b, 4 * hd, generator=g)  # saturated steps
    w_hh, b_hh = torch.randn(4 * hd, hd, generator=g) / hd ** 0.5, 0.3 * torch.randn(4 * hd, generator=g)
    dys = torch.randn(t, b, hd, generator=g)
    return gx, w_hh, b_hh, dys


def _torch_lstm(dtype):
    """nn.LSTM whose input projection is the identity (W_ih = I, b_ih = 0), so that its input IS gx: (ys, dgx, dW_hh, db_hh)"""
    gx, w_hh, b_hh, dys = _segment_case()
    hd = w_hh.shape[1]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        lstm = torch.nn.LSTM(4 * hd, hd).to(dtype)
        with torch.no_grad():
            lstm.weight_ih_l0.copy_(torch.eye(4 * hd))
            lstm.bias_ih_l0.zero_()
            lstm.weight_hh_l0.copy_(w_hh)
            lstm.bias_hh_l0.copy_(b_hh)
        x = gx.to(dtype).requires_grad_()
        ys, _ = lstm(x)
        ys.backward(dys.to(dtype))
        return [v.detach().double() for v in (ys, x.grad, lstm.weight_hh_l0.grad, lstm.bias_hh_l0.grad)]
    finally:
        torch.set_num_threads(threads)


def _row_errors(got, truth):
    """max |got - truth| of a row / the row's root-sum-square, rows = the last dimension (a vector is one row)"""
    got, truth = got.double().reshape(-1, got.shape[-1]), truth.reshape(-1, truth.shape[-1])
    return (got - truth).abs().amax(dim=1) / truth.pow(2).sum(dim=1).sqrt()


def _check_segment(name, got):
    truth, stick = _torch_lstm(torch.float64), _torch_lstm(torch.float32)
    failed = []
    for what, g, t, s in zip(("ys", "dgx", "dW_hh", "db_hh"), got, truth, stick):
        e, e32 = float(_row_errors(g, t).max()), float(_row_errors(s, t).max())
        lim = 4 * max(e32, 2.0 ** -24)  # (a stick below one rounding of the row's scale is an accident, not a measure)
        print(f"LSTMPREC {name} segment T=6 B=5 hd=16 {what}: err {e:.3e} torch-f32 {e32:.3e} limit {lim:.3e}")
        assert bool(torch.isfinite(g).all())
        if not e <= lim:
            failed.append((what, e, lim))
    assert not failed, failed


def _run_segment(device):
    from diamond_amd import engine as E
    from diamond_amd import lstm_native as LN

    gx, w_hh, b_hh, dys = _segment_case()
    gx, w_hh, b_hh = (v.to(device).requires_grad_() for v in (gx, w_hh, b_hh))
    ys = LN.LstmSegmentFn.apply(E.PackCache(), gx, w_hh, b_hh)
    dgx, dw, db = torch.autograd.grad(ys, [gx, w_hh, b_hh], dys.to(device))
    return [v.detach().cpu() for v in (ys, dgx, dw, db)]


def test_segment_against_float64_lstm_interpreter():
    from tests.simt.host_harness import engine_on_interpreter

    with engine_on_interpreter():
        got = _run_segment("cpu")
    _check_segment("simt", got)


@pytest.mark.gpu
def test_segment_against_float64_lstm_gpu():
    _check_segment("gpu", _run_segment("cuda"))
