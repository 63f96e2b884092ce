"""Frame metrics computed on the device.  `frame_ssim`: per-frame SSIM (Wang et al. 2004) of uint8 levels in fp64, one
dmd_frame_ssim call -- the number that drops when a prediction loses local contrast (a blurred average of futures scores well on
MSE / PSNR), which video-prediction reports pair with PSNR.  `open_loop_eval(..., ssim=True)` uses the same entry point against the
replay arena, without an fp32 copy of the targets.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

import torch
from torch import Tensor

from . import native as nv


def ssim_constants(sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> Tuple[Tuple[float, ...], float, float]:
    """(the 11-tap Gaussian window normalised to sum 1, C1 = (k1 * 255)^2, C2 = (k2 * 255)^2), all fp64."""
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"frame_ssim: sigma {sigma}")
    g = [math.exp(-((i - nv.SSIM_TAPS // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(nv.SSIM_TAPS)]
    total = math.fsum(g)
    return tuple(v / total for v in g), (k1 * 255.0) ** 2, (k2 * 255.0) ** 2


def ssim_params(n: int, c: int, h: int, w: int, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> nv.SsimParams:
    """A parameter block with the sizes, the window and the constants filled in (ValueError for sizes the entry refuses)."""
    if h < nv.SSIM_TAPS or w < nv.SSIM_TAPS:
        raise ValueError(f"frame_ssim: frames of {h} x {w}: the window needs {nv.SSIM_TAPS} x {nv.SSIM_TAPS}")
    if not (0 <= n <= 65535 and 1 <= c <= 65535 and h <= 32768 and w <= 32768):
        raise ValueError(f"frame_ssim: N {n} (0 ... 65535), C {c} (1 ... 65535), H {h}, W {w} (11 ... 32768)")
    p = nv.SsimParams()
    p.N, p.C, p.H, p.W = n, c, h, w
    win, p.c1, p.c2 = ssim_constants(sigma, k1, k2)
    p.win[:] = win
    return p


def set_operand(p: nv.SsimParams, which: str, t: Tensor) -> None:
    """Operand `which` ("a" / "b") of `p` <- a contiguous fp32 or uint8 tensor."""
    setattr(p, f"{which}_f32", nv.fptr(t) if t.dtype == torch.float32 else None)
    setattr(p, f"{which}_u8", nv.ptr(t) if t.dtype == torch.uint8 else None)


def ssim_workspace(p: nv.SsimParams, device) -> Tensor:
    return torch.empty(max(1, nv.lib().dmd_ssim_workspace_doubles(p.N, p.C, p.H, p.W)), dtype=torch.float64, device=device)


def frame_ssim(a: Tensor, b: Tensor, *, sigma: float = 1.5, k1: float = 0.01, k2: float = 0.03) -> Tensor:
    """Per-frame SSIM of `a` against `b`: (N, 2) fp64 on the device, columns mean ssim and mean contrast-structure term (cs).
    a, b: (N, C, H, W) on the current device, each uint8 levels or fp32 in [-1, 1] (taken at its level, the rounding and clamping
    of dmd_quantize_u8), H, W >= 11.  Gaussian window of 11 taps (sigma), C1 = (k1 * 255)^2, C2 = (k2 * 255)^2, positions whose
    window lies inside the frame -- what the common implementations compute for 8-bit images.  fp64, one summation order: the
    same bits on every run; identical frames give exactly 1.  ValueError for shape / dtype / size errors before anything is
    launched; the host does not wait for the result."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, Tensor) or t.dim() != 4:
            raise ValueError(f"frame_ssim: {name} must be a (N, C, H, W) tensor")
        if t.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"frame_ssim: {name} is {t.dtype}: uint8 levels or float32 in [-1, 1]")
    if a.shape != b.shape:
        raise ValueError(f"frame_ssim: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    if a.device != b.device:
        raise ValueError(f"frame_ssim: a on {a.device}, b on {b.device}")
    p = ssim_params(*a.shape, sigma=sigma, k1=k1, k2=k2)
    nv.check_current_device(a.device)
    out = torch.empty((p.N, 2), dtype=torch.float64, device=a.device)
    if p.N == 0:
        return out
    a, b = a.contiguous(), b.contiguous()
    set_operand(p, "a", a)
    set_operand(p, "b", b)
    work = ssim_workspace(p, a.device)
    p.workspace, p.out = nv.ptr(work), nv.ptr(out)
    nv.check(nv.lib().dmd_frame_ssim(C.byref(p), nv.stream()), "dmd_frame_ssim")
    return out
