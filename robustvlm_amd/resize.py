"""``BicubicResize``: the resizer of the reference's low-resolution evaluations as a native, differentiable op.

CLIP_eval/clip_robustbench.py:104-114 and CLIP_benchmark/clip_benchmark/cli.py:231-234 attack CIFAR / STL-10 in the dataset's own
pixel space and make the up-sampling part of the model: ``ClassificationModel(..., resizer=Resize(224, BICUBIC, antialias=False))``.
On a float tensor torchvision's ``Resize`` is ``F.interpolate(x, size, mode='bicubic', align_corners=False, antialias=False)``
(no clamp of the overshoot); this module is that operator on rvlm_resize_bicubic / rvlm_resize_bicubic_adjoint
(csrc/resize_kernels.hip).  Given to :class:`ClassificationModel` it is fused into the engine's patch embedding
(``VitEngine.set_input_size``) wherever its result is the model's own resolution.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .engine import _require_cuda


def resize_taps(n_in: int, n_out: int):
    """The tap table of one axis as (idx [n_out, 4] int32, w [n_out, 4] float32): rvlm_resize_taps, host only."""
    idx = np.empty((int(n_out), 4), np.int32)
    w = np.empty((int(n_out), 4), np.float32)
    L.check(L.load().rvlm_resize_taps(int(n_in), int(n_out), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                      w.ctypes.data_as(C.POINTER(C.c_float))), "rvlm_resize_taps")
    return idx, w


def _check_input(x):
    _require_cuda(x, "resize input")
    if x.dim() != 4:
        raise ValueError(f"expected [B, C, h, w] images, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"BicubicResize takes float32 tensors (the attack's pixel space), got {x.dtype}")


class _ResizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_h: int, out_w: int):
        xc = x.detach().contiguous()
        B, Cn, h, w = xc.shape
        y = torch.empty(B, Cn, out_h, out_w, dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            L.check(L.load().rvlm_resize_bicubic(xc.data_ptr(), B * Cn, h, w, out_h, out_w, y.data_ptr(), L.stream_ptr()),
                    "rvlm_resize_bicubic")
        ctx.in_hw = (h, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        g = gy.detach().to(torch.float32).contiguous()
        B, Cn, H, W = g.shape
        h, w = ctx.in_hw
        gx = torch.empty(B, Cn, h, w, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            L.check(L.load().rvlm_resize_bicubic_adjoint(g.data_ptr(), B * Cn, h, w, H, W, gx.data_ptr(), L.stream_ptr()),
                    "rvlm_resize_bicubic_adjoint")
        return gx, None, None


class BicubicResize(torch.nn.Module):
    """``torchvision.transforms.Resize(size, interpolation=BICUBIC, antialias=False)`` for float32 device tensors
    ``[B, C, h, w]``.  ``size``: an int (the smaller edge; the other follows the aspect ratio with torchvision's rounding) or
    ``(H, W)``.  Any pair of sizes, down-sampling included.  No fallback: CPU tensors, other dtypes and ``antialias=True``
    raise."""

    def __init__(self, size, antialias: bool = False):
        super().__init__()
        if antialias:
            raise NotImplementedError("BicubicResize covers antialias=False (the reference's resizer)")
        if isinstance(size, (list, tuple)):
            if len(size) not in (1, 2) or not all(isinstance(v, int) and v > 0 for v in size):
                raise ValueError(f"size must be a positive int or (H, W), got {size!r}")
            size = int(size[0]) if len(size) == 1 else (int(size[0]), int(size[1]))
        elif isinstance(size, int) and not isinstance(size, bool) and size > 0:
            size = int(size)
        else:
            raise ValueError(f"size must be a positive int or (H, W), got {size!r}")
        self.size = size
        self.antialias = False

    def output_size(self, h: int, w: int):
        """(H, W) for an input of (h, w): torchvision's ``_compute_resized_output_size``."""
        if isinstance(self.size, tuple):
            return self.size
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = self.size, int(self.size * long / short)
        return (new_long, new_short) if w <= h else (new_short, new_long)

    def forward(self, x):
        _check_input(x)
        H, W = self.output_size(int(x.shape[-2]), int(x.shape[-1]))
        return _ResizeFn.apply(x, H, W)

    def extra_repr(self):
        return f"size={self.size}, interpolation=bicubic, antialias=False"
