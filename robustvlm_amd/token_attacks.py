"""Batched APGD on what a VLM reads from the tower: ``apgd`` of vlm_eval/attacks/apgd.py:163-368 (L-inf and L2, no mask,
maximising) with FARE's l2 over the tokens as the loss, run for every image of a batch on its own and as ONE device loop per
chunk of ``max_batch`` images (rvlm_apgd_run_tokens) - where ``vlm_attacks.apgd(TokenLossModel(...))`` takes one sample at a time
with a Python round trip per iteration.  Nothing inside the loop reads back to the host; the flag word is read once at the end.
CPU tensors raise (no CPU fallback).
"""
from __future__ import annotations

import torch

from . import _lib as L
from .attack_utils import LINF
from .clip_model import ClipVisionTower
from .engine import _require_cuda, _f32c
from .pgd_train import _raise_from_flags


def apgd_tokens(tower, x, ref_tokens, norm, eps, n_iter=10, pert_init=None, alpha=None, rho=0.75, return_trace=False):
    """``tower``: a :class:`ClipVisionTower` (its ``select_layer`` / ``select_feature`` / ``ln_post`` give depth, rows and
    ln_post); ``x`` ``[B, 3, H, W]`` in [0, 1]; ``ref_tokens``: what ``tower(x)`` returns, the tokens to move away from.  The loss
    of image b is ``sum (tower(x_adv)[b] - ref_tokens[b])^2``.  ``norm``: 'linf' | 'Linf' | 'l2' | 'L2'.  The first step size is
    ``alpha * eps`` (``alpha`` None: 2, the reference's), ``rho`` the oscillation threshold.  ``pert_init``: start at
    ``x + pert_init`` (clamped to [0, 1]); without one the start is ``x`` itself, where this loss has a zero gradient when
    ``ref_tokens`` are ``x``'s own tokens.  Batches beyond the engine's ``max_batch`` run in chunks (every quantity is per image).

    Returns ``(x_best, loss_best [B], x_best_adv)`` as the reference does (:368): the iterate of highest loss, that loss, and the
    last iterate before a restart; with ``return_trace`` a fourth value, the losses ``[n_iter + 1, B]`` (row 0: the start point)."""
    if norm not in ("linf", "Linf", "l2", "L2"):
        raise NotImplementedError(f"apgd_tokens covers norm 'linf' / 'Linf' / 'l2' / 'L2' (got {norm!r})")
    kind = 0 if norm in LINF else 2
    _require_cuda(x, "x")
    _require_cuda(ref_tokens, "ref_tokens")
    if not isinstance(tower, ClipVisionTower):
        raise TypeError("apgd_tokens expects a robustvlm_amd.ClipVisionTower")
    if pert_init is not None:
        _require_cuda(pert_init, "pert_init")
        if pert_init.shape != x.shape:
            raise ValueError(f"pert_init.shape: {tuple(pert_init.shape)}, x.shape: {tuple(x.shape)}")
    if x.dim() != 4 or ref_tokens.dim() != 3 or ref_tokens.shape[0] != x.shape[0]:
        raise ValueError(f"expected x [B, 3, H, W] and ref_tokens [B, n, W], got {tuple(x.shape)} and {tuple(ref_tokens.shape)}")
    eng = tower.model
    x = _f32c(x)
    ref = _f32c(ref_tokens)
    x_init = None if pert_init is None else x + _f32c(pert_init)
    step0 = (2. if alpha is None else alpha) * eps
    select = "patch" if tower.select_feature == "patch" else "all"
    outs, all_flags = [], []
    for lo in range(0, x.shape[0], eng.max_batch):
        hi = min(lo + eng.max_batch, x.shape[0])
        xb, lb, xl, flags, trace, _ = eng.apgd_run_tokens(
            x[lo:hi], None if x_init is None else x_init[lo:hi], ref[lo:hi], eps, n_iter, step0, depth=tower.depth,
            ln_post=tower.ln_post, select=select, norm_kind=kind, rho=rho, want_trace=return_trace)
        outs.append((xb, lb, xl, trace))
        all_flags.append(flags)
    flags = 0
    for f in torch.stack(all_flags).flatten().tolist():       # the loops' only host sync
        flags |= int(f)
    assert not (flags & L.FLAG_TOKENS_NONFINITE), "non-finite token loss"
    _raise_from_flags(flags)
    x_best, loss_best, x_last = (torch.cat([o[j] for o in outs], dim=0) for j in range(3))
    if return_trace:
        return x_best, loss_best, x_last, torch.cat([o[3] for o in outs], dim=1)
    return x_best, loss_best, x_last
