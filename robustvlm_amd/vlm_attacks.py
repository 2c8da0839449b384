"""Drop-in ``PGD`` (vlm_eval/attacks/pgd.py:5-87) and ``APGD`` / ``apgd`` (vlm_eval/attacks/apgd.py:5-49, 163-368): the attacks
``vlm_eval/run_evaluation.py`` runs against a vision-language model, on a ``[B, n_img, 1, 3, H, W]`` tensor with a mask over the
image axis (``mask_out`` = 'context' | 'query' | an int | None, for ``APGD`` also 'none').  The model returns the loss itself.

Two routes, both on the GPU:

* generic - ``model`` is any torch callable returning the loss (this is where an LLM sits): forward and ``torch.autograd.grad`` in
  torch, every other operation of an iteration in librvlm.so: rvlm_pgd_masked_update (PGD: one launch), rvlm_apgd_masked_step +
  rvlm_apgd_masked_bookkeeping (APGD: three).  The mask is ``uint8 [n_img]``, never a full-size tensor.  Nothing inside the loop
  reads a value back to the host (no ``.item()``, no ``nonzero()``); the reference's per-iteration prints / asserts are bits of a
  device flag word read once after the loop.  ``verbose=True`` prints, and so synchronises.
* engine - ``model`` is a :class:`TokenLossModel` (a :class:`ClipVisionTower` and the tokens to move away from or towards): forward,
  FARE's l2 over the tokens and the input gradient are one rvlm_vit_tokens_fwd_inputgrad call per iteration and no autograd graph
  is built.  Masked images still go through the forward (their tokens are part of the loss); only their gradient is dropped.

L-inf and L2; the reference's L1 / L0 branches of ``apgd`` raise NotImplementedError.  CPU tensors raise (no CPU fallback).
"""
from __future__ import annotations

import torch

from . import _lib as L
from .attack_utils import LINF, L2
from .clip_model import ClipVisionTower
from .engine import _require_cuda, _f32c
from .pgd_train import _raise_from_flags


def _check_mask_out(mask_out):
    if not (mask_out in ('context', 'query') or isinstance(mask_out, int) or mask_out is None):
        raise NotImplementedError(f'Unknown mask_out: {mask_out}')                        # pgd.py:86, apgd.py:45


def _image_mask(mask_out, data):
    """``_set_mask`` of both classes (pgd.py:75-87, apgd.py:34-46) as one byte per image: 1 = attacked, 0 = masked out.  Built on
    the device (no host-to-device copy)."""
    _check_mask_out(mask_out)
    mask = torch.ones(data.shape[1], dtype=torch.uint8, device=data.device)
    if mask_out == 'context':
        mask[:-1] = 0
    elif mask_out == 'query':
        mask[-1] = 0
    elif mask_out is not None:
        mask[mask_out] = 0
    return mask


def _mask_from_tensor(mask, x):
    """``apgd(mask=...)``: None, one value per image, or the reference's full-size 0/1 tensor (constant behind the image axis)."""
    if mask is None:
        return None
    n_img = x.shape[1]
    if mask.numel() == n_img:
        return (mask.reshape(n_img) != 0).to(device=x.device, dtype=torch.uint8).contiguous()
    if tuple(mask.shape) != tuple(x.shape):
        raise ValueError(f"mask must have one value per image ({n_img}) or x's shape {tuple(x.shape)}, got {tuple(mask.shape)}")
    m = mask.to(x.device).reshape(x.shape[0], n_img, -1)
    per = m[0, :, 0]
    if not bool(((m == per.view(1, -1, 1)) & ((m == 0) | (m == 1))).all()):
        raise NotImplementedError("the native apgd takes a 0/1 mask that is constant over each image")
    return (per != 0).to(torch.uint8).contiguous()


def _geometry(x):
    if x.dim() < 2:
        raise ValueError(f"expected [B, n_img, ...] (the reference passes [B, n_img, 1, 3, H, W]), got {tuple(x.shape)}")
    B, n_img = x.shape[0], x.shape[1]
    return B, n_img, x[0, 0].numel()


def _norm_kind(norm, what):
    if norm in LINF:
        return 0
    if norm in L2:
        return 2
    raise NotImplementedError(f'{what}: norm {norm} not supported on the native path (L-inf and L2 are)')


class TokenLossModel(torch.nn.Module):
    """The loss a VLM-side attack can drive without an LLM: FARE's l2 over the tokens the VLM reads,
    ``sum (tower(x) - target_tokens)^2`` over every image, row and feature of a sample.  ``forward(x)`` takes the attacks'
    ``[B, n_img, 1, 3, H, W]`` (or anything that flattens to ``[B * n_img, 3, H, W]``) and returns the loss ``[B]``, differentiable
    through the tower; :class:`PGD` / :class:`APGD` recognise the class and call :meth:`loss_and_grad` instead - one native call,
    no autograd graph.  ``target_tokens``: ``[B * n_img, n, W]`` as ``tower`` returns them (``select_feature`` / ``select_layer`` /
    ``ln_post`` are the tower's).  ``mode='max'`` moves away from them (untargeted), ``'min'`` towards them (targeted)."""

    def __init__(self, tower: ClipVisionTower, target_tokens: torch.Tensor):
        super().__init__()
        if not isinstance(tower, ClipVisionTower):
            raise TypeError("TokenLossModel expects a robustvlm_amd.ClipVisionTower")
        _require_cuda(target_tokens, "target_tokens")
        self.tower = tower
        self.target_tokens = _f32c(target_tokens)

    def _images(self, x):
        ih, iw = self.tower.model.input_size
        if x.dim() < 4 or tuple(x.shape[-3:]) != (3, ih, iw):
            raise ValueError(f"expected [..., 3, {ih}, {iw}] images, got {tuple(x.shape)}")
        return x.reshape(-1, 3, ih, iw)

    def forward(self, x):
        tok = self.tower(self._images(x))
        per = ((tok - self.target_tokens) ** 2).sum(dim=(1, 2))
        return per.view(x.shape[0], -1).sum(dim=1)

    def loss_and_grad(self, x, delta=None):
        """(loss [B], d loss.sum() / d x shaped like x) of ``x (+ delta)`` from rvlm_vit_tokens_fwd_inputgrad."""
        t = self.tower
        xi = self._images(_f32c(x))
        di = None if delta is None else self._images(_f32c(delta))
        _, per, _, g = t.model.tokens_fwd_inputgrad(xi, di, self.target_tokens, depth=t.depth, ln_post=t.ln_post,
                                                    select="patch" if t.select_feature == "patch" else "all", reduction="none")
        return per.view(x.shape[0], -1).sum(dim=1), g.view(x.shape)


class PGD:
    """
    Minimize or maximize given loss
    """

    def __init__(self, forward, norm, eps, mode='min', mask_out='context', image_space=True):
        self.model = forward

        self.norm = norm
        self.eps = eps
        self.momentum = 0.9

        self.mode = mode
        self.mask_out = mask_out
        self.image_space = image_space

    def perturb(self, data_clean, iterations, stepsize, perturbation=None, verbose=False, return_loss=False):
        kind = _norm_kind(self.norm, "PGD")
        if self.mode not in ('min', 'max'):
            raise ValueError(f'Unknown mode: {self.mode}')                                 # pgd.py:55
        _check_mask_out(self.mask_out)
        _require_cuda(data_clean, "data_clean")
        lib = L.load()
        x = _f32c(data_clean)
        B, n_img, P = _geometry(x)
        mask = self._set_mask(x)
        flags = torch.zeros(1, dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            if self.image_space:                                                           # :22-24
                L.check(lib.rvlm_check_image_range(x.data_ptr(), x.numel(), flags.data_ptr(), L.stream_ptr()))
            delta = torch.zeros_like(x) if perturbation is None else _f32c(perturbation).clone()
            if delta.shape != x.shape:
                raise ValueError(f"perturbation {tuple(delta.shape)} does not match data_clean {tuple(x.shape)}")
            velocity = torch.zeros_like(x)
            engine = isinstance(self.model, TokenLossModel)
            for i in range(iterations):
                if engine:
                    loss, gradient = self.model.loss_and_grad(x, delta)
                else:
                    p = delta.detach().requires_grad_(True)
                    with torch.enable_grad():
                        loss = self.model(data_clean + p)
                    gradient = _f32c(torch.autograd.grad(loss, p)[0])
                    loss = loss.detach()
                # print 10 times in total and last iteration
                if verbose and (i % (iterations // 10 + 1) == 0 or i == iterations - 1):
                    print(f'[iteration] {i} [loss] {loss.item()}')
                L.check(lib.rvlm_pgd_masked_update(
                    x.data_ptr(), gradient.data_ptr(), delta.data_ptr(), velocity.data_ptr(), mask.data_ptr(), B, n_img, P, kind,
                    float(self.eps), float(stepsize), float(self.momentum), 1 if self.mode == 'max' else 0,
                    int(bool(self.image_space)), None, flags.data_ptr(), L.stream_ptr()), "rvlm_pgd_masked_update")
        _raise_from_flags(int(flags.item()))          # the loop's only host sync
        if return_loss:
            return data_clean + delta, loss
        else:
            return data_clean + delta

    def _set_mask(self, data):
        """One byte per image (1 = attacked) where the reference builds a full-size tensor (pgd.py:75-87)."""
        return _image_mask(self.mask_out, data)


class APGD:
    def __init__(self, model, norm, eps, mask_out='context', initial_stepsize=None, decrease_every=None, decrease_every_max=None,
                 random_init=False):
        # model returns loss sum over batch
        # thus currently only works with batch size 1
        # initial_stepsize: in terms of eps. called alpha in apgd
        # decrease_every: potentially decrease stepsize every x fraction of total iterations. default: 0.22
        self.model = model
        self.norm = norm
        self.eps = eps
        self.initial_stepsize = initial_stepsize
        self.decrease_every = decrease_every
        self.decrease_every_max = decrease_every_max
        self.random_init = random_init
        if mask_out != 'none':
            self.mask_out = mask_out
        else:
            self.mask_out = None

    def perturb(self, data_clean, iterations, pert_init=None, verbose=False):
        _check_mask_out(self.mask_out)
        mask = self._set_mask(data_clean)
        data_adv, _, _ = apgd(
            self.model, data_clean, norm=self.norm, eps=self.eps, n_iter=iterations,
            use_rs=self.random_init, mask=mask, alpha=self.initial_stepsize,
            n_iter_2=self.decrease_every, n_iter_min=self.decrease_every_max, pert_init=pert_init,
            verbose=verbose
            )

        return data_adv

    def _set_mask(self, data):
        """One byte per image (1 = attacked) where the reference builds a full-size tensor (apgd.py:34-46)."""
        return _image_mask(self.mask_out, data)

    def __str__(self):
        return 'APGD'


def L2_norm(x, keepdim=False):
    z = (x ** 2).view(x.shape[0], -1).sum(-1).sqrt()
    if keepdim:
        z = z.view(-1, *[1] * (len(x.shape) - 1))
    return z


def apgd(model, x, norm, eps, n_iter=10, use_rs=False, mask=None, alpha=None, n_iter_2=None,
         n_iter_min=None, pert_init=None, verbose=False, is_train=True):
    """Signature of apgd.py:163-164; returns (x_best, loss_best, x_best_adv) (:368).  ``mask``: None, one value per image, or the
    reference's full-size tensor.  ``model(x)`` returns the loss ``[B]`` (a scalar is taken as ``[1]``)."""
    assert x.shape[0] == 1  # only support batch size 1 for now
    norm = norm.replace('l', 'L')
    if norm not in ('Linf', 'L2'):
        raise NotImplementedError(f"apgd on the native path covers norm='Linf' and 'L2' (got {norm})")
    kind = 0 if norm == 'Linf' else 2
    _require_cuda(x, "x")
    lib = L.load()
    x = _f32c(x)
    device = x.device
    B, n_img, P = _geometry(x)
    mask = _mask_from_tensor(mask, x)

    if not use_rs:
        x_adv = x.clone()
    else:
        if norm == 'Linf':
            t = torch.zeros_like(x).uniform_(-eps, eps).detach()
            x_adv = x + t
        elif norm == 'L2':
            t = torch.randn(x.shape).to(device).detach()
            x_adv = x + eps * torch.ones_like(x).detach() * t / (L2_norm(t, keepdim=True) + 1e-12)
    if pert_init is not None:
        assert not use_rs
        assert pert_init.shape == x.shape, f'pert_init.shape: {pert_init.shape}, x.shape: {x.shape}'
        _require_cuda(pert_init, "pert_init")
        x_adv = x + _f32c(pert_init)

    x_adv = x_adv.clamp(0., 1.).contiguous()
    x_best = x_adv.clone()
    x_best_adv = x_adv.clone()
    x_adv_old = x_adv.clone()
    loss_steps = torch.zeros([n_iter, B], dtype=torch.float32, device=device)

    # set params (apgd.py:192-213)
    n_iter_2_frac = 0.22 if n_iter_2 is None else n_iter_2
    n_iter_min_frac = 0.06 if n_iter_min is None else n_iter_min
    n_iter_2 = max(int(n_iter_2_frac * n_iter), 1)
    n_iter_min = max(int(n_iter_min_frac * n_iter), 1)
    size_decr = max(int(0.03 * n_iter), 1)
    k = n_iter_2 + 0
    alpha = 2. if alpha is None else alpha
    step_size = torch.full([B], alpha * eps, dtype=torch.float32, device=device)
    counter3 = 0

    engine = isinstance(model, TokenLossModel)

    def evaluate(need_grad):
        """(loss_indiv [B], gradient | None) at x_adv; the gradient is the raw one, the step kernel masks it."""
        if engine and need_grad:
            return model.loss_and_grad(x_adv)
        if not need_grad:
            with torch.no_grad():
                return _f32c(model(x_adv)).reshape(B), None
        xa = x_adv.detach().requires_grad_(True)
        with torch.enable_grad():
            loss_indiv = model(xa)
            loss = loss_indiv.sum()
        g = _f32c(torch.autograd.grad(loss, [xa])[0])
        return _f32c(loss_indiv).reshape(B), g

    flags = torch.zeros(1, dtype=torch.int32, device=device)
    scratch = torch.zeros(5 * B, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        loss_indiv, grad = evaluate(True)
        grad_best = grad.clone()
        loss_best = loss_indiv.clone()
        loss_best_last_check = loss_best.clone()
        reduced_last_check = torch.ones_like(loss_best)

        for i in range(n_iter):
            ### gradient step
            loss_curr = loss_indiv
            a = 0.75 if i > 0 else 1.0
            L.check(lib.rvlm_apgd_masked_step(
                x.data_ptr(), x_adv.data_ptr(), x_adv_old.data_ptr(), grad.data_ptr(), L.ptr(mask), step_size.data_ptr(), a,
                float(eps), B, n_img, P, kind, flags.data_ptr(), L.stream_ptr()), "rvlm_apgd_masked_step")

            ### get gradient (the last iteration saves one backward pass and keeps the gradient it has, apgd.py:300-304)
            loss_indiv, g = evaluate(i < n_iter - 1)
            if g is not None:
                grad = g

            if verbose and (i % max(n_iter // 10, 1) == 0 or i == n_iter - 1):
                print('iteration: {} - best loss: {:.6f} curr loss {:.6f} {}'.format(
                    i, loss_best.sum(), loss_curr.sum(), ' - step size: {:.5f}'.format(step_size.mean())))

            ### check step size
            counter3 += 1
            do_check = int(counter3 == k)
            L.check(lib.rvlm_apgd_masked_bookkeeping(
                i, B, n_iter, k, do_check, loss_indiv.data_ptr(), loss_steps.data_ptr(), loss_best.data_ptr(),
                loss_best_last_check.data_ptr(), reduced_last_check.data_ptr(), step_size.data_ptr(), x_adv.data_ptr(),
                grad.data_ptr(), x_best.data_ptr(), grad_best.data_ptr(), x_best_adv.data_ptr(), scratch.data_ptr(), n_img * P,
                L.stream_ptr()), "rvlm_apgd_masked_bookkeeping")
            if do_check:
                counter3 = 0
                k = max(k - size_decr, n_iter_min)

    if int(flags.item()) & L.FLAG_NAN_GRAD:           # the loop's only host sync
        print('attention: nan in gradient')
    return x_best, loss_best, x_best_adv
