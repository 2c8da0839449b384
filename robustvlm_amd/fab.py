"""Drop-in ``FABAttack`` (autoattack/fab_base.py + fab_pt.py ``FABAttack_PT``) for the ``fab`` / ``fab-t`` entries of
AutoAttack: L-inf, targeted (FAB-T) and untargeted, random restarts / target classes over the still-robust points.

Per iteration FAB linearises the classifier at the iterate x1 (logit difference ``df`` and its input gradient ``dg``),
projects x1 and the clean image onto the hyperplane ``dg.z = -df + dg.x1`` inside the box, mixes the two projections, and
steps back towards the clean image once x1 is misclassified.  The device work besides the model is three HIP kernels
(csrc/fab_kernels.hip): ``rvlm_fab_linf_step`` (reductions, both box-constrained projections found by a sort-free search,
the update - in one launch), ``rvlm_fab_track_best`` after the prediction forward, and for untargeted FAB
``rvlm_fab_jacobian_argmin`` once per class.  Everything is per-image masks on the device: the iteration loop does not
synchronise with the host.

Two routes, as in :class:`~robustvlm_amd.autopgd.APGDAttack`:

* engine route (targeted, ``predict`` is a :class:`ClassificationModel` over the engine with a logit scale and the identity
  resizer, more than one image): ``df`` and ``dg`` come from one ``rvlm_vit_fwd_inputgrad`` call with
  ``RVLM_LOSS_LOGIT_DIFF`` - no autograd graph; batches beyond the engine's ``max_batch`` run as chunks.
* generic route (any differentiable torch callable on device tensors): ``torch.autograd.grad`` of the logit difference.
  Targeted: one backward per iteration.  Untargeted: the class Jacobian is streamed through ``rvlm_fab_jacobian_argmin``
  class by class instead of the reference's ``[K, B, D]`` tensor - that is ``K + 1`` backward passes per iteration (one
  for the true class, one per class), meant for small heads; untargeted FAB on a ``ClassificationModel`` takes this
  route.

The random start of restarts > 0 is drawn on the CPU generator in the reference's order (fab_base.py:120-128), so a seed
reproduces the reference's start.  L2 / L1 raise NotImplementedError (their projections are different algorithms).
"""
from __future__ import annotations

import ctypes as C
import time

import torch

from . import _lib as L
from .clip_model import ClassificationModel
from .engine import _require_cuda, _f32c

DEFAULT_EPS_DICT_BY_NORM = {'Linf': .3, 'L2': 1., 'L1': 5.0}


class FABAttack():
    """Fast Adaptive Boundary Attack https://arxiv.org/abs/1907.02044 (constructor of fab_pt.py:35-50)."""

    def __init__(self, predict, norm='Linf', n_restarts=1, n_iter=100, eps=None, alpha_max=0.1, eta=1.05, beta=0.9,
                 loss_fn=None, verbose=False, seed=0, targeted=False, device=None, n_target_classes=9):
        self.predict = predict
        self.norm = norm
        self.n_restarts = n_restarts
        self.n_iter = n_iter
        self.eps = eps if eps is not None else DEFAULT_EPS_DICT_BY_NORM[norm]
        self.alpha_max = alpha_max
        self.eta = eta
        self.beta = beta
        self.targeted = targeted
        self.verbose = verbose
        self.seed = seed
        self.target_class = None
        self.device = device
        self.n_target_classes = n_target_classes
        if norm != 'Linf':
            raise NotImplementedError("native FABAttack covers norm='Linf'")

    # ---- model access (fab_pt.py:66-73)
    def _predict_fn(self, x):
        return self.predict(x)

    def _get_predicted_label(self, x):
        with torch.no_grad():
            return self._predict_fn(x).max(dim=1)[1]

    def _engine_route(self, n, is_targeted, x=None):
        """FAB-T on a ClassificationModel whose resizer is the identity or - for images ``x`` - one the engine runs itself
        (a BicubicResize up to the model's resolution): df, dg come from rvlm_vit_fwd_inputgrad at the images' own size."""
        m = self.predict
        return (is_targeted and isinstance(m, ClassificationModel) and n > 1 and bool(m.logit_scale)
                and (m._identity_resizer or (x is not None and m.engine_input_size(x) is not None)))

    # ---- df, dg of one iterate on the generic route
    def get_diff_logits_grads_batch_targeted(self, imgs, la, la_target):
        """df [B] = -(z_y - z_t), dg [B, ...] = its input gradient (fab_pt.py:100-114)."""
        u = torch.arange(imgs.shape[0], device=imgs.device)
        im = imgs.clone().requires_grad_()
        with torch.enable_grad():
            z = self.predict(im)
            diffy = -(z[u, la] - z[u, la_target])
            (g,) = torch.autograd.grad(diffy.sum(), im)
        return _f32c(diffy), _f32c(g)

    def get_diff_logits_grads_batch(self, imgs, la):
        """The class nearest in the linearisation (fab_pt.py:76-98 + fab_base.py:166-184): df [B], dg [B, ...] of
        argmin_k |z_k - z_y| / |grad z_k - grad z_y|_1, streamed class by class (K + 1 backward passes)."""
        lib = L.load()
        B, n = imgs.shape[0], imgs[0].numel()
        u = torch.arange(B, device=imgs.device)
        im = imgs.clone().requires_grad_()
        best_dist = torch.full([B], float('inf'), device=imgs.device)
        best_df = torch.zeros(B, device=imgs.device)
        best_w = torch.zeros_like(imgs)
        with torch.enable_grad():
            z = self.predict(im)
            zy = z[u, la]
            g_y = _f32c(torch.autograd.grad(zy.sum(), im, retain_graph=True)[0])
            for k in range(z.shape[-1]):
                g_k = _f32c(torch.autograd.grad(z[:, k].sum(), im, retain_graph=True)[0])
                df_k = _f32c(z[:, k] - zy)
                with torch.cuda.device(imgs.device):
                    L.check(lib.rvlm_fab_jacobian_argmin(g_k.data_ptr(), g_y.data_ptr(), df_k.data_ptr(), la.data_ptr(), k, B,
                                                         n, best_dist.data_ptr(), best_df.data_ptr(), best_w.data_ptr(),
                                                         L.stream_ptr()), "rvlm_fab_jacobian_argmin")
        return best_df, best_w

    # ---- the iteration loop on a batch of clean-correct points (fab_base.py:160-254); returns (adv, res2)
    def _iterate(self, im2, la2, la_target2, x1, engine):
        lib = L.load()
        B, n = im2.shape[0], im2[0].numel()
        dev = im2.device
        adv = im2.clone()
        res2 = torch.full([B], 1e10, device=dev, dtype=torch.float32)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        eq = torch.empty(B, dtype=torch.uint8, device=dev)
        m = self.predict
        if engine:
            eng = m.model
            eng._check_images(x1)
            T = _f32c(m.text_embedding)
            ls = eng._loss_spec("logit-diff", "none", True, T, la2, m.logit_scale_value, y_target=la_target2, B=B)
            df = torch.empty(B, device=dev, dtype=torch.float32)
            dg = torch.empty_like(x1)
        with torch.cuda.device(dev):
            for _ in range(self.n_iter):
                if engine:
                    L.check(lib.rvlm_vit_fwd_inputgrad(eng._h, x1.data_ptr(), None, B, C.byref(ls), None, df.data_ptr(), None,
                                                       dg.data_ptr(), L.stream_ptr()), "rvlm_vit_fwd_inputgrad")
                    eng.generation += 1
                elif la_target2 is not None:
                    df, dg = self.get_diff_logits_grads_batch_targeted(x1, la2, la_target2)
                else:
                    df, dg = self.get_diff_logits_grads_batch(x1, la2)
                L.check(lib.rvlm_fab_linf_step(x1.data_ptr(), im2.data_ptr(), dg.data_ptr(), df.data_ptr(), B, n,
                                               float(self.alpha_max), float(self.eta), None, flags.data_ptr(), L.stream_ptr()),
                        "rvlm_fab_linf_step")
                with torch.no_grad():
                    logits = _f32c(self._predict_fn(x1))
                L.check(lib.rvlm_argmax_eq(logits.data_ptr(), la2.data_ptr(), B, logits.shape[1], eq.data_ptr(), L.stream_ptr()),
                        "rvlm_argmax_eq")
                L.check(lib.rvlm_fab_track_best(x1.data_ptr(), im2.data_ptr(), adv.data_ptr(), res2.data_ptr(), eq.data_ptr(),
                                                float(self.beta), B, n, L.stream_ptr()), "rvlm_fab_track_best")
        self.flags = flags      # RVLM_FLAG_FAB_NONFINITE if a gradient held NaN / Inf (read it after the run: no sync here)
        return adv, res2

    def attack_single_run(self, x, y=None, use_rand_start=False, is_targeted=False):
        """
        :param x:             clean images
        :param y:             clean labels, if None we use the predicted labels
        :param is_targeted    True if we ise targeted version. Targeted class is assigned by `self.target_class`
        """
        _require_cuda(x, "x")
        if self.device is None:
            self.device = x.device
        lib = L.load()
        x = x.detach().clone().float().to(self.device).contiguous()
        y_pred = self._get_predicted_label(x)
        y = (y_pred if y is None else y).detach().clone().long().to(self.device)
        pred = y_pred == y
        corr_classified = int(pred.sum())
        if self.verbose:
            print('Clean accuracy: {:.2%}'.format(pred.float().mean()))
        if corr_classified == 0:
            return x
        pred = pred.nonzero().flatten()
        la_target2 = None
        if is_targeted:
            with torch.no_grad():
                output = self._predict_fn(x)
            # the target_class-th most likely class of every point (fab_base.py:111-113 takes it from a full sort)
            la_target2 = output.topk(self.target_class, dim=-1)[1][:, -1][pred].detach().clone().contiguous()
        startt = time.time()
        # runs the attack only on correctly classified points
        im2 = x[pred].detach().clone().contiguous()
        la2 = y[pred].detach().clone().contiguous()
        bs = im2.shape[0]
        x1 = im2.clone()
        if use_rand_start:
            # fab_base.py:120-128 with res2 = 1e10: im2 + (eps / 2) t / max|t|, t drawn on the CPU generator like the reference
            t = (2 * torch.rand(x1.shape).to(self.device) - 1).contiguous()
            with torch.cuda.device(self.device):
                L.check(lib.rvlm_linf_random_start(im2.data_ptr(), t.data_ptr(), float(self.eps) * .5, im2[0].numel(), bs,
                                                   x1.data_ptr(), L.stream_ptr()), "rvlm_linf_random_start")
            x1.clamp_(0.0, 1.0)
        if self._engine_route(bs, is_targeted, im2):
            # every quantity is per sample: batches beyond the engine's workspace run as chunks of >= 2 images
            mb = self.predict.model.max_batch
            bounds = list(range(0, bs, mb)) + [bs]
            if len(bounds) > 2 and bounds[-1] - bounds[-2] < 2:
                bounds[-2] -= 1
            with self.predict.engine_route(im2):      # (a resizer the engine runs: the handle works at im2's size meanwhile)
                parts = [self._iterate(im2[lo:hi], la2[lo:hi], la_target2[lo:hi], x1[lo:hi], True)
                         for lo, hi in zip(bounds[:-1], bounds[1:])]
            adv, res2 = (torch.cat([p[i] for p in parts]) for i in range(2))
        else:
            adv, res2 = self._iterate(im2, la2, la_target2, x1, False)
        ind_succ = (res2 < 1e10).nonzero().flatten()
        if self.verbose:
            print('success rate: {:.0f}/{:.0f}'.format(ind_succ.numel(), corr_classified)
                  + ' (on correctly classified points) in {:.1f} s'.format(time.time() - startt))
        adv_c = x.clone()
        adv_c[pred[ind_succ]] = adv[ind_succ].clone()
        return adv_c

    def _attack_survivors(self, x, y, acc, adv, use_rand_start, is_targeted):
        """One run over the points that are still robust (the loop body of fab_base.py:275-290 / :303-318): a result
        counts only if it is misclassified AND within eps."""
        ind_to_fool = acc.nonzero().flatten()
        if ind_to_fool.numel() == 0:
            return
        x_to_fool, y_to_fool = x[ind_to_fool].clone(), y[ind_to_fool].clone()
        adv_curr = self.attack_single_run(x_to_fool, y_to_fool, use_rand_start=use_rand_start, is_targeted=is_targeted)
        acc_curr = self._predict_fn(adv_curr).max(1)[1] == y_to_fool
        res = (x_to_fool - adv_curr).abs().reshape(x_to_fool.shape[0], -1).max(1)[0]
        acc_curr = torch.max(acc_curr, res > self.eps)
        ind_curr = (acc_curr == 0).nonzero().flatten()
        acc[ind_to_fool[ind_curr]] = 0
        adv[ind_to_fool[ind_curr]] = adv_curr[ind_curr].clone()

    def perturb(self, x, y):
        _require_cuda(x, "x")
        if self.device is None:
            self.device = x.device
        adv = x.clone()
        with torch.no_grad():
            acc = self._predict_fn(x).max(1)[1] == y
            startt = time.time()
            torch.random.manual_seed(self.seed)
            torch.cuda.random.manual_seed(self.seed)
            if not self.targeted:
                for counter in range(self.n_restarts):
                    self._attack_survivors(x, y, acc, adv, counter > 0, False)
                    if self.verbose:
                        print('restart {} - robust accuracy: {:.2%} at eps = {:.5f} - cum. time: {:.1f} s'.format(
                            counter, acc.float().mean(), self.eps, time.time() - startt))
            else:
                for target_class in range(2, self.n_target_classes + 2):
                    self.target_class = target_class
                    for counter in range(self.n_restarts):
                        self._attack_survivors(x, y, acc, adv, counter > 0, True)
                        if self.verbose:
                            print('restart {} - target_class {} - robust accuracy: {:.2%} at eps = {:.5f} - cum. time: {:.1f} s'
                                  .format(counter, self.target_class, acc.float().mean(), self.eps, time.time() - startt))
        return adv
