"""Drop-in ``SquareAttack`` (autoattack/square.py) for the black-box evaluation route
(CLIP_eval/clip_robustbench.py:150-151 -> ``AutoAttack(version='custom', attacks_to_run=['square'])``): L-inf and L2
(``--norm linf|l2``), margin / cross-entropy loss, untargeted or targeted, random restarts over the still-correct points.

A query-only attack: the device work is the model forward (``predict``, e.g. :class:`ClassificationModel` over the
engine) plus two HIP kernels per query - ``rvlm_square_linf_propose`` / ``rvlm_square_l2_propose`` builds the candidates of
the still-robust images, ``rvlm_square_accept`` keeps the ones that improved.  The random numbers are drawn on the CPU
generator in the reference's order (square.py:113-119 draws with ``torch.rand(shape)`` and moves the result to the device),
so a seed reproduces the reference's sequence of squares.

L2 (square.py:305-420): the whole query - three families of window / image norms, the new window content, the write-back of
both windows and the projection onto the eps sphere - is one launch; only ``eta(s)`` ([s, s]) and the signs travel to the
device.  Its sums run in the kernel's own fixed order, so candidates agree with the reference's to rounding, not to the bit.
The reference's per-query NaN asserts (:416-417) are a bit of a device flag word read once after the loop.  L1 raises
NotImplementedError (not selected by the repo's configs).
"""
from __future__ import annotations

import math
import time

import torch
import torch.nn.functional as F

from . import _lib as L
from .engine import _require_cuda, _f32c


def p_selection(it, n_queries, p_init, rescale):
    """Fraction of the image one square covers at query ``it`` (square.py:192-219)."""
    if rescale:
        it = int(it / n_queries * 10000)
    halvings = sum(it > b for b in (10, 50, 200, 500, 1000, 2000, 4000, 6000, 8000))
    return p_init / (1 << halvings)


def l2_window_size(it, n_queries, p_init, rescale, c, h, w):
    """Side of the L2 windows at query ``it`` (square.py:340-344): at least 3, odd, at most the image."""
    p = p_selection(it, n_queries, p_init, rescale)
    s = max(int(round(math.sqrt(p * (c * h * w) / c))), 3)
    return min(s + (s % 2 == 0), min(h, w))


def _pyramid(rows, cols):
    """Nested rectangles around the centre (rows // 2, cols // 2), the k-th one reaching k cells each way and adding
    1 / (k + 1)^2 (fp32, added in the order of k), then scaled to unit L2 norm (eta_rectangles, square.py:143-157)."""
    t = torch.zeros(rows, cols)
    cr, cc = rows // 2, cols // 2
    for k in range(max(cr, cc) + 1):
        t[max(cr - k, 0):min(cr + k + 1, rows), max(cc - k, 0):min(cc + k + 1, cols)] += 1.0 / (torch.Tensor([k + 1]).view(1, 1) ** 2)
    return t / (t ** 2).sum(dim=(0, 1), keepdim=True).sqrt()


_ETA_CACHE = {}


def eta_window(s):
    """The L2 attack's [s, s] update pattern before its transpose coin (eta, square.py:172-177): a pyramid on the upper
    s // 2 rows, minus a pyramid on the rest, unit L2 norm.  CPU float32, the reference's bits; cached per ``s`` (do not
    write into the result)."""
    if s not in _ETA_CACHE:
        t = torch.zeros(s, s)
        t[:s // 2] = _pyramid(s // 2, s)
        t[s // 2:] = -1. * _pyramid(s - s // 2, s)
        _ETA_CACHE[s] = t / (t ** 2).sum(dim=(0, 1), keepdim=True).sqrt()
    return _ETA_CACHE[s]


class SquareAttack():
    """Square Attack https://arxiv.org/abs/1912.00049 (constructor of square.py:36-66)."""

    def __init__(self, predict, norm='Linf', n_queries=5000, eps=None, p_init=.8, n_restarts=1, seed=0, verbose=False,
                 targeted=False, loss='margin', resc_schedule=True, device=None):
        self.predict = predict
        self.norm = norm
        self.n_queries = n_queries
        self.eps = eps
        self.p_init = p_init
        self.n_restarts = n_restarts
        self.seed = seed
        self.verbose = verbose
        self.targeted = targeted
        self.loss = loss
        self.rescale_schedule = resc_schedule
        self.device = device
        self.return_all = False
        self.flags = None       # L2: device word, RVLM_FLAG_SQUARE_NONFINITE if a candidate held NaN / Inf (checked after each run)
        if norm not in ('Linf', 'L2'):
            raise NotImplementedError("native SquareAttack covers norm='Linf' and 'L2'")

    def margin_and_loss(self, x, y):
        """:param y: correct labels if untargeted else target labels  (square.py:68-86)"""
        with torch.no_grad():
            logits = self.predict(x).float().clone()
        xent = F.cross_entropy(logits, y, reduction='none')   # bit-identical with the reference's bookkeeping
        z_y = logits.gather(1, y.view(-1, 1)).squeeze(1)
        z_other = logits.scatter(1, y.view(-1, 1), -float('inf')).max(dim=-1)[0]
        if self.targeted:
            return z_other - z_y, xent
        if self.loss == 'ce':
            return z_y - z_other, -1. * xent
        return z_y - z_other, z_y - z_other

    def init_hyperparam(self, x):
        assert self.norm in ['Linf', 'L2', 'L1']
        assert not self.eps is None
        assert self.loss in ['ce', 'margin']
        if self.device is None:
            self.device = x.device
        self.orig_dim = list(x.shape[1:])
        self.ndims = len(self.orig_dim)
        if self.seed is None:
            self.seed = time.time()

    # the reference's two random primitives (CPU generator, then to the device)
    def random_choice(self, shape):
        return torch.sign(2 * torch.rand(shape) - 1).to(self.device)

    def random_int(self, low=0, high=1, shape=[1]):
        return (low + (high - low) * torch.rand(shape)).long().to(self.device)

    def random_target_classes(self, y_pred, n_classes):
        y = torch.zeros_like(y_pred)
        for i in range(y_pred.shape[0]):
            others = [k for k in range(n_classes) if k != int(y_pred[i])]
            y[i] = others[int(self.random_int(0, len(others)))]
        return y.long().to(self.device)

    def eta(self, s):
        """eta(s) with its coin (square.py:187-188), drawn on the CPU generator."""
        t = eta_window(s)
        return t.permute([1, 0]) if torch.rand([1]) > 0.5 else t

    def _l2_start(self, n, c, h, w):
        """The start perturbation over eps (square.py:306-320) on the CPU, with the reference's draws: a grid of
        (h // s0) x (w // s0) tiles of side s0 = h // 5, each eta(s0) times a sign per image and channel, unit L2 norm per image."""
        if h < 5:
            raise ValueError(f"SquareAttack L2: the start tiles have side h // 5, which is 0 for h = {h}")
        s0 = h // 5
        first = (h - s0 * 5) // 2
        d = torch.zeros(n, c, h, w)
        for i in range(h // s0):
            for j in range(w // s0):
                vh, vw = first + i * s0, first + j * s0
                tile = self.eta(s0).view(1, 1, s0, s0) * torch.sign(2 * torch.rand([n, c, 1, 1]) - 1)
                if s0 > 1 and (vh + s0 > h or vw + s0 > w):
                    raise ValueError(f"SquareAttack L2: a start tile of side {s0} at ({vh}, {vw}) crosses the border of a "
                                     f"{h} x {w} image")
                d[:, :, vh:vh + s0, vw:vw + s0] += tile
        return d / ((d ** 2).view(n, -1).sum(-1).sqrt().view(-1, 1, 1, 1) + 1e-12)

    def _single_run_l2(self, x, y):
        """square.py:305-420."""
        lib = L.load()
        x = _f32c(x)
        n, c, h, w = x.shape
        n_features = c * h * w
        eps = float(self.eps)
        start = self._l2_start(n, c, h, w)                          # raises before any device work
        with torch.no_grad(), torch.cuda.device(x.device):
            if self.flags is None or self.flags.device != x.device:
                self.flags = torch.zeros(1, dtype=torch.int32, device=x.device)
            x_best = torch.clamp(x + start.to(x.device) * eps, 0., 1.).contiguous()
            margin_min, loss_min = self.margin_and_loss(x_best, y)
            n_queries = torch.ones(n, device=x.device)
            if (margin_min < 0.0).all():
                return n_queries, x_best
            x_new_buf = torch.empty_like(x)
            todo = (margin_min > 0.0).nonzero().flatten()           # the one host sync per query
            for it in range(self.n_queries):
                m = int(todo.numel())
                s = l2_window_size(it, self.n_queries, self.p_init, self.rescale_schedule, c, h, w)
                # the reference's draws, in its order, on the CPU generator; only eta and the signs travel to the device
                vh = int((0 + (h - s - 0) * torch.rand([1])).long())
                vw = int((0 + (w - s - 0) * torch.rand([1])).long())
                vh2 = int((0 + (h - s - 0) * torch.rand([1])).long())
                vw2 = int((0 + (w - s - 0) * torch.rand([1])).long())
                eta = self.eta(s).contiguous().to(x.device, non_blocking=True)
                sign = torch.sign(2 * torch.rand([m, c, 1, 1]) - 1).reshape(m, c).to(x.device, non_blocking=True)
                if m > 0:
                    x_new = x_new_buf[:m]
                    L.check(lib.rvlm_square_l2_propose(x.data_ptr(), x_best.data_ptr(), todo.data_ptr(), m, c, h, w, vh, vw, vh2, vw2,
                                                       s, eps, eta.data_ptr(), sign.data_ptr(), x_new.data_ptr(),
                                                       self.flags.data_ptr(), L.stream_ptr()), "rvlm_square_l2_propose")
                    margin, loss = self.margin_and_loss(x_new, y[todo])
                    better = (loss < loss_min[todo]).float()
                    loss_min[todo] = better * loss + (1. - better) * loss_min[todo]
                    take = torch.max(better, (margin <= 0.).float()).contiguous()
                    margin_min[todo] = take * margin + (1. - take) * margin_min[todo]
                    L.check(lib.rvlm_square_accept(x_best.data_ptr(), x_new.data_ptr(), todo.data_ptr(), take.data_ptr(), m,
                                                   n_features, L.stream_ptr()), "rvlm_square_accept")
                    n_queries[todo] += 1.
                todo = (margin_min > 0.0).nonzero().flatten()
                if self.verbose and todo.numel() != n:
                    done = (margin_min <= 0.).nonzero().flatten()
                    print('{}'.format(it + 1), '- success rate={}/{} ({:.2%})'.format(done.numel(), n, done.numel() / n),
                          '- avg # queries={:.1f}'.format(n_queries[done].mean().item()),
                          '- med # queries={:.1f}'.format(n_queries[done].median().item()),
                          '- loss={:.3f}'.format(loss_min.mean()))
                if todo.numel() == 0:
                    break
            if int(self.flags.item()) & L.FLAG_SQUARE_NONFINITE:     # square.py:416-417, once per run
                self.flags.zero_()
                raise AssertionError("SquareAttack L2: NaN / Inf in a candidate (RVLM_FLAG_SQUARE_NONFINITE)")
        return n_queries, x_best

    def attack_single_run(self, x, y):
        """Returns (queries used per sample, x_best) like square.py:221-300 (L-inf) and :305-420 (L2)."""
        if self.norm == 'L2':
            return self._single_run_l2(x, y)
        lib = L.load()
        x = _f32c(x)
        n, c, h, w = x.shape
        n_features = c * h * w
        eps = float(self.eps)
        with torch.no_grad(), torch.cuda.device(x.device):
            x_best = torch.clamp(x + eps * self.random_choice([n, c, 1, w]), 0., 1.).contiguous()
            margin_min, loss_min = self.margin_and_loss(x_best, y)
            n_queries = torch.ones(n, device=x.device)
            if (margin_min < 0.0).all():
                return n_queries, x_best
            x_new_buf = torch.empty_like(x)
            todo = (margin_min > 0.0).nonzero().flatten()           # the one host sync per query
            for it in range(self.n_queries):
                m = int(todo.numel())
                p = p_selection(it, self.n_queries, self.p_init, self.rescale_schedule)
                s = min(max(int(round(math.sqrt(p * n_features / c))), 1), min(h, w))
                # the reference's draws, in its order, on the CPU generator; only the signs travel to the device
                vh = int((0 + (h - s - 0) * torch.rand([1])).long())
                vw = int((0 + (w - s - 0) * torch.rand([1])).long())
                sign = torch.sign(2 * torch.rand([c, 1, 1]) - 1).reshape(c).to(x.device, non_blocking=True)
                if m > 0:
                    x_new = x_new_buf[:m]
                    L.check(lib.rvlm_square_linf_propose(x.data_ptr(), x_best.data_ptr(), todo.data_ptr(), m, c, h, w,
                                                         vh, vw, s, eps, sign.data_ptr(), x_new.data_ptr(),
                                                         L.stream_ptr()), "rvlm_square_linf_propose")
                    margin, loss = self.margin_and_loss(x_new, y[todo])
                    better = (loss < loss_min[todo]).float()
                    loss_min[todo] = better * loss + (1. - better) * loss_min[todo]
                    take = torch.max(better, (margin <= 0.).float()).contiguous()
                    margin_min[todo] = take * margin + (1. - take) * margin_min[todo]
                    L.check(lib.rvlm_square_accept(x_best.data_ptr(), x_new.data_ptr(), todo.data_ptr(),
                                                   take.data_ptr(), m, n_features, L.stream_ptr()), "rvlm_square_accept")
                    n_queries[todo] += 1.
                todo = (margin_min > 0.0).nonzero().flatten()
                if self.verbose and todo.numel() != n:
                    done = (margin_min <= 0.).nonzero().flatten()
                    print('{}'.format(it + 1), '- success rate={}/{} ({:.2%})'.format(done.numel(), n, done.numel() / n),
                          '- avg # queries={:.1f}'.format(n_queries[done].mean().item()),
                          '- med # queries={:.1f}'.format(n_queries[done].median().item()),
                          '- loss={:.3f}'.format(loss_min.mean()))
                if todo.numel() == 0:
                    break
        return n_queries, x_best

    def perturb(self, x, y=None):
        """:param x: clean images  :param y: untargeted: clean labels (None -> the predicted ones); targeted: target
        labels (None -> random classes different from the prediction)   (square.py:549-618)"""
        _require_cuda(x, "x")
        self.init_hyperparam(x)
        adv = x.clone()
        with torch.no_grad():
            if y is None:
                out = self.predict(x)
                pred = out.max(1)[1]
                y = self.random_target_classes(pred, out.shape[-1]) if self.targeted \
                    else pred.detach().clone().long().to(self.device)
            else:
                y = y.detach().clone().long().to(self.device)
            hit = self.predict(x).max(1)[1] == y
        acc = ~hit if self.targeted else hit
        t_start = time.time()
        torch.random.manual_seed(self.seed)
        torch.cuda.random.manual_seed(self.seed)
        for r in range(self.n_restarts):
            todo = acc.nonzero().flatten()
            if todo.numel() == 0:
                continue
            _, cand = self.attack_single_run(x[todo].clone(), y[todo].clone())
            with torch.no_grad():
                hit = self.predict(cand).max(1)[1] == y[todo]
            still = ~hit if self.targeted else hit
            broken = (still == 0).nonzero().flatten()
            acc[todo[broken]] = 0
            adv[todo[broken]] = cand[broken].clone()
            if self.verbose:
                print('restart {} - robust accuracy: {:.2%}'.format(r, acc.float().mean()),
                      '- cum. time: {:.1f} s'.format(time.time() - t_start))
        return adv
