#!/usr/bin/env python3
"""Golden vectors of the attacks at the dataset's own resolution (tests/golden/attacks_resize_tiny.npz), made by RUNNING THE
REFERENCE's attack code with the bicubic resizer inside the model.

Run once from the repo root:  python tests/golden/make_golden_resize.py
Needs the reference tree (imported at run time, nothing of it is copied here); only arrays are committed.

CLIP_eval/clip_robustbench.py:60-68,104-114 builds ``ClassificationModel(..., resizer=Resize(224, BICUBIC, antialias=False))`` for
CIFAR: images, perturbation and eps ball are 32 x 32, the up-sampling is part of the model.  Here: the tiny ViT (32 x 32, patch 8)
+ 10-class head of make_golden.py behind ``resizer = F.interpolate(x, 32, mode='bicubic', align_corners=False)`` - what
torchvision's Resize runs on a float tensor - at input sizes 16 (integer scale) and 12 (scale 8 / 3):

  * APGDAttack(loss='ce', n_restarts=2).perturb             (autoattack/autopgd_base.py)
  * AutoAttack(version='custom', ['apgd-ce', 'apgd-t'])     (autoattack/autoattack.py), robust flags after each stage
  * pgd(), cross-entropy on the zero-shot head, mode='max'  (train/pgd_train.py)
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("RVLM_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import vit_ref  # noqa: E402
from oracle.vit_ref import init_weights, ClipVisionModelRef  # noqa: E402

from train.pgd_train import pgd as ref_pgd  # noqa: E402
from autoattack.autopgd_base import APGDAttack as RefAPGDAttack  # noqa: E402
from autoattack import AutoAttack as RefAutoAttack  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(OUT, "make_golden.py"))
_mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mg)          # the reference's loss wrappers, exec'd from its own source (make_golden.py)
REFL, weights_digest = _mg.REFL, _mg.weights_digest

N_ITER, N_TARGET, BS = 8, 3, 4


def main():
    cfg = vit_ref.VIT_TINY
    w = init_weights(cfg, seed=3)
    out = dict(weights_seed=np.int64(3), weights_sha256=np.array(weights_digest(w)), n_iter=np.int64(N_ITER),
               n_target_classes=np.int64(N_TARGET), bs=np.int64(BS), sizes=np.array([16, 12]))
    for size, seed, eps in ((16, 92, 4 / 255), (12, 91, 8 / 255)):      # mixed robust sets, clean margins 1.5 - 15 (no saturated CE)
        g = torch.Generator().manual_seed(seed)
        B = 7
        x = torch.rand(B, 3, size, size, generator=g)
        T = torch.randn(cfg.out_dim, 10, generator=g)
        T = T / T.norm(dim=0, keepdim=True)
        resizer = lambda v: F.interpolate(v, (cfg.image_size, cfg.image_size), mode="bicubic", align_corners=False)  # noqa: E731
        head = vit_ref.ClassificationModelRef(cfg, w, T, 100.0).eval()
        clf = lambda v: head(resizer(v))  # noqa: E731
        with torch.no_grad():
            y = clf(x).max(1)[1]
        tag = f"s{size}_"
        out.update({tag + "x": x.numpy(), tag + "y": y.numpy(), tag + "T": T.numpy(), tag + "eps": np.float64(eps)})
        with torch.no_grad():
            out[tag + "logits"] = clf(x).numpy()

        # (a) APGD-CE, two restarts, + the loss of the best point of a single run (attack_single_run's loss_best)
        atk = RefAPGDAttack(clf, n_iter=N_ITER, norm="Linf", n_restarts=2, eps=eps, seed=0, loss="ce", device="cpu",
                            alpha=2.0, use_rs=True)
        adv = atk.perturb(x.clone(), y.clone())
        with torch.no_grad():
            out[tag + "apgd_adv"] = adv.numpy()
            out[tag + "apgd_robust"] = (clf(adv).max(1)[1] == y).numpy()
        atk.init_hyperparam(x)
        torch.random.manual_seed(0)
        _, acc1, loss_best, xba = atk.attack_single_run(x.clone(), y.clone())
        out[tag + "run_acc"] = acc1.numpy()
        out[tag + "run_loss_best"] = loss_best.detach().numpy()
        out[tag + "run_x_best_adv"] = xba.detach().numpy()

        # (b) AutoAttack custom: apgd-ce then apgd-t
        aa = RefAutoAttack(clf, norm="Linf", eps=eps, seed=0, verbose=False, version="custom",
                           attacks_to_run=["apgd-ce", "apgd-t"], device="cpu", alpha=2.0, iterations_apgd=N_ITER, use_rs=True)
        aa.apgd.n_restarts = 1
        aa.apgd_targeted.n_target_classes = N_TARGET
        x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=BS, return_labels=True)
        with torch.no_grad():
            out[tag + "aa_x_adv"] = x_adv.numpy()
            out[tag + "aa_y_adv"] = y_adv.numpy()
            out[tag + "aa_robust"] = (clf(x_adv).max(1)[1] == y).numpy()
        aa1 = RefAutoAttack(clf, norm="Linf", eps=eps, seed=0, verbose=False, version="custom", attacks_to_run=["apgd-ce"],
                            device="cpu", alpha=2.0, iterations_apgd=N_ITER, use_rs=True)
        aa1.apgd.n_restarts = 1
        xa1 = aa1.run_standard_evaluation(x.clone(), y.clone(), bs=BS)
        with torch.no_grad():
            out[tag + "aa_robust_after_ce"] = (clf(xa1).max(1)[1] == y).numpy()

        # (c) pgd(), TeCoA's loss (cross-entropy of the head on the normalised embedding), ascending
        model = ClipVisionModelRef(cfg, w).eval()
        fwd = lambda v, output_normalize: model(resizer(v), output_normalize)  # noqa: E731
        wrap = REFL["ComputeLossWrapper"](None, T, "mean", "ce", 100.)
        d0 = torch.zeros_like(x).uniform_(-eps, eps, generator=g)
        xadv = ref_pgd(fwd, wrap, x, y, "linf", eps, 10, eps / 4, True, perturbation=d0.clone().requires_grad_(True), mode="max")
        out[tag + "pgd_delta0"] = d0.numpy()
        out[tag + "pgd_xadv"] = xadv.detach().numpy()
        with torch.no_grad():
            out[tag + "pgd_loss_final"] = np.float32(wrap(fwd(xadv, True), y).item())
            out[tag + "pgd_loss_start"] = np.float32(wrap(fwd(x + d0, True), y).item())
        print(f"size {size}: eps {eps:.4f}  apgd robust {out[tag + 'apgd_robust'].astype(int)}  "
              f"aa after ce {out[tag + 'aa_robust_after_ce'].astype(int)}  aa {out[tag + 'aa_robust'].astype(int)}  "
              f"pgd loss {out[tag + 'pgd_loss_start']:.4f} -> {out[tag + 'pgd_loss_final']:.4f}")
    p = os.path.join(OUT, "attacks_resize_tiny.npz")
    np.savez_compressed(p, **out)
    print(f"wrote {os.path.basename(p)}: {os.path.getsize(p) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
