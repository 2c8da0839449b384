#!/usr/bin/env python3
"""Golden vectors of the FAB attack (tests/golden/fab_tiny.npz), made by RUNNING THE REFERENCE's autoattack package.

Run once from the repo root:  python tests/golden/make_golden_fab.py
Needs the reference tree (imported at run time, nothing of it is copied here); only arrays are committed.

  * projection_linf (autoattack/fab_projections.py) on designed rows, evaluated in float64 on the float32 inputs - the
    reference's own float32 run carries the rounding of a 150 528-term cumulative sum, which is not what a kernel should be
    held to: lambda below the smallest room, in the middle, the hyperplane missing the box, exact zeros in w, an all-zero w,
    both signs of c, t on the faces, D = 1003 (odd) and D = 3000 (a multiple of 4, not of 256); two rows at D = 150 528 rebuilt
    by tests/fab_cases.py (stored: lambda and every 997th element of d).
  * FABAttack_PT.perturb targeted / untargeted and AutoAttack(version='standard') with reduced budgets, plus 'fab-t' alone, on
    the tiny ViT + 10-class head of make_golden.py's g7_autoattack.  FAB is continuous, so the comparison is by the set of
    fooled images and the per-sample distance; eps / seeds are chosen so that every image that falls does so with a margin
    (printed below: the smallest |distance - eps| / eps, and the logit margin of every final point).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("RVLM_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import vit_ref  # noqa: E402
from oracle.vit_ref import init_weights  # noqa: E402
from tests.fab_cases import hashed_row  # noqa: E402

from autoattack.fab_projections import projection_linf  # noqa: E402
from autoattack.fab_pt import FABAttack_PT  # noqa: E402
from autoattack import AutoAttack as RefAutoAttack  # noqa: E402


def ref_projection64(t, w, b):
    d = projection_linf(torch.from_numpy(t).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double())
    return d.numpy()


def designed_rows(D, seed):
    g = np.random.default_rng(seed)
    rows = []

    def add(t, w, c):
        t, w = t.astype(np.float32), w.astype(np.float32)
        rows.append((t, w, np.float32(np.dot(w.astype(np.float64), t.astype(np.float64)) + c)))
    inner = lambda: g.uniform(0.2, 0.8, D)          # noqa: E731
    full = lambda: g.uniform(0.0, 1.0, D)           # noqa: E731
    w = g.standard_normal(D)
    add(inner(), w, 0.1 * np.abs(w).sum())                      # lambda = 0.1, below the smallest room (0.2)
    add(inner(), w, -0.05 * np.abs(w).sum())                    # the same, c < 0
    w = g.standard_normal(D)
    add(full(), w, 0.25 * np.abs(w).sum())                      # lambda in the middle of the rooms
    add(full(), w, -0.4 * np.abs(w).sum())
    add(full(), w, 2.0 * np.abs(w).sum())                       # the hyperplane misses the box
    add(full(), w, -3.0 * np.abs(w).sum())
    w = g.standard_normal(D) * (g.uniform(size=D) > 0.4)        # exact zeros in w
    add(full(), w, 0.2 * np.abs(w).sum())
    add(full(), np.zeros(D), 1.5)                               # all-zero w
    t = np.round(g.uniform(size=D))                             # t on the faces
    w = g.standard_normal(D)
    add(t, w, 0.1 * np.abs(w).sum())
    t = full(); t[::3] = 0.0; t[1::3] = 1.0
    add(t, w, -0.3 * np.abs(w).sum())
    t, w, b = (np.stack([r[i] for r in rows]) for i in range(3))
    return t, w, b


def main():
    out = {}
    # ---- projection
    for tag, D, seed in (("p1003", 1003, 11), ("p3000", 3000, 12)):
        t, w, b = designed_rows(D, seed)
        d = ref_projection64(t, w, b)
        out[f"{tag}_t"], out[f"{tag}_w"], out[f"{tag}_b"] = t, w, b
        out[f"{tag}_d"] = d.astype(np.float32)
        out[f"{tag}_lambda"] = np.abs(d).max(1)
    D = 150528
    big = [(1, 300.0), (2, -5000.0)]
    lam, samp = [], []
    for salt, off in big:
        t, w, b = hashed_row(D, salt, off)
        d = ref_projection64(t[None], w[None], np.array([b]))[0]
        lam.append(np.abs(d).max())
        samp.append(d[::997].astype(np.float32))
    out["big_D"], out["big_salt_offset"] = np.int64(D), np.array(big, dtype=np.float64)
    out["big_lambda"], out["big_d_stride997"] = np.array(lam), np.stack(samp)

    # ---- attacks on the tiny ViT + 10-class head (the model of make_golden.py g7_autoattack)
    cfg = vit_ref.VIT_TINY
    w = init_weights(cfg, seed=3)
    g = torch.Generator().manual_seed(80)
    x = torch.rand(7, 3, cfg.image_size, cfg.image_size, generator=g)
    T = torch.randn(cfg.out_dim, 10, generator=g)
    T = T / T.norm(dim=0, keepdim=True)
    clf = vit_ref.ClassificationModelRef(cfg, w, T, 100.0).eval()
    with torch.no_grad():
        y = clf(x).max(1)[1]
    calls = []

    def predict(v):
        calls.append(tuple(v.shape))
        return clf(v)

    def summary(tag, adv, eps):
        with torch.no_grad():
            z = clf(adv)
        dist = (adv - x).abs().reshape(7, -1).max(1)[0]
        top2 = z.topk(2, dim=1)[0]
        moved = dist > 0
        edge = ((dist[moved] - eps).abs() / eps).min().item() if moved.any() else float("nan")
        print(f"{tag}: fooled {(z.max(1)[1] != y).int().tolist()} dist/eps {(dist / eps).numpy().round(3).tolist()} "
              f"min |dist-eps|/eps {edge:.3f} min logit margin {(top2[:, 0] - top2[:, 1]).min().item():.3f} calls {len(calls)}")
        out[f"{tag}_dist"] = dist.double().numpy()
        out[f"{tag}_fooled"] = (z.max(1)[1] != y).numpy()
        out[f"{tag}_y_adv"] = z.max(1)[1].numpy()
        out[f"{tag}_n_model_calls"] = np.int64(len(calls))

    # eps = 3.5 / 255: FAB's minimum-norm results on these images are 0.3, 2.0, 2.8 and 2.8 - 3.0 / 255 (they fall, at least 15 %
    # inside eps) and 3.8 / 255 or more (they survive, at least 9 % outside); at 3 / 255 and 4 / 255 one image sits within 1 - 4 %
    eps = float(os.environ.get("FAB_EPS", 3.5)) / 255
    out.update(x=x.numpy(), y=y.numpy(), T=T.numpy(), eps=np.float64(eps), weights_seed=np.int64(3), n_iter=np.int64(10),
               n_target_classes=np.int64(3), bs=np.int64(4), iterations_apgd=np.int64(6), square_queries=np.int64(50))
    calls.clear()
    atk = FABAttack_PT(predict, norm="Linf", n_restarts=1, n_iter=10, eps=eps, seed=0, targeted=True, device="cpu",
                       n_target_classes=3)
    summary("fabt", atk.perturb(x.clone(), y.clone()), eps)
    calls.clear()
    atk = FABAttack_PT(predict, norm="Linf", n_restarts=2, n_iter=10, eps=eps, seed=0, targeted=False, device="cpu")
    summary("fab", atk.perturb(x.clone(), y.clone()), eps)
    for tag, kw in (("aa_std", dict(version="standard")), ("aa_fabt", dict(version="custom", attacks_to_run=["fab-t"]))):
        calls.clear()
        aa = RefAutoAttack(predict, norm="Linf", eps=eps, seed=0, verbose=False, device="cpu", alpha=2.0, iterations_apgd=6,
                           use_rs=True, **kw)
        aa.apgd.n_restarts, aa.apgd_targeted.n_target_classes = 1, 3
        aa.fab.n_iter, aa.fab.n_target_classes, aa.fab.n_restarts = 10, 3, 1
        aa.square.n_queries = 50
        x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=4, return_labels=True)
        summary(tag, x_adv, eps)
        out[f"{tag}_y_adv_returned"] = y_adv.numpy()
    p = os.path.join(OUT, "fab_tiny.npz")
    np.savez_compressed(p, **out)
    print(f"wrote fab_tiny.npz: {os.path.getsize(p) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
