#!/usr/bin/env python3
"""Golden vectors of the L2 Square Attack (tests/golden/square_l2_tiny.npz), made by RUNNING THE REFERENCE's autoattack package.

Run once from the repo root:  python tests/golden/make_golden_square_l2.py
Needs the reference tree (imported at run time, nothing of it is copied here); only arrays are committed.

  * eta(s) of autoattack/square.py for s in {2, 3, 5, 6, 7, 9, 21, 44, 45}, each with the outcome of its transpose coin, and the
    window sizes the reference's L2 loop asks eta() for over 5000 queries at 3 x 224 x 224 with resc_schedule=False (logged from
    a real attack_single_run on one image against a classifier that never gives way).
  * SquareAttack(norm='L2').perturb, one attack_single_run after torch.random.manual_seed(11), and AutoAttack(norm='L2',
    version='custom', ['square']) with 50 queries and bs = 4, on the tiny ViT + 10-class head, images and labels of
    make_golden.py's g9_square.

L2 candidates cannot be bit-identical across two summation orders, so a recorded trajectory must not hinge on a rounding.  For
every recorded setting this script ASSERTS, over every accept decision of the single run, min |loss - loss_min| / |loss_min|
>= 1e-4 and min |margin| >= 1e-3 (both printed), and that re-running the reference with uniform noise of +-1e-6 per pixel on the
classifier's input (a generator of its own, three noise seeds) gives identical query counters, robust flags and perturb output;
every run must leave at least one fooled and at least one robust image.  Setting "a" is eps = 0.75, margin loss, seed 5; setting
"b" is the first that passes in the printed search over eps in {1, 2, 3}, loss in {'ce', 'margin'}, seeds 0-9 (the other
arguments as in "a").
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

from autoattack.square import SquareAttack as RefSquare  # noqa: E402
from autoattack import AutoAttack as RefAutoAttack  # noqa: E402

ETA_SIZES = (2, 3, 5, 6, 7, 9, 21, 44, 45)
GAP_MIN, MARGIN_MIN, NOISE, NOISE_SEEDS = 1e-4, 1e-3, 1e-6, (0, 1, 2)
NQ, RESTARTS = 50, 2


class DecisionLog:
    """Follows the margins / losses a single run sees and keeps the two smallest distances of a decision from its threshold."""

    def __init__(self):
        self.margin_min = self.loss_min = None
        self.gap, self.margin = float("inf"), float("inf")

    def see(self, margin, loss):
        margin, loss = margin.double(), loss.double()
        self.margin = min(self.margin, margin.abs().min().item())
        if self.margin_min is None:
            self.margin_min, self.loss_min = margin.clone(), loss.clone()
            return
        act = (self.margin_min > 0).nonzero().flatten()
        assert act.numel() == margin.numel()
        lm = self.loss_min[act]
        self.gap = min(self.gap, ((loss - lm).abs() / lm.abs()).min().item())
        take = (loss < lm) | (margin <= 0)
        self.loss_min[act] = torch.where(loss < lm, loss, lm)
        self.margin_min[act] = torch.where(take, margin, self.margin_min[act])


def main():
    out = {}
    # ---- eta(s) and the coin
    holder = RefSquare(None, norm="L2", eps=1.0, device="cpu")
    torch.random.manual_seed(123)
    for s in ETA_SIZES:
        state = torch.get_rng_state()
        coin = bool(torch.rand([1]) > 0.5)
        torch.set_rng_state(state)
        out[f"eta_{s}"] = holder.eta(s).contiguous().numpy().copy()
        out[f"eta_{s}_transposed"] = np.bool_(coin)
    print("eta coins", {s: bool(out[f"eta_{s}_transposed"]) for s in ETA_SIZES})

    # ---- the window sizes of 5000 queries at 3 x 224 x 224 (resc_schedule=False), logged from the loop itself
    sizes = []
    sched = RefSquare(lambda v: torch.tensor([[1.0, 0.0]]).repeat(v.shape[0], 1), norm="L2", n_queries=5000, eps=1.0, p_init=.8,
                      resc_schedule=False, device="cpu")
    sched.init_hyperparam(torch.zeros(1, 3, 224, 224))
    eta0 = sched.eta
    sched.eta = lambda s: (sizes.append(s), eta0(s))[1]
    torch.random.manual_seed(0)
    sched.attack_single_run(torch.full((1, 3, 224, 224), 0.5), torch.zeros(1, dtype=torch.long))
    n_start = (224 // (224 // 5)) ** 2
    assert len(sizes) == n_start + 5000
    out["schedule_224"] = np.array(sizes[n_start:], dtype=np.int32)
    print("schedule: distinct sizes", sorted(set(sizes[n_start:]), reverse=True))

    # ---- attacks on the tiny ViT + 10-class head (the model, images and labels of make_golden.py g9_square)
    cfg = vit_ref.VIT_TINY
    w = init_weights(cfg, seed=3)
    g = torch.Generator().manual_seed(80)
    x = torch.rand(7, 3, cfg.image_size, cfg.image_size, generator=g)
    T = torch.randn(cfg.out_dim, 10, generator=g)
    T = T / T.norm(dim=0, keepdim=True)
    clf = vit_ref.ClassificationModelRef(cfg, w, T, 100.0).eval()
    with torch.no_grad():
        y = clf(x).max(1)[1]
    out.update(x=x.numpy(), y=y.numpy(), T=T.numpy(), weights_seed=np.int64(3))

    def run(eps, loss, seed, noise_seed=None, log=None):
        calls = []
        ng = None if noise_seed is None else torch.Generator().manual_seed(1000 + noise_seed)

        def predict(v):
            calls.append(tuple(v.shape))
            if ng is not None:
                v = v + (2 * torch.rand(v.shape, generator=ng) - 1) * NOISE
            with torch.no_grad():
                return clf(v)

        atk = RefSquare(predict, norm="L2", n_queries=NQ, eps=eps, p_init=.8, n_restarts=RESTARTS, seed=seed, verbose=False,
                        loss=loss, resc_schedule=False, device="cpu")
        adv = atk.perturb(x.clone(), y.clone())
        n_calls = len(calls)
        with torch.no_grad():
            robust = clf(adv).max(1)[1] == y
        if log is not None:
            mal = atk.margin_and_loss

            def logged(xx, yy):
                m, l = mal(xx, yy)
                log.see(m, l)
                return m, l
            atk.margin_and_loss = logged
        torch.random.manual_seed(11)
        used, xb = atk.attack_single_run(x.clone(), y.clone())
        return dict(adv=adv, robust=robust, n_calls=n_calls, used=used, xb=xb)

    def passes(eps, loss, seed):
        log = DecisionLog()
        r = run(eps, loss, seed, log=log)
        mixed = bool(r["robust"].any()) and not bool(r["robust"].all())
        with torch.no_grad():
            run_robust = clf(r["xb"]).max(1)[1] == y
        mixed = mixed and bool(run_robust.any()) and not bool(run_robust.all())
        ok = log.gap >= GAP_MIN and log.margin >= MARGIN_MIN and mixed
        stable = True
        if ok:
            for ns in NOISE_SEEDS:
                q = run(eps, loss, seed, noise_seed=ns)
                stable = stable and torch.equal(q["used"], r["used"]) and torch.equal(q["robust"], r["robust"]) and \
                    torch.equal(q["adv"], r["adv"]) and q["n_calls"] == r["n_calls"]
        print(f"eps {eps} loss {loss} seed {seed}: gap {log.gap:.2e} margin {log.margin:.2e} robust "
              f"{r['robust'].int().tolist()} single-run robust {run_robust.int().tolist()} queries {r['used'].int().tolist()} "
              f"-> {'pass' if ok and stable else 'fail'}{'' if stable else ' (moves under noise)'}")
        return r if ok and stable else None

    def record(tag, eps, loss, seed, r):
        out[f"{tag}_eps"], out[f"{tag}_loss"], out[f"{tag}_seed"] = np.float64(eps), np.array(loss), np.int64(seed)
        out[f"{tag}_n_queries"], out[f"{tag}_n_restarts"] = np.int64(NQ), np.int64(RESTARTS)
        out[f"{tag}_adv"], out[f"{tag}_robust"] = r["adv"].numpy(), r["robust"].numpy()
        out[f"{tag}_n_model_calls"] = np.int64(r["n_calls"])
        out[f"{tag}_run_queries"], out[f"{tag}_run_x_best"] = r["used"].numpy(), r["xb"].numpy()

    r = passes(0.75, "margin", 5)
    assert r is not None, "the setting the issue names does not pass its own condition"
    record("a", 0.75, "margin", 5, r)
    tags = ["a"]
    found = False
    for eps in (1.0, 2.0, 3.0):
        for loss in ("ce", "margin"):
            for seed in range(10):
                if not found:
                    r = passes(eps, loss, seed)
                    if r is not None:
                        record("b", eps, loss, seed, r)
                        tags.append("b")
                        found = True
    out["settings"] = np.array(tags)

    # ---- through AutoAttack (its own SquareAttack: p_init .8, n_restarts 1, resc_schedule False, margin loss)
    def run_aa(noise_seed=None):
        calls = []
        ng = None if noise_seed is None else torch.Generator().manual_seed(2000 + noise_seed)

        def predict(v):
            calls.append(tuple(v.shape))
            if ng is not None:
                v = v + (2 * torch.rand(v.shape, generator=ng) - 1) * NOISE
            with torch.no_grad():
                return clf(v)
        aa = RefAutoAttack(predict, norm="L2", eps=0.75, seed=0, verbose=False, version="custom", attacks_to_run=["square"],
                           device="cpu")
        aa.square.n_queries = 50
        x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=4, return_labels=True)
        return x_adv, y_adv, len(calls)

    x_adv, y_adv, n_calls = run_aa()
    for ns in NOISE_SEEDS:
        xa, ya, nc = run_aa(ns)
        assert torch.equal(xa, x_adv) and torch.equal(ya, y_adv) and nc == n_calls, "the AutoAttack run moves under noise"
    with torch.no_grad():
        robust = clf(x_adv).max(1)[1] == y
    assert bool(robust.any()) and not bool(robust.all())
    out.update(aa_eps=np.float64(0.75), aa_n_queries=np.int64(50), aa_x_adv=x_adv.numpy(), aa_y_adv=y_adv.numpy(),
               aa_robust=robust.numpy(), aa_n_model_calls=np.int64(n_calls))
    print("square-l2 aa robust", robust.int().tolist(), "calls", n_calls)
    p = os.path.join(OUT, "square_l2_tiny.npz")
    np.savez_compressed(p, **out)
    print(f"wrote square_l2_tiny.npz: {os.path.getsize(p) / 1024:.1f} KiB, settings {tags}")


if __name__ == "__main__":
    main()
