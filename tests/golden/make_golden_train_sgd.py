#!/usr/bin/env python3
"""Golden vectors for the SGD-with-momentum optimizer step (``--opt sgd`` / ``--momentum_sgd``, train/adversarial_training_clip.py:
198-206), produced by RUNNING THE REFERENCE'S OWN ``train_one_epoch``.

Run once from the repo root:  python tests/golden/make_golden_train_sgd.py
Needs the reference checkout make_golden_train.py reads (read-only), so no test runs it; only its output
tests/golden/train_step_sgd_tiny*.npz is committed.  Everything that executes the reference is make_golden_train.py's harness,
imported from that file as it is (its module docstring says what is run from the reference and what the harness supplies); the one
difference is the optimizer,
``torch.optim.SGD(model.model.parameters(), lr, momentum=0.9, weight_decay=1e-2)`` in place of AdamW.

Inputs are NOT stored again: the seeded tiny ViT, the batches, the labels and the text head are those of train_step_tiny.npz (same
seeds; asserted equal below), and the tests read them from that file.

SGD's update is not normalised, so the learning rate decides whether the fixture can tell anything: it is chosen per case such that
for EVERY parameter tensor  3e-5 <= max|w_5 - w_0| / max|w_0| <= 5e-2  (two orders above five fp32 roundings of a parameter; small
enough that a 2e-3 gradient difference is not amplified along the trajectory).  Asserted here, re-checked by tests/test_sgd_host.py.

Recorded per case, in train_step_sgd_tiny.npz: lr_used / lr_after, loss / loss-total / cos-sims / acc / racc of every step and the
adversarial batches.  The snapshots - EVERY element of every parameter after steps 1, 3, 5 and of every momentum buffer after steps
3, 5 - are 6.9 MB, and no file may reach 1 MiB, so they go to files of their own, three per case:
  train_step_sgd_tiny_{case}_s1.npz   ``w::{key}``                       parameters after step 1
  train_step_sgd_tiny_{case}_s3.npz   ``w::{key}``, ``buf::{key}``       parameters and momentum buffers after step 3 - with
                                      lr_after[2] the whole state a reference run would have saved there (resume test)
  train_step_sgd_tiny_{case}_s5.npz   ``w::{key}``, ``buf::{key}``       the same after step 5
"""
import importlib.util
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_train", os.path.join(HERE, "make_golden_train.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                     # sets the thread count / deterministic algorithms, imports the reference

from oracle import vit_ref  # noqa: E402
from oracle.vit_ref import init_weights  # noqa: E402

CASES = {k: G.CASES[k] for k in ("fare_pgd", "tecoa_pgd", "none_cw")}
LRS = {"fare_pgd": 1e-4, "tecoa_pgd": 1e-5, "none_cw": 1e-5}
MOMENTUM, WD, WARMUP, STEPS, N_STEPS = 0.9, G.WD, G.WARMUP, G.STEPS, G.N_STEPS
W_STEPS, BUF_STEPS = (1, 3, 5), (3, 5)
RATIO_MIN, RATIO_MAX = 3e-5, 5e-2


def save(name, arrs):
    p = os.path.join(G.OUT, name)
    np.savez_compressed(p, **arrs)
    size = os.path.getsize(p)
    print(f"wrote {name}: {size / 1024:.1f} KiB")
    assert size < 2 ** 20, (name, size)


class Recorder(G.WandbRecorder):
    """Also keeps the optimizer's momentum buffers (wandb.log runs after optimizer.step() and the scheduler)."""
    optimizer = None

    def log(self, data):
        super().log(data)
        st = self.optimizer.state
        self.rows[-1]["_bufs"] = {k: st[p]["momentum_buffer"].detach().clone() for k, p in self.model.named().items()}


def main():
    cfg = vit_ref.VIT_TINY
    w = init_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(77)
    batches = [(torch.rand(G.B, 3, cfg.image_size, cfg.image_size, generator=g), torch.randint(0, G.C, (G.B,), generator=g))
               for _ in range(N_STEPS)]
    eval_batch = (torch.rand(6, 3, cfg.image_size, cfg.image_size, generator=g), torch.randint(0, G.C, (6,), generator=g))
    T = torch.nn.functional.normalize(torch.randn(cfg.out_dim, G.C, generator=g), dim=0)
    eps, step = 4 / 255, 1 / 255
    z = np.load(os.path.join(G.OUT, "train_step_tiny.npz"))
    assert np.array_equal(z["x"], np.stack([b[0].numpy() for b in batches])) and np.array_equal(z["T"], T.numpy())
    assert np.array_equal(z["y"], np.stack([b[1].numpy() for b in batches]))
    assert all(np.array_equal(z["w::" + k], v.numpy()) for k, v in w.items())
    assert float(z["eps"]) == eps and float(z["wd"]) == WD and int(z["warmup"]) == WARMUP and int(z["steps"]) == STEPS

    arrs = dict(cases=np.array(sorted(CASES)), keys=np.array(list(w)), momentum=np.float64(MOMENTUM), wd=np.float64(WD),
                warmup=np.int64(WARMUP), steps=np.int64(STEPS),
                ratio_min=np.float64(RATIO_MIN), ratio_max=np.float64(RATIO_MAX))
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None

    for name, c in CASES.items():
        lr = LRS[name]
        torch.manual_seed(1234)
        rec, adv_log = Recorder(), []
        ns = G.build_namespace(rec, adv_log)
        model, model_orig = G.TinyClipVision(cfg, w), G.TinyClipVision(cfg, w)
        rec.model = model
        optimizer = torch.optim.SGD(model.model.parameters(), lr=lr, momentum=MOMENTUM, weight_decay=WD)   # …clip.py:198-204
        rec.optimizer = optimizer
        scheduler = G.cosine_lr(optimizer, lr, WARMUP, STEPS)                                              # …clip.py:211
        lr_used = []
        inner_step = optimizer.step

        def step_and_note(*a, _inner=inner_step, _opt=optimizer, **k):
            lr_used.append(_opt.param_groups[0]["lr"])
            return _inner(*a, **k)
        optimizer.step = step_and_note
        args = types.SimpleNamespace(norm="linf", eps=eps, iterations_adv=10, stepsize_adv=step, eval_freq=1000,
                                     log_freq=1, save_checkpoints=False, steps=N_STEPS, total_epochs=1.0,
                                     output_dir="/nonexistent", **c)
        step_total = ns["train_one_epoch"](0, model=model, model_orig=model_orig, dataloader=batches,
                                           dataloader_eval=[eval_batch], optimizer=optimizer, scheduler=scheduler,
                                           embedding_text_labels_norm=T, normalize=None, args=args, epoch=0)
        assert step_total == N_STEPS and len(rec.rows) == N_STEPS and len(lr_used) == N_STEPS
        group = optimizer.state_dict()["param_groups"][0]
        assert group["momentum"] == MOMENTUM and group["dampening"] == 0 and group["nesterov"] is False
        n_train_attacks = 0 if c["attack"] == "none" else N_STEPS
        assert len(adv_log) == n_train_attacks + 1          # + the validation attack after the first step (not recorded)
        if n_train_attacks:
            adv_log.pop(1)
            arrs[f"{name}::x_adv"] = np.stack([a.numpy() for a in adv_log])
        arrs[f"{name}::lr"] = np.float64(lr)
        arrs[f"{name}::lr_used"] = np.array(lr_used, dtype=np.float64)
        arrs[f"{name}::lr_after"] = np.array([r["lr"] for r in rec.rows], dtype=np.float64)
        for key, col in (("loss", "loss"), ("loss_total", "loss-total"), ("cos_sim_clean", "cos-sim-clean"),
                         ("cos_sim", "cos-sim"), ("acc", "acc"), ("racc", "racc")):
            arrs[f"{name}::{key}"] = np.array([r[col] for r in rec.rows], dtype=np.float64)
        for s in W_STEPS:
            row, snap = rec.rows[s - 1], {}
            for k in w:
                snap["w::" + k] = row["_weights"][k].numpy()
                if s in BUF_STEPS:
                    snap["buf::" + k] = row["_bufs"][k].numpy()
            save(f"train_step_sgd_tiny_{name}_s{s}.npz", snap)
        w5 = rec.rows[N_STEPS - 1]["_weights"]
        ratios = np.array([float((w5[k].double() - v.double()).abs().max() / v.abs().max()) for k, v in w.items()])
        print(f"{name}: lr {lr:g}  lr used {lr_used}  loss {arrs[f'{name}::loss']}\n"
              f"    max|w_5 - w_0| / max|w_0| over the tensors: smallest {ratios.min():.3g}, largest {ratios.max():.3g}")
        assert RATIO_MIN <= ratios.min() and ratios.max() <= RATIO_MAX, (name, lr, ratios.min(), ratios.max())

    save("train_step_sgd_tiny.npz", arrs)

if __name__ == "__main__":
    main()
