#!/usr/bin/env python3
"""Generate tests/golden/vlm_attacks.npz by RUNNING the reference's VLM-side attacks on the CPU:
``vlm_eval.attacks.pgd.PGD`` and ``vlm_eval.attacks.apgd.APGD`` / ``apgd`` (imported at run time from the reference tree named by
the environment variable RVLM_REFERENCE; nothing of it is copied here, only arrays are written).

    RVLM_REFERENCE=<reference checkout> python tests/golden/make_golden_vlm_attacks.py

The "VLM" is a tiny seeded torch network (a strided conv, an MLP per image, a sum over the image axis and a read-out) that maps
``[1, 3, 1, 3, 8, 8]`` to the loss - a scalar for PGD, ``[1]`` for apgd.  Images are 8 x 8 rather than 16 x 16 so that the file,
which holds a gradient per model call, stays a fraction of the size limit for a committed file.

Every model call is recorded: the loss it returned and the gradient that flowed back to its input.  The tests REPLAY these traces
through the native attacks instead of re-evaluating the network on the GPU (the apgd controller compares losses at the last ulp and
the rounding of a matmul differs from host to host - the reason tests/golden/apgd_train_smallnet_*.npz are replayed too).  To
keep the traces small the network rounds the gradient it hands back to fp16 (a hook on its input, so the reference itself runs
on that gradient): L2 cases store it as fp16, L-inf cases, which read nothing but its sign, as int8 signs.

Cases: PGD, 10 steps, L-inf and L2 x mask_out in {context, query, 1, None} x mode in {min, max}, two without image_space per norm,
one with NaN injected into the gradient (on an attacked and on a masked image); apgd through ``APGD.perturb``'s arguments at
n_iter in {10, 50} with and without pert_init, all three outputs kept.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("RVLM_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "vlm_eval", "attacks")):
    sys.exit("set RVLM_REFERENCE to a checkout of the reference (it must hold vlm_eval/attacks/)")
sys.path.insert(0, REF)
OUT = os.path.join(ROOT, "tests", "golden", "vlm_attacks.npz")

from vlm_eval.attacks.pgd import PGD as RefPGD  # noqa: E402
from vlm_eval.attacks.apgd import APGD as RefAPGD, apgd as ref_apgd  # noqa: E402

N_IMG, SIDE = 3, 8
SHAPE = (1, N_IMG, 1, 3, SIDE, SIDE)


class TinyVLM(torch.nn.Module):
    def __init__(self, seed, sharp=4.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.conv_w = torch.randn(4, 3, 3, 3, generator=g) * sharp / 27 ** 0.5
        self.conv_b = torch.randn(4, generator=g) * 0.1
        self.fc1 = torch.randn(64, 16, generator=g) * sharp / 64 ** 0.5
        self.fc2 = torch.randn(16, generator=g) * sharp / 16 ** 0.5
        self.scalar = False
        self.nan_at = None          # (call index, flat positions): NaN written into that call's gradient
        self.losses, self.grads = [], []

    def weights(self):
        return {"conv_w": self.conv_w, "conv_b": self.conv_b, "fc1": self.fc1, "fc2": self.fc2}

    def forward(self, x):
        call = len(self.losses)
        self.grads.append(None)

        def hook(g):
            g = g.half().float()
            if self.nan_at is not None and self.nan_at[0] == call:
                g = g.clone()
                g.view(-1)[self.nan_at[1]] = float("nan")
            self.grads[call] = g.detach().clone()
            return g

        if x.requires_grad:
            x.register_hook(hook)
        B, n = x.shape[:2]
        h = torch.tanh(F.conv2d(x.reshape(B * n, 3, SIDE, SIDE), self.conv_w, self.conv_b, stride=2, padding=1))
        h = torch.tanh(h.flatten(1) @ self.fc1)
        loss = torch.tanh(h.view(B, n, 16).sum(1)) @ self.fc2
        self.losses.append(loss.detach().clone().reshape(-1))
        return loss.sum() if self.scalar else loss


def trace(net, signs_only):
    losses = torch.stack(net.losses).numpy().astype(np.float32)
    grads = torch.stack([torch.zeros(SHAPE) if g is None else g for g in net.grads]).numpy()
    has = np.array([g is not None for g in net.grads])
    return losses, (np.sign(grads).astype(np.int8) if signs_only else grads.astype(np.float16)), has


def main():
    out, cases = {}, []
    gen = torch.Generator().manual_seed(20240)
    x = torch.rand(SHAPE, generator=gen)
    out["x"] = x.numpy()
    net0 = TinyVLM(11)
    for k, v in net0.weights().items():
        out["w::" + k] = v.numpy()

    def run_pgd(name, norm, mask_out, mode, image_space, pert, nan_at=None, x_in=x):
        net = TinyVLM(11)
        net.scalar, net.nan_at = True, nan_at
        eps, step = (4 / 255, 1 / 255) if norm == "linf" else (0.5, 0.1)
        atk = RefPGD(net, norm, eps, mode=mode, mask_out=mask_out, image_space=image_space)
        adv, loss = atk.perturb(x_in.clone(), 10, step, perturbation=None if pert is None else pert.clone(), return_loss=True)
        losses, grads, has = trace(net, norm == "linf" and nan_at is None)
        out[name + "/adv"], out[name + "/loss"] = adv.detach().numpy(), np.float32(loss.item())
        out[name + "/losses"], out[name + "/grads"], out[name + "/has_grad"] = losses, grads, has
        if pert is not None:
            out[name + "/pert"] = pert.numpy()
        cases.append(dict(name=name, kind="pgd", norm=norm, mask_out=mask_out, mode=mode, image_space=image_space, eps=eps,
                          stepsize=step, iterations=10, pert=pert is not None, nan=nan_at is not None, shifted=x_in is not x))

    for norm in ("linf", "l2"):
        for mask_out in ("context", "query", 1, None):
            for mode in ("min", "max"):
                pert = None
                if mode == "max":               # half of the cases start from a perturbation on every image, masked ones included
                    r = 4 / 255 if norm == "linf" else 0.004
                    pert = (torch.rand(SHAPE, generator=gen) * 2 - 1) * r
                run_pgd(f"pgd_{norm}_{mask_out}_{mode}", norm, mask_out, mode, True, pert)
        # image_space=False: no [0,1] clamp, so the data may lie anywhere (shifted out of [0,1] here)
        x_shift = x * 3 - 1
        out["x_shift"] = x_shift.numpy()
        run_pgd(f"pgd_{norm}_context_min_nospace", norm, "context", "min", False, None, x_in=x_shift)
        run_pgd(f"pgd_{norm}_None_max_nospace", norm, None, "max", False, None, x_in=x_shift)
    # NaN in the gradient of call 3: two positions on the attacked (last) image and one on a masked one
    P = 3 * SIDE * SIDE
    run_pgd("pgd_linf_context_max_nan", "linf", "context", "max", True, None, nan_at=(3, [2 * P + 5, 2 * P + 77, 9]))

    def run_apgd(name, norm, mask_out, n_iter, with_init, alpha):
        net = TinyVLM(11)
        eps = 4 / 255 if norm == "linf" else 0.5
        pert = None
        if with_init:
            r = eps if norm == "linf" else 0.004
            pert = (torch.rand(SHAPE, generator=gen) * 2 - 1) * r
        atk = RefAPGD(net, norm, eps, mask_out=mask_out, initial_stepsize=alpha)
        mask = atk._set_mask(x)
        # APGD.perturb keeps only the first output of apgd(); call apgd() the way perturb does, to keep all three
        x_best, loss_best, x_best_adv = ref_apgd(net, x.clone(), norm=norm, eps=eps, n_iter=n_iter, use_rs=False, mask=mask,
                                                 alpha=alpha, n_iter_2=None, n_iter_min=None,
                                                 pert_init=None if pert is None else pert.clone())
        net2 = TinyVLM(11)
        again = RefAPGD(net2, norm, eps, mask_out=mask_out, initial_stepsize=alpha).perturb(
            x.clone(), n_iter, pert_init=None if pert is None else pert.clone())
        assert torch.equal(again, x_best)
        losses, grads, has = trace(net, norm == "linf")
        out[name + "/x_best"], out[name + "/loss_best"] = x_best.detach().numpy(), loss_best.detach().numpy()
        out[name + "/x_best_adv"] = x_best_adv.detach().numpy()
        out[name + "/losses"], out[name + "/grads"], out[name + "/has_grad"] = losses, grads, has
        if pert is not None:
            out[name + "/pert"] = pert.numpy()
        cases.append(dict(name=name, kind="apgd", norm=norm, mask_out=mask_out, n_iter=n_iter, eps=eps, alpha=alpha,
                          pert=pert is not None))

    for norm in ("linf", "l2"):
        run_apgd(f"apgd_{norm}_10", norm, "context", 10, False, 1.0)
        run_apgd(f"apgd_{norm}_10_init", norm, "query", 10, True, None)
        run_apgd(f"apgd_{norm}_50", norm, 1, 50, False, None)
        run_apgd(f"apgd_{norm}_50_init", norm, "none", 50, True, 1.0)

    h = hashlib.sha256()
    for rel in ("vlm_eval/attacks/pgd.py", "vlm_eval/attacks/apgd.py", "vlm_eval/attacks/utils.py"):
        with open(os.path.join(REF, rel), "rb") as f:
            h.update(f.read())
    out["reference_sha256"] = np.array(h.hexdigest())
    out["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
