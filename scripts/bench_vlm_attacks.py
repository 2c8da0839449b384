#!/usr/bin/env python
"""Milliseconds per iteration of the VLM-side APGD (L-inf) at the two shapes the reference attacks:
``[1, 5, 1, 3, 224, 224]`` (OpenFlamingo: 4 context images + 1 query, mask_out='context') and ``[1, 1, 1, 3, 336, 336]`` (LLaVA,
mask_out=None).

(i)  the attack arithmetic alone - everything of an iteration but the model: the native loop (rvlm_apgd_masked_step +
     rvlm_apgd_masked_bookkeeping, 3 launches, no read-back) next to the reference loop's torch operations on the same GPU, written
     out below from vlm_eval/attacks/apgd.py:240-266 (L-inf branch) and :321-351 (not imported).  Both get the loss and the
     gradient of each iteration from the same pre-computed device tensors, so no model time is in either number.  The torch
     loop's ``nonzero()`` calls (each a host synchronisation) are counted.
(ii) the engine route end to end: ``APGD(TokenLossModel(...)).perturb`` on ViT-L/14 (224 px, 5 images) and ViT-L/14-336 (1 image),
     bf16, seeded weights - forward, token loss, input gradient and the attack arithmetic.

One process, one GPU.  Every timed region runs under its own time limit (SIGALRM); the script stops at the first region that fails
or runs out of time and exits non-zero.  One JSON line per region.

    python scripts/bench_vlm_attacks.py [--iters 100] [--repeats 5] [--engine-iters 20] [--limit 120]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import robustvlm_amd as R  # noqa: E402
from robustvlm_amd.vlm_attacks import APGD, TokenLossModel, apgd  # noqa: E402

EPS = 4 / 255


class Scripted:
    """Stands for the VLM: call c returns losses[c]; the gradient handed back is grads[c % len(grads)]."""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, value, G):
            ctx.G = G
            return value.clone()

        @staticmethod
        def backward(ctx, go):
            return ctx.G.clone(), None, None

    def __init__(self, losses, grads):
        self.losses, self.grads, self.calls = losses, grads, 0

    def __call__(self, x):
        c = self.calls
        self.calls += 1
        return self._Fn.apply(x, self.losses[c], self.grads[c % len(self.grads)])


def torch_apgd_linf(model, x, eps, n_iter, mask, alpha, counts):
    """The reference loop, L-inf branch, operation for operation (apgd.py:171-237 set-up, :239-266 step, :291-351 bookkeeping)."""
    def nz(t):
        counts["nonzero"] += 1
        return t.nonzero().squeeze()

    x_adv = x.clone().clamp(0., 1.)
    x_best = x_adv.clone()
    x_best_adv = x_adv.clone()
    loss_steps = torch.zeros([n_iter, x.shape[0]], device=x.device)
    loss_best_steps = torch.zeros([n_iter + 1, x.shape[0]], device=x.device)
    n_iter_2, n_iter_min, size_decr = max(int(0.22 * n_iter), 1), max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1)
    k = n_iter_2 + 0
    step_size = alpha * eps * torch.ones([x.shape[0], *[1] * (len(x.shape) - 1)], device=x.device)
    counter3 = 0
    x_adv.requires_grad_()
    with torch.enable_grad():
        loss_indiv = model(x_adv)
        loss = loss_indiv.sum()
    grad = torch.autograd.grad(loss, [x_adv])[0].detach()
    grad *= mask
    grad_best = grad.clone()
    x_adv.detach_()
    loss_indiv = loss_indiv.detach()
    loss_best = loss_indiv.detach().clone()
    loss_best_last_check = loss_best.clone()
    reduced_last_check = torch.ones_like(loss_best)
    x_adv_old = x_adv.clone().detach()
    for i in range(n_iter):
        x_adv = x_adv.detach()
        grad2 = x_adv - x_adv_old
        x_adv_old = x_adv.clone()
        a = 0.75 if i > 0 else 1.0
        x_adv_1 = x_adv + step_size * torch.sign(grad)
        x_adv_1 = torch.clamp(torch.min(torch.max(x_adv_1, x - eps), x + eps), 0.0, 1.0)
        x_adv_1 = torch.clamp(torch.min(torch.max(x_adv + (x_adv_1 - x_adv) * a + grad2 * (1 - a), x - eps), x + eps), 0.0, 1.0)
        x_adv = x_adv_1 + 0.
        x_adv.requires_grad_()
        with torch.enable_grad():
            loss_indiv = model(x_adv)
            loss = loss_indiv.sum()
        if i < n_iter - 1:
            grad = torch.autograd.grad(loss, [x_adv])[0].detach()
            grad *= mask
        x_adv.detach_()
        loss_indiv = loss_indiv.detach()
        x_best_adv = x_adv + 0.
        y1 = loss_indiv.detach().clone()
        loss_steps[i] = y1 + 0
        ind = nz(y1 > loss_best)
        x_best[ind] = x_adv[ind].clone()
        grad_best[ind] = grad[ind].clone()
        loss_best[ind] = y1[ind] + 0
        loss_best_steps[i + 1] = loss_best + 0
        counter3 += 1
        if counter3 == k:
            t = torch.zeros(loss_steps.shape[1]).to(x.device)
            for counter5 in range(k):
                t += (loss_steps[i - counter5] > loss_steps[i - counter5 - 1]).float()
            fl_oscillation = (t <= k * 0.75 * torch.ones_like(t)).float()
            fl_reduce_no_impr = (1. - reduced_last_check) * (loss_best_last_check >= loss_best).float()
            fl_oscillation = torch.max(fl_oscillation, fl_reduce_no_impr)
            reduced_last_check = fl_oscillation.clone()
            loss_best_last_check = loss_best.clone()
            counts["sync"] += 1
            if fl_oscillation.sum() > 0:
                ind_fl_osc = nz(fl_oscillation > 0)
                step_size[ind_fl_osc] /= 2.0
                x_adv[ind_fl_osc] = x_best[ind_fl_osc].clone()
                grad[ind_fl_osc] = grad_best[ind_fl_osc].clone()
            counter3 = 0
            k = max(k - size_decr, n_iter_min)
    return x_best, loss_best, x_best_adv


class Limit:
    """One timed region: a time limit of its own, a JSON line, False on failure."""

    def __init__(self, seconds):
        self.seconds = seconds

    def run(self, name, fn):
        def on_alarm(signum, frame):
            raise TimeoutError(f"{name}: over {self.seconds} s")
        signal.signal(signal.SIGALRM, on_alarm)
        signal.alarm(self.seconds)
        try:
            out = fn()
            torch.cuda.synchronize()
        except Exception as e:   # noqa: BLE001
            print(json.dumps({"region": name, "status": 1, "error": f"{type(e).__name__}: {e}"}), flush=True)
            return False
        finally:
            signal.alarm(0)
        print(json.dumps({"region": name, "status": 0, **out}), flush=True)
        return True


def wall_ms(fn, repeats):
    """Median / min / max wall milliseconds of fn() + device synchronise, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engine-iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lim = Limit(args.limit)
    shapes = (("openflamingo_5x224", (1, 5, 1, 3, 224, 224), "context", "ViT-L-14"),
              ("llava_1x336", (1, 1, 1, 3, 336, 336), None, "ViT-L-14-336"))
    n = args.iters
    for tag, shape, mask_out, model_name in shapes:
        g = torch.Generator().manual_seed(0)
        x = torch.rand(shape, generator=g).to(dev)
        grads = torch.randn((4,) + shape, generator=g).to(dev)
        losses = torch.cumsum(torch.randn(n + 1, 1, generator=g), 0).to(dev)
        atk = APGD(None, "linf", EPS, mask_out=mask_out, initial_stepsize=1.0)
        mask_bytes = atk._set_mask(x)
        mask_full = mask_bytes.view(1, -1, 1, 1, 1, 1).expand(shape).float().contiguous()

        def arithmetic():
            counts = {"nonzero": 0, "sync": 0}
            native = lambda: apgd(Scripted(losses, grads), x, "linf", EPS, n_iter=n, mask=mask_bytes, alpha=1.0)   # noqa: E731
            ref = lambda: torch_apgd_linf(Scripted(losses, grads), x, EPS, n, mask_full, 1.0, counts)             # noqa: E731
            a, b = native(), ref()
            same = bool(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]))
            counts.update(nonzero=0, sync=0)
            ref()
            syncs = (counts["nonzero"] + counts["sync"]) / n
            # alternate the two loops so that both see the same machine
            tn, tr = [], []
            for _ in range(args.repeats):
                tn.append(wall_ms(native, 1)[0])
                tr.append(wall_ms(ref, 1)[0])
            return {"shape": list(shape), "elements": x.numel(), "iterations": n, "same_outputs": same,
                    "native_ms_per_iter": statistics.median(tn) / n, "native_min_max": [min(tn) / n, max(tn) / n],
                    "torch_loop_ms_per_iter": statistics.median(tr) / n, "torch_min_max": [min(tr) / n, max(tr) / n],
                    "native_launches_per_iter": 3, "native_host_syncs_per_iter": 0, "torch_loop_host_syncs_per_iter": syncs}

        if not lim.run(f"arithmetic_{tag}", arithmetic):
            return 1

        def engine():
            cfg = R.CONFIGS[model_name]
            n_img = shape[1]
            eng = R.VitEngine(cfg, R.random_state_dict(cfg, seed=0, device=dev), precision="bf16", max_batch=n_img)
            try:
                tower = R.ClipVisionTower(eng, select_layer=-2, select_feature="patch").eval()
                with torch.no_grad():
                    ref_tok = tower(x.reshape(-1, *shape[-3:])).clone()
                d0 = ((torch.rand(shape, generator=g) * 2 - 1) * EPS).to(dev)
                atk = APGD(TokenLossModel(tower, ref_tok), "linf", EPS, mask_out=mask_out, initial_stepsize=1.0)
                it = args.engine_iters
                med, lo, hi = wall_ms(lambda: atk.perturb(x, it, pert_init=d0), args.repeats)
                return {"model": model_name, "precision": "bf16", "shape": list(shape), "iterations": it,
                        "ms_per_iter": med / (it + 1), "min_max": [lo / (it + 1), hi / (it + 1)],
                        "note": "per model call: n_iter + 1 calls per perturb"}
            finally:
                eng.close()

        if not lim.run(f"engine_{tag}", engine):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
