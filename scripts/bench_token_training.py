#!/usr/bin/env python
"""Milliseconds per training step of the token loss (loss="l2-tokens") next to the pooled step of the same build.

ViT-L/14 bf16, seeded weights, B random 224 x 224 images, L-inf 4/255, --iters-adv PGD steps, AdamW.  Three trainers of one
process on one GPU: the pooled step (FARE's embedding l2), the token step at token_depth = layers - 1 (LLaVA's tower) and at
token_depth = layers (OpenFlamingo's), patch rows.  Per trainer and round, HIP events around

    attack            the inner PGD loop
    forward           the saving forward alone (save = 2)
    forward_backward  forward + loss + weight gradients (what the step runs); backward = forward_backward - forward
    optimizer         the fused optimizer launch over the span the step moves + the refresh of the engine's GEMM copies
    step              one whole train_step (frozen-model pass, attack, clean pass for the metrics, the above)

The trainers ALTERNATE inside every round, so that a drift of the clocks or a neighbour on the host meets all three alike; the
medians over --rounds rounds and the spread (min, max) go out as one JSON line per trainer.  There is no pass / fail threshold.

    python scripts/bench_token_training.py [--batch 128] [--iters-adv 10] [--rounds 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import robustvlm_amd as R  # noqa: E402
from robustvlm_amd.trainer import AdversarialTrainer  # noqa: E402
from benchlib import host_cpu_info  # noqa: E402


def ms_of(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Arm:
    """One trainer and the pieces of its step as callables."""

    def __init__(self, name, cfg, sd, B, iters_adv, x, **kw):
        self.name, self.x = name, x
        self.tr = tr = AdversarialTrainer(cfg, sd, batch_size=B, precision="bf16", attack="pgd", iterations_adv=iters_adv,
                                          metrics=True, **kw)
        eng = tr.engine
        with torch.no_grad():
            if tr.token_mode:
                self.ref = tr._select_rows(tr.engine_orig.forward_tokens(x, depth=tr.token_depth)).contiguous()
            else:
                self.ref = tr.model_orig(x, False)
        if tr.token_mode:
            self.x_adv = tr._attack_tokens(x, self.ref)
            self.phases = {
                "attack": lambda: tr._attack_tokens(x, self.ref),
                "forward": lambda: eng.forward_tokens(self.x_adv, depth=tr.token_depth, save=2),
                "forward_backward": lambda: tr._tokens_loss_backward(self.x_adv, self.ref, 1.0, False, False),
                "optimizer": lambda: (tr._optimizer_step(tr._token_span_lo), eng.load_state_dict(tr.params.views)),
            }
        else:
            self.x_adv = tr._attack(x, None, self.ref)
            self.phases = {
                "attack": lambda: tr._attack(x, None, self.ref),
                "forward": lambda: eng.forward(self.x_adv, None, False, save=2),
                "forward_backward": lambda: tr._loss_backward(self.x_adv, None, self.ref, "l2", None, 1.0, False, False),
                "optimizer": lambda: (tr._optimizer_step(), eng.load_state_dict(tr.params.views)),
            }
        self.phases["step"] = lambda: tr.train_step(x, None)
        self.ms = {k: [] for k in self.phases}

    def round(self, keep):
        self.tr.step_total = max(self.tr.step_total, 1)      # (the optimizer phase alone: AdamW's bias correction needs step >= 1)
        for k, fn in self.phases.items():
            t = ms_of(fn)
            if keep:
                self.ms[k].append(t)

    def result(self):
        out = {}
        for k, v in self.ms.items():
            out[k] = dict(ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3))
        out["backward_derived"] = dict(ms_median=round(out["forward_backward"]["ms_median"] - out["forward"]["ms_median"], 3),
                                       how="forward_backward - forward (medians)")
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters-adv", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_training.py needs an MI355X: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = R.CONFIGS[args.model]
    B = args.batch
    sd = R.random_state_dict(cfg, seed=0, device=dev)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(0)).to(dev)
    tok = dict(loss="l2-tokens", inner_loss="l2-tokens", token_select="patch")
    arms = [Arm("pooled", cfg, sd, B, args.iters_adv, x),
            Arm(f"tokens_depth_{cfg.layers - 1}", cfg, sd, B, args.iters_adv, x, token_depth=cfg.layers - 1, **tok),
            Arm(f"tokens_depth_{cfg.layers}", cfg, sd, B, args.iters_adv, x, token_depth=cfg.layers, **tok)]
    for r in range(args.warmup + args.rounds):
        for arm in arms:
            arm.round(keep=r >= args.warmup)
    cpu, cores, _ = host_cpu_info()
    common = dict(bench="token_training_step", model=args.model, precision="bf16", batch=B, iterations_adv=args.iters_adv,
                  rounds=args.rounds, warmup=args.warmup, device=torch.cuda.get_device_name(dev), host=f"{cpu} ({cores} cores)",
                  timing="HIP events around each phase, one process, arms alternating inside every round")
    for arm in arms:
        reached = arm.tr.params.numel - (arm.tr._token_span_lo if arm.tr.token_mode else 0)
        print(json.dumps(dict(arm=arm.name, params_moved=reached, params_total=arm.tr.params.numel, **arm.result(), **common)),
              flush=True)
        arm.tr.close()


if __name__ == "__main__":
    main()
