#!/usr/bin/env python
"""Throughput of the native text tower on the zero-shot head workloads: 1000 prompts x 1 template and 1000 x 80 templates
(CLIP_eval/eval_utils.py:63-85, CLIP_eval/clip_robustbench.py:211-224), each precision, with the automatic active length and at the
full context.  Seeded weights and seeded token ids (prompt lengths 8-20, as "This is a photo of a {}" tokenises).  Warm-up calls,
then the median of the timed calls, each between two stream synchronisations.  One process, one GPU; one JSON line per configuration.

    python scripts/bench_text_head.py [--model ViT-L-14] [--precisions x3,bf16,fp32] [--templates 1,80] [--calls 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import robustvlm_amd as R  # noqa: E402


def seeded_prompts(n, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(n, cfg.context, dtype=torch.int32)
    lens = torch.randint(8, 21, (n,), generator=g)
    body = torch.randint(1, cfg.vocab - 2, (n, cfg.context), generator=g, dtype=torch.int32)
    pos = torch.arange(cfg.context).expand(n, -1)
    tok = torch.where(pos < (lens - 1)[:, None], body, tok)
    tok[:, 0] = cfg.vocab - 2
    tok[torch.arange(n), lens - 1] = cfg.vocab - 1
    return tok


def gemm_flops_per_token(cfg):
    return 2.0 * cfg.layers * 12 * cfg.width * cfg.width      # qkv 3 W^2 + out W^2 + fc1 4 W^2 + fc2 4 W^2, 2 FLOP per MAC


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--precisions", default="x3,bf16,fp32")
    ap.add_argument("--templates", default="1,80")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=1024)
    args = ap.parse_args()
    cfg = R.TEXT_CONFIGS[args.model]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sd = R.random_text_state_dict(cfg, seed=0, device=dev)
    for precision in args.precisions.split(","):
        eng = R.TextEngine(cfg, sd, precision=precision, max_batch=args.max_batch)
        model = R.ClipTextModel(eng)
        for n_t in (int(v) for v in args.templates.split(",")):
            n = args.classes * n_t
            tok = seeded_prompts(n, cfg, seed=n_t).to(dev)
            auto = R.TextEngine.active_length(tok)
            for active in (auto, 0):
                # the per-call work as the user pays for it: the head arithmetic included (normalise / ensemble average)
                def call():
                    if n_t == 1:
                        return eng.encode(tok, normalize=True, active_len=active).T
                    return R.zeroshot_head(eng.encode(tok, normalize=False, active_len=active).reshape(args.classes, n_t, -1))
                for _ in range(args.warmup):
                    call()
                ms = []
                for _ in range(args.calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                med = statistics.median(ms)
                positions = active or cfg.context
                print(json.dumps({
                    "bench": "text_head", "model": args.model, "precision": precision, "prompts": n, "templates": n_t,
                    "active_len": positions, "full_context": active == 0, "ms_per_call": round(med, 3),
                    "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": args.calls, "warmup": args.warmup,
                    "prompts_per_s": round(n / med * 1e3, 1),
                    # algorithmic FLOPs of the linears over the evaluated positions / the whole call's time: a lower bound of the
                    # in-kernel GEMM rate (the call also holds attention, LayerNorm, the head and the host loop over chunks)
                    "gemm_tflops": round(gemm_flops_per_token(cfg) * n * positions / (med * 1e-3) / 1e12, 2),
                    "max_batch": args.max_batch, "workspace_gib": round(eng.workspace_bytes / 2 ** 30, 2)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
