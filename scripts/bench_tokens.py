#!/usr/bin/env python
"""Rate of the token-FARE attack loop next to the pooled loop, and the token loss + seed kernel alone.

ViT-L/14 bf16, seeded weights, B random 224 x 224 images, L-inf 4/255, 10-step PGD from a random start:
(i)   the pooled loop (rvlm_pgd_run_norm, FARE's embedding l2) - the yardstick;
(ii)  the token loop at depth = layers - 1, patch rows (LLaVA's tower) and at depth = layers, patch rows (OpenFlamingo's tower,
      class-token tail bypassed) - rvlm_pgd_run_tokens;
(iii) rvlm_tokens_l2_loss_grad alone at [B, 257, 1024] with the seed written as bf16 only, as fp32 only and as both: microseconds
      (HIP events, median of --iters calls) and the algorithmic bytes over that time.
One process, one GPU; one JSON line per part.

    python scripts/bench_tokens.py [--batch 128] [--steps 10] [--repeats 5] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import robustvlm_amd as R  # noqa: E402
from robustvlm_amd import _lib as L  # noqa: E402


def timed(fn, n, warmup):
    """Median / min / max milliseconds of n calls (HIP events), after warm-up calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    cfg = R.CONFIGS[args.model]
    B = args.batch
    eng = R.VitEngine(cfg, R.random_state_dict(cfg, seed=0, device=dev), precision="bf16", max_batch=B)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
    eps = 4 / 255
    d0 = ((torch.rand(x.shape, generator=g) * 2 - 1) * eps).to(dev)
    common = dict(model=args.model, precision="bf16", batch=B, steps=args.steps, device=torch.cuda.get_device_name(dev))

    e0 = eng.forward(x)
    loops = {"pooled": lambda: eng.pgd_run(x, d0, "l2", "mean", e0, None, False, eps, args.steps, eps / 4, 0.9, "max")}
    for name, depth in (("tokens_depth_L-1", cfg.layers - 1), ("tokens_depth_L", cfg.layers)):
        ref = eng.forward_tokens(x, depth=depth)[:, 1:].contiguous()
        loops[name] = (lambda ref=ref, depth=depth: eng.pgd_run_tokens(x, d0, ref, eps, args.steps, eps / 4, 0.9, "max", depth=depth,
                                                                       select="patch"))
    for name, fn in loops.items():
        med, lo, hi = timed(fn, args.repeats, args.warmup)
        _, flags, _ = fn()
        print(json.dumps(dict(bench="token_fare_pgd", loop=name, ms_median=med, ms_min=lo, ms_max=hi,
                              images_per_s=B * 1e3 / med, flags=int(flags), **common)), flush=True)

    S, W = eng.n_tokens, cfg.width
    rows = (B * S + 255) // 256 * 256
    t = torch.randn(B, S, W, device=dev)
    ref = (t[:, 1:] + 0.1 * torch.randn(B, S - 1, W, device=dev)).contiguous()
    s32 = torch.empty(rows, W, device=dev)
    s16 = torch.empty(rows, W, device=dev, dtype=torch.bfloat16)
    per = torch.empty(B, device=dev)
    scalar = torch.empty(1, device=dev)
    scratch = torch.empty(B * ((S + 7) // 8), device=dev)
    for form, a32, a16, wbytes in (("bf16", None, s16, 2), ("fp32", s32, None, 4), ("fp32+bf16", s32, s16, 6)):
        fn = lambda: L.check(lib.rvlm_tokens_l2_loss_grad(  # noqa: E731
            t.data_ptr(), ref.data_ptr(), B, S, W, L.TOKENS_PATCH, L.RED_MEAN, L.ptr(a32), L.ptr(a16), rows, per.data_ptr(),
            scalar.data_ptr(), scratch.data_ptr(), None, L.stream_ptr()))
        med, lo, hi = timed(fn, args.iters, args.warmup)
        nbytes = B * (S - 1) * W * 8 + rows * W * wbytes
        print(json.dumps(dict(bench="tokens_l2_loss_grad", seed=form, shape=[B, S, W], us_median=med * 1e3, us_min=lo * 1e3,
                              us_max=hi * 1e3, bytes=nbytes, gb_per_s=nbytes / (med * 1e-3) / 1e9)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
