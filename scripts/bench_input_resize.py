#!/usr/bin/env python
"""Cost of attacking at the dataset's own resolution: the bicubic resizer inside the engine against the generic route.

ViT-L/14 bf16, seeded weights, B random 32 x 32 images (CIFAR's geometry), 10-class random unit-norm head, APGDAttack (CE,
L-inf 4/255, 100 steps, one restart) through ClassificationModel:
(i)   resizer=BicubicResize(224): the device loop at 32 x 32 (rvlm_apgd_run after rvlm_vit_set_input_size) - "fused";
(ii)  the same resizer behind a plain callable: one autograd graph per iteration through the standalone kernels - "generic";
(iii) the images resized once to 224 x 224 and attacked there with no resizer (BASELINE config 5's shape) - "native224".
(iv)  the two fused patch-embedding kernels alone (HIP events, median of --iters calls) next to their 224 x 224 twins.
One process, one GPU; one JSON line per part.

    python scripts/bench_input_resize.py [--batch 256] [--steps 100] [--size 32] [--iters 20]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--routes", default="fused,generic,native224")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    cfg = R.CONFIGS[args.model]
    B, img, P = args.batch, cfg.image_size, cfg.patch
    eng = R.VitEngine(cfg, R.random_state_dict(cfg, seed=0, device=dev), precision="bf16", max_batch=B)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, args.size, args.size, generator=g).to(dev)
    T = torch.nn.functional.normalize(torch.randn(cfg.out_dim, args.classes, generator=g), dim=0).to(dev).contiguous()
    rs = R.BicubicResize(img)
    models = {"fused": (R.ClassificationModel(eng, T, resizer=rs).eval(), x),
              "generic": (R.ClassificationModel(eng, T, resizer=lambda v: rs(v)).eval(), x),
              "native224": (R.ClassificationModel(eng, T).eval(), rs(x).clamp(0, 1).contiguous())}
    eps = 4 / 255
    for name in args.routes.split(","):
        clf, xin = models[name]
        with torch.no_grad():
            y = clf(xin).max(1)[1]
        R.APGDAttack(clf, n_iter=3, norm="Linf", n_restarts=1, eps=eps, seed=0, loss="ce").perturb(xin.clone(), y.clone())   # warm-up
        atk = R.APGDAttack(clf, n_iter=args.steps, norm="Linf", n_restarts=1, eps=eps, seed=0, loss="ce")
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        adv = atk.perturb(xin.clone(), y.clone())
        b.record()
        b.synchronize()
        sec = a.elapsed_time(b) / 1e3
        with torch.no_grad():
            robust = float((clf(adv).max(1)[1] == y).float().mean())
        print(json.dumps(dict(bench="apgd_ce_input_resize", route=name, model=args.model, precision="bf16", batch=B,
                              input=list(xin.shape[-2:]), steps=args.steps, seconds=sec, images_per_s=B / sec,
                              linf=float((adv - xin).abs().max()), robust_fraction=robust,
                              device=torch.cuda.get_device_name(dev))), flush=True)

    # (iv) the patch-embedding kernels alone
    K = 3 * P * P
    Kpad = (K + 63) // 64 * 64
    rows = B * (img // P) ** 2
    mean, std = (C.c_float * 3)(*R.CLIP_MEAN), (C.c_float * 3)(*R.CLIP_STD)
    big = rs(x).contiguous()
    a0 = torch.empty(rows, Kpad, dtype=torch.bfloat16, device=dev)
    da0 = torch.randn(rows, Kpad, device=dev)
    g_small, g_big = torch.empty_like(x), torch.empty_like(big)
    st = L.stream_ptr
    s = args.size
    parts = {
        "resize_im2col_normalize": lambda: L.check(lib.rvlm_k_resize_im2col_normalize(
            x.data_ptr(), None, B, s, s, img, P, mean, std, a0.data_ptr(), Kpad, Kpad, 1, st())),
        "im2col_normalize_224": lambda: L.check(lib.rvlm_k_im2col_normalize(
            big.data_ptr(), None, B, img, P, mean, std, a0.data_ptr(), Kpad, Kpad, 1, st())),
        "col2im_resize_grad": lambda: L.check(lib.rvlm_k_col2im_resize_grad(
            da0.data_ptr(), Kpad, 0, B, s, s, img, P, std, g_small.data_ptr(), st())),
        "col2im_grad_224": lambda: L.check(lib.rvlm_k_col2im_grad(da0.data_ptr(), Kpad, 0, B, img, P, std, g_big.data_ptr(), st())),
        "resize_bicubic": lambda: L.check(lib.rvlm_resize_bicubic(x.data_ptr(), B * 3, s, s, img, img, big.data_ptr(), st())),
        "resize_bicubic_adjoint": lambda: L.check(lib.rvlm_resize_bicubic_adjoint(
            g_big.data_ptr(), B * 3, s, s, img, img, g_small.data_ptr(), st())),
    }
    for name, fn in parts.items():
        med, lo, hi = timed(fn, args.iters, args.warmup)
        print(json.dumps(dict(bench="input_resize_kernel", kernel=name, batch=B, input=[s, s], output=[img, img],
                              us_median=med * 1e3, us_min=lo * 1e3, us_max=hi * 1e3)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
