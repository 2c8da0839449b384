#!/usr/bin/env python
"""Cost of the FAB kernels next to the model work of a FAB-T iteration, and the projection alone.

ViT-L/14 bf16, B images, seeded weights, 1 000-class random unit-norm head.
(i)  One FAB-T iteration = forward + input-gradient backward (rvlm_vit_fwd_inputgrad, RVLM_LOSS_LOGIT_DIFF), rvlm_fab_linf_step,
     prediction forward + head + arg-max, rvlm_fab_track_best.  Each part is timed by HIP events around it over --iters
     iterations after --warmup; reported: median ms per part, the FAB kernels' share (target <= 5 %), images / s of a
     100-iteration run with one target class.
(ii) rvlm_fab_projection_linf alone at R = 2 B rows, D = 150 528: median us and bytes moved / us against the algorithmic minimum
     (one read of w, t and one write of d per row; the kernel walks a row 10 times - walks after the first are cache hits).
One process, one GPU; one JSON line per part.

    python scripts/bench_fab.py [--batch 128] [--iters 20] [--warmup 3]
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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    cfg = R.CONFIGS[args.model]
    B = args.batch
    eng = R.VitEngine(cfg, R.random_state_dict(cfg, seed=0, device=dev), precision="bf16", max_batch=B)
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g).to(dev)
    T = torch.nn.functional.normalize(torch.randn(cfg.out_dim, args.classes, generator=g), dim=0).to(dev).contiguous()
    clf = R.ClassificationModel(eng, T).eval()
    with torch.no_grad():
        top = clf(x0).topk(2, dim=1)[1]
    y, yt = top[:, 0].contiguous(), top[:, 1].contiguous()
    n = x0[0].numel()
    x1 = (x0 + (torch.rand(x0.shape, generator=g).to(dev) - .5) * (4 / 255)).clamp(0, 1).contiguous()
    df, dg = torch.empty(B, device=dev), torch.empty_like(x1)
    adv, res2 = x0.clone(), torch.full([B], 1e10, device=dev)
    eq = torch.empty(B, dtype=torch.uint8, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    ls = eng._loss_spec("logit-diff", "none", True, T, y, 100.0, y_target=yt, B=B)
    st = L.stream_ptr

    def model_grad():
        L.check(lib.rvlm_vit_fwd_inputgrad(eng._h, x1.data_ptr(), None, B, C.byref(ls), None, df.data_ptr(), None, dg.data_ptr(), st()))

    def fab_step():
        L.check(lib.rvlm_fab_linf_step(x1.data_ptr(), x0.data_ptr(), dg.data_ptr(), df.data_ptr(), B, n, 0.1, 1.05, None,
                                       flags.data_ptr(), st()))

    def model_pred():
        with torch.no_grad():
            z = clf(x1)
        L.check(lib.rvlm_argmax_eq(z.data_ptr(), y.data_ptr(), B, z.shape[1], eq.data_ptr(), st()))

    def fab_track():
        L.check(lib.rvlm_fab_track_best(x1.data_ptr(), x0.data_ptr(), adv.data_ptr(), res2.data_ptr(), eq.data_ptr(), 0.9, B, n, st()))

    parts = {"model_fwd_inputgrad": model_grad, "fab_linf_step": fab_step, "model_prediction": model_pred, "fab_track_best": fab_track}
    # interleaved like the attack (each part sees the state the previous one left), every part under its own events
    samples = {k: [] for k in parts}
    for it in range(args.warmup + args.iters):
        for k, fn in parts.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            if it >= args.warmup:
                samples[k].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in samples.items()}
    fab_ms = med["fab_linf_step"] + med["fab_track_best"]
    total = sum(med.values())
    print(json.dumps(dict(bench="fab_t_iteration", model=args.model, precision="bf16", batch=B, classes=args.classes,
                          iters=args.iters, ms_median=med, ms_min={k: min(v) for k, v in samples.items()},
                          ms_max={k: max(v) for k, v in samples.items()}, ms_iteration=total, fab_kernel_ms=fab_ms,
                          fab_share=fab_ms / total, target_share=0.05, nonfinite_flag=int(flags.item()),
                          device=torch.cuda.get_device_name(dev))), flush=True)
    # the attack itself: 100 iterations, one target class
    atk = R.FABAttack(clf, norm="Linf", n_iter=100, eps=4 / 255, seed=0, targeted=True, n_target_classes=1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = atk.perturb(x0.clone(), y.clone())
    b.record(); b.synchronize()
    sec = a.elapsed_time(b) / 1e3
    dist = (out - x0).abs().reshape(B, -1).max(1)[0]
    print(json.dumps(dict(bench="fab_t_perturb", n_iter=100, n_target_classes=1, batch=B, seconds=sec, images_per_s=B / sec,
                          fooled_within_eps=int((dist > 0).sum()))), flush=True)
    # (ii) the projection alone
    Rr = 2 * B
    t = torch.rand(Rr, n, generator=g).to(dev)
    w = torch.randn(Rr, n, generator=g).to(dev)
    bb = ((w * t).sum(1) + 0.05 * w.abs().sum(1)).contiguous()
    d, lam = torch.empty_like(t), torch.empty(Rr, device=dev)

    def proj():
        L.check(lib.rvlm_fab_projection_linf(t.data_ptr(), w.data_ptr(), bb.data_ptr(), Rr, n, d.data_ptr(), lam.data_ptr(),
                                             flags.data_ptr(), st()))
    m, lo, hi = timed(proj, args.iters, args.warmup)
    min_bytes = 3.0 * Rr * n * 4
    print(json.dumps(dict(bench="fab_projection_linf", rows=Rr, D=n, us_median=m * 1e3, us_min=lo * 1e3, us_max=hi * 1e3,
                          algorithmic_min_bytes=min_bytes, min_bytes_per_us=min_bytes / (m * 1e3),
                          walked_bytes_per_us=(2 * 9 + 3) * Rr * n * 4 / (m * 1e3))), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
