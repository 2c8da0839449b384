#!/usr/bin/env python3
"""bench_square_l2.py - what one query of the L2 Square Attack costs on the device.

  * rvlm_square_l2_propose at [128, 3, 224, 224], s = 45 and s = 3: microseconds per call (median of 20 calls after warm-up, HIP
    events), next to the same query written with the reference's tensor expressions (autoattack/square.py:339-379) on device
    tensors in the same process, and GB/s against the least traffic a query needs: one read of x and of x_best, one write of x_new.
    The script fails if the kernel is slower than the tensor expressions.
  * a full SquareAttack(norm='L2') run on ViT-L/14 bf16 + a 1000-class head at B = 128: ms per query, split into the model forward
    (HIP events around every predict call) and everything else (host clock around the run, which ends in a synchronise).

Usage: python scripts/bench_square_l2.py [--batch 128] [--queries 40] [--no-model]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import robustvlm_amd as R  # noqa: E402
from robustvlm_amd import _lib as L  # noqa: E402


def tensor_query(x, x_best, idx, c, vh, vw, vh2, vw2, s, eps, eta, sign):
    """One query with whole-tensor fp32 operations, the way the reference spells it."""
    xc, d = x[idx], x_best[idx] - x[idx]
    m1 = torch.zeros_like(xc)
    m1[:, :, vh:vh + s, vw:vw + s] = 1.0
    nw1 = (d[:, :, vh:vh + s, vw:vw + s] ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    m2 = torch.zeros_like(xc)
    m2[:, :, vh2:vh2 + s, vw2:vw2 + s] = 1.
    nimg = ((x_best[idx] - xc) ** 2).view(xc.shape[0], -1).sum(-1).sqrt().view(-1, 1, 1, 1)
    nws = ((d * torch.max(m1, m2)) ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    new = torch.ones([xc.shape[0], c, s, s], device=x.device)
    new *= eta.view(1, 1, s, s) * sign.view(-1, c, 1, 1)
    new += d[:, :, vh:vh + s, vw:vw + s] / (1e-12 + nw1)
    new = new / (1e-12 + (new ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()) * (
        torch.max((eps * torch.ones_like(new)) ** 2 - nimg ** 2, torch.zeros_like(new)) / c + nws ** 2).sqrt()
    d[:, :, vh2:vh2 + s, vw2:vw2 + s] = 0.
    d[:, :, vh:vh + s, vw:vw + s] = new + 0
    t = (d ** 2).view(d.shape[0], -1).sum(-1).sqrt()
    return torch.clamp(xc + d / (t.view(-1, 1, 1, 1) + 1e-12) * eps, 0., 1.)


def median_us(fn, calls=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--queries", type=int, default=40)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_square_l2.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    B, c, h, w, eps = args.batch, 3, 224, 224, 3.0
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, c, h, w, generator=g).to(dev)
    t = torch.randn(B, c, h, w, generator=g).to(dev)
    x_best = torch.clamp(x + 0.9 * eps * t / t.flatten(1).norm(dim=1).view(-1, 1, 1, 1), 0., 1.).contiguous()
    idx = torch.arange(B, device=dev)
    x_new = torch.empty_like(x)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    least = 3 * x.numel() * 4
    slower = False
    for s, (vh, vw, vh2, vw2) in ((45, (20, 100, 150, 60)), (3, (7, 9, 200, 118))):
        eta = R.square.eta_window(s).contiguous().to(dev)
        sign = torch.sign(2 * torch.rand(B, c, generator=g) - 1).to(dev)

        def kernel():
            L.check(lib.rvlm_square_l2_propose(x.data_ptr(), x_best.data_ptr(), idx.data_ptr(), B, c, h, w, vh, vw, vh2, vw2, s, eps,
                                               eta.data_ptr(), sign.data_ptr(), x_new.data_ptr(), flags.data_ptr(), L.stream_ptr()))

        def tensors():
            return tensor_query(x, x_best, idx, c, vh, vw, vh2, vw2, s, eps, eta, sign)
        k_med, k_min, k_max = median_us(kernel)
        t_med, t_min, t_max = median_us(tensors)
        diff = float((x_new - tensors()).abs().max())
        print(f"[{B}, {c}, {h}, {w}] s={s}: rvlm_square_l2_propose {k_med:.1f} us (min {k_min:.1f}, max {k_max:.1f}) = "
              f"{least / k_med / 1e3:.0f} GB/s of the least traffic ({least / 1e6:.0f} MB); tensor expressions {t_med:.1f} us "
              f"(min {t_min:.1f}, max {t_max:.1f}); ratio {t_med / k_med:.1f}x; max |kernel - tensors| {diff:.2e}")
        slower = slower or k_med > t_med
    assert int(flags.item()) == 0
    if not args.no_model:
        cfg = R.CONFIGS["ViT-L-14"]
        from oracle import vit_ref as V
        wts = V.init_weights(V.VIT_L_14, seed=3)
        eng = R.VitEngine(cfg, {k: v.to(dev) for k, v in wts.items()}, precision="bf16", max_batch=B)
        T = torch.randn(cfg.out_dim, 1000, generator=g).to(dev)
        clf = R.ClassificationModel(eng, T / T.norm(dim=0, keepdim=True)).eval()
        spans = []

        def predict(v):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = clf(v)
            b.record()
            spans.append((a, b, v.shape[0]))
            return out
        with torch.no_grad():
            y = clf(x).max(1)[1]
        atk = R.SquareAttack(predict, norm="L2", n_queries=args.queries, eps=eps, p_init=.8, n_restarts=1, seed=0, resc_schedule=False)
        atk.init_hyperparam(x)
        for timed in (False, True):                                      # the first run warms every shape up
            spans.clear()
            torch.random.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            used, _ = atk.attack_single_run(x, y)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        fwd = sum(a.elapsed_time(b) for a, b, _ in spans)
        n = len(spans)
        print(f"SquareAttack L2 on ViT-L/14 bf16 + 1000-class head, B={B}, eps={eps}: {n} model calls "
              f"(mean {sum(m for _, _, m in spans) / n:.1f} images each), {wall / n:.2f} ms per query = {fwd / n:.2f} ms model forward + "
              f"{(wall - fwd) / n:.2f} ms everything else (draws, eta / sign upload, propose, accept, bookkeeping, the host sync)")
        eng.close()
    if slower:
        raise SystemExit("rvlm_square_l2_propose is slower than the tensor expressions")


if __name__ == "__main__":
    main()
