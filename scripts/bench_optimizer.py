#!/usr/bin/env python
"""The two optimizer kernels alone, at the size of a real step: rvlm_sgd_step and rvlm_adamw_step over n = FlatParams(model).numel
fp32 elements (304 M for ViT-L/14), seeded random parameters / gradients / state.

Both are pure HBM streams with the same access pattern; per element SGD with momentum moves 20 B (reads p, g, buf; writes p, buf),
AdamW 28 B (reads p, g, m, v; writes p, m, v).  The yardstick for the SGD kernel is the AdamW kernel of the same run: less
arithmetic on the same pattern, so its byte rate should be no lower.  The SGD kernel is also timed through pointers offset by one
float, which takes its one-float-at-a-time path (what the 16-byte accesses buy).

Timed by HIP events around each call, the three kernels interleaved, median of --iters after --warmup; one JSON line per kernel
with ms and achieved bytes / s.  One process, one GPU.

    python scripts/bench_optimizer.py [--model ViT-L-14] [--iters 20] [--warmup 3]
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
from robustvlm_amd.trainer import FlatParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    n = FlatParams(R.CONFIGS[args.model], None, dev).numel
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n + 4, generator=g, device=dev) * 0.02
    grad = torch.randn(n + 4, generator=g, device=dev) * 1e-3
    buf, m, v = torch.zeros_like(p), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    lr, wd, st = 1e-5, 1e-4, L.stream_ptr
    step = [0]

    def sgd(off=0):
        L.check(lib.rvlm_sgd_step(p[off:].data_ptr(), grad[off:].data_ptr(), buf[off:].data_ptr(), n, lr, 0.9, wd, 0, 1.0, st()),
                "rvlm_sgd_step")

    def adamw():
        step[0] += 1
        L.check(lib.rvlm_adamw_step(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999, 1e-8, wd, step[0],
                                    1.0, st()), "rvlm_adamw_step")

    parts = {"rvlm_sgd_step": (sgd, 20), "rvlm_adamw_step": (adamw, 28), "rvlm_sgd_step_unaligned": (lambda: sgd(1), 20)}
    samples = {k: [] for k in parts}
    for it in range(args.warmup + args.iters):
        for k, (fn, _) in parts.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            if it >= args.warmup:
                samples[k].append(a.elapsed_time(b))
    assert bool(torch.isfinite(p).all())
    for k, (_, bytes_per_elem) in parts.items():
        ms = statistics.median(samples[k])
        print(json.dumps(dict(bench=k, model=args.model, n=n, iters=args.iters, ms_median=round(ms, 4), ms_min=round(min(samples[k]), 4),
                              ms_max=round(max(samples[k]), 4), bytes_per_element=bytes_per_elem,
                              bytes_per_s=round(bytes_per_elem * n / (ms * 1e-3), 1),
                              device=torch.cuda.get_device_name(dev))), flush=True)


if __name__ == "__main__":
    main()
