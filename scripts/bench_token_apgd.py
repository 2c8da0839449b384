#!/usr/bin/env python
"""Time of the batched token APGD loop (rvlm_apgd_run_tokens) next to the same loop driven from Python and to the token PGD loop.

ViT-L/14 bf16, seeded weights, B random 224 x 224 images, depth = layers - 1, patch rows (LLaVA's tower), L-inf 4/255 from a random
start inside the ball, median of --repeats calls (HIP events):
(i)   the fused loop, VitEngine.apgd_run_tokens, at every n_iter of --n-iter (default 10 and 50);
(ii)  (a) the same loop from Python over the public entries - tokens_fwd_inputgrad + rvlm_apgd_linf_step + rvlm_apgd_controller_rho
      + rvlm_apgd_select, the host's schedule, no read-back inside the loop - at the same n_iter;
(iii) (b) pgd_run_tokens at 10 steps: its per-iteration cost c is one forward + one backward (+ the update), so the fused APGD loop is
      expected at about (n_iter + 1) forwards + n_iter backwards = (n_iter + 1 / 2 or so) c; printed as `expected_ms` with the
      forward share of c measured by a non-saving token forward.
One process, one GPU; one JSON line per measurement.

    python scripts/bench_token_apgd.py [--batch 128] [--n-iter 10 50] [--repeats 5]
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


def schedule(n_iter):
    k = max(int(0.22 * n_iter), 1)
    n_iter_min, size_decr = max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1)
    counter3, out = 0, []
    for _ in range(n_iter):
        counter3 += 1
        do_check = int(counter3 == k)
        out.append((k, do_check))
        if do_check:
            counter3, k = 0, max(k - size_decr, n_iter_min)
    return out


def python_loop(eng, lib, x, x_init, ref, depth, eps, n_iter, step0):
    """apgd() on the token loss over the public entries; returns (x_best, loss_best)."""
    B, npix = x.shape[0], x[0].numel()
    x_adv = x_init.clamp(0., 1.)
    x_best, x_best_adv, x_old = x_adv.clone(), x_adv.clone(), x_adv.clone()
    f32, u8 = dict(dtype=torch.float32, device=x.device), dict(dtype=torch.uint8, device=x.device)
    loss_steps = torch.zeros(n_iter, B, **f32)
    _, per, _, grad = eng.tokens_fwd_inputgrad(x_adv, None, ref, depth=depth, select="patch", reduction="none")
    grad_best, loss_best, lbc = grad.clone(), per.clone(), per.clone()
    reduced, step = torch.ones(B, **f32), torch.full((B,), step0, **f32)
    pred, acc, f0, f1, f2 = (torch.zeros(B, **u8) for _ in range(5))
    for i, (k, do_check) in enumerate(schedule(n_iter)):
        L.check(lib.rvlm_apgd_linf_step(x.data_ptr(), x_adv.data_ptr(), x_old.data_ptr(), grad.data_ptr(), step.data_ptr(),
                                        0.75 if i > 0 else 1.0, eps, npix, B, L.stream_ptr()))
        if i < n_iter - 1:
            _, per, _, grad = eng.tokens_fwd_inputgrad(x_adv, None, ref, depth=depth, select="patch", reduction="none")
        else:       # the last iteration runs no backward (apgd.py:300-304)
            per = torch.empty(B, **f32)
            L.check(lib.rvlm_vit_tokens_fwd_inputgrad(eng._h, x_adv.data_ptr(), None, B, depth, 0, L.TOKENS_PATCH, ref.data_ptr(),
                                                      L.RED_NONE, None, per.data_ptr(), None, None, L.stream_ptr()))
        L.check(lib.rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, 0.75, per.data_ptr(), pred.data_ptr(), loss_steps.data_ptr(),
                                             loss_best.data_ptr(), lbc.data_ptr(), reduced.data_ptr(), step.data_ptr(),
                                             acc.data_ptr(), f0.data_ptr(), f1.data_ptr(), f2.data_ptr(), L.stream_ptr()))
        L.check(lib.rvlm_apgd_select(x_adv.data_ptr(), grad.data_ptr(), x_best.data_ptr(), grad_best.data_ptr(),
                                     x_best_adv.data_ptr(), f0.data_ptr(), f1.data_ptr(), f2.data_ptr(), npix, B, L.stream_ptr()))
    return x_best, loss_best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-L-14")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--n-iter", type=int, nargs="+", default=[10, 50])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
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
    x_init = (x + d0).contiguous()
    depth = cfg.layers - 1
    ref = eng.forward_tokens(x, depth=depth)[:, 1:].contiguous()
    common = dict(bench="token_apgd", model=args.model, precision="bf16", batch=B, depth=depth, select="patch",
                  device=torch.cuda.get_device_name(dev))

    def line(**kw):
        print(json.dumps(dict(common, **kw)), flush=True)

    med, lo, hi = timed(lambda: eng.pgd_run_tokens(x, d0, ref, eps, 10, eps / 4, 0.9, "max", depth=depth, select="patch"),
                        args.repeats, args.warmup)
    c_iter = med / 10
    line(loop="pgd_run_tokens", n_iter=10, ms_median=med, ms_min=lo, ms_max=hi, ms_per_iteration=c_iter)
    fmed, flo, fhi = timed(lambda: eng.forward_tokens(x_init, depth=depth, save=True), args.repeats, args.warmup)
    line(loop="forward_tokens(save)", ms_median=fmed, ms_min=flo, ms_max=fhi)
    for n_iter in args.n_iter:
        expected = (n_iter + 1) * fmed + n_iter * (c_iter - fmed)
        med, lo, hi = timed(lambda: eng.apgd_run_tokens(x, x_init, ref, eps, n_iter, 2 * eps, depth=depth, select="patch"),
                            args.repeats, args.warmup)
        flags = int(eng.apgd_run_tokens(x, x_init, ref, eps, n_iter, 2 * eps, depth=depth, select="patch")[3].item())
        line(loop="apgd_run_tokens (fused)", n_iter=n_iter, ms_median=med, ms_min=lo, ms_max=hi, expected_ms=expected,
             of_expected=med / expected, images_per_s=B * 1e3 / med, flags=flags)
        pmed, plo, phi = timed(lambda: python_loop(eng, lib, x, x_init, ref, depth, eps, n_iter, 2 * eps), args.repeats, args.warmup)
        line(loop="python loop over the public entries", n_iter=n_iter, ms_median=pmed, ms_min=plo, ms_max=phi,
             fused_over_python=med / pmed)
    eng.close()


if __name__ == "__main__":
    main()
