"""Worker of tests/test_gpu_token_training.py::test_token_bucketed_allreduce_on_rccl_single_rank: the loss="l2-tokens" step of the
trainer with its bucketed, asynchronous gradient all-reduce over the REACHED stages, in a one-rank group on the real RCCL backend
(the group is set up as tests/rccl_worker.py does).  With one rank the reduction is the identity, so one step must leave the
parameters the non-reducing trainer leaves, bit for bit."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import robustvlm_amd as R                                   # noqa: E402
from robustvlm_amd.trainer import AdversarialTrainer         # noqa: E402
from oracle import vit_ref as V                              # noqa: E402  (weights / config only: test infrastructure)


def main(out):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    c = V.VIT_TINY2
    cfg = R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)
    w = {k: v.to(dev) for k, v in V.init_weights(c, seed=21).items()}
    g = torch.Generator().manual_seed(7)
    x = torch.rand(4, 3, c.image_size, c.image_size, generator=g).to(dev)
    xa = (x + 0.03 * (torch.rand(x.shape, generator=g).to(dev) * 2 - 1)).clamp(0, 1)
    kw = dict(batch_size=4, precision="bf16", lr=1e-3, wd=1e-2, warmup=2, steps=10, attack="none", loss="l2-tokens",
              inner_loss="l2-tokens", token_depth=-2, token_select="patch")
    plain = AdversarialTrainer(cfg, w, **kw)
    plain.train_step(x, None, data_adv=xa)
    ref = plain.params.flat.clone()
    plain.close()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    tr = AdversarialTrainer(cfg, w, n_buckets=3, always_reduce=True, **kw)
    assert tr._device_collectives
    buckets = [list(b) for b in tr._token_buckets]
    tr.train_step(x, None, data_adv=xa)
    torch.cuda.synchronize()
    same = bool(torch.equal(tr.params.flat, ref))
    moved = not bool(torch.equal(tr.params.flat[tr._token_span_lo:], w_flat(tr, w)[tr._token_span_lo:]))
    tr.close()
    dist.destroy_process_group()
    torch.save(dict(same=same and moved, buckets=buckets), out)


def w_flat(tr, w):
    flat = torch.empty_like(tr.params.flat)
    for k, (o, n) in tr.params.offsets.items():
        flat[o:o + n] = w[k].reshape(-1)
    return flat


if __name__ == "__main__":
    main(sys.argv[1])
