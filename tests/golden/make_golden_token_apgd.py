#!/usr/bin/env python3
"""Generate tests/golden/token_apgd_tiny.npz by RUNNING the reference's ``vlm_eval.attacks.apgd.apgd`` on the CPU, one image at a
time (it asserts a batch of one), with the token l2 of a tiny seeded tower as the model.  The reference is imported at run time from
the tree named by the environment variable RVLM_REFERENCE; nothing of it is copied here, only arrays are written.

    RVLM_REFERENCE=<reference checkout> python tests/golden/make_golden_token_apgd.py

Model: oracle.vit_ref.VIT_TINY (32 px, S = 17) with init_weights(seed=9), truncated to ``depth`` blocks; the closure returns
``sum (tokens(x_adv) - tokens(x))^2`` over the selected rows, the loss rvlm_apgd_run_tokens attacks.  B = 4 seeded images and one
seeded pert_init direction u in [-1, 1] per pixel: the L-inf cases start at ``x + eps * u``, the L2 cases at ``x + 0.5 eps u /
|u|_2`` (inside the ball; tests/token_apgd_cases.py::pert_init).

Cases: {linf, l2} x {(depth 1, patch rows), (depth 2, all rows)} x n_iter in {1, 10, 25} x {small radius (4/255 | 0.5), large
radius (32/255 | 6.0)}.  At the small radii the loss never decreases (the controller halves a step only where the loss has stopped
moving); at the large ones it does, and the generator ASSERTS so for n_iter >= 10: every image's trace has a decrease and at least one image of the
batch ends with a halved step (read off the reference's own ``verbose`` print of ``step_size.mean()`` - a batch of one - in its last
iteration, before that iteration's check).

Stored per case ``<name>/``: ``x_best`` (packed), ``loss_best`` [B], ``trace`` [n_iter + 1, B] (every loss the model returned: row 0
the start point), ``step_seen`` [B] (the step size printed in the last iteration) and the last iterate as ``x_last_idx`` /
``x_last_rows`` (packed): the images whose last iterate differs from ``x_best`` (for the others ``x_last == x_best`` bit for bit).
Shared: ``x``, ``u``, the weights seed.  The packing is lossless (tests/token_apgd_cases.py, which also reads the file for the
tests) and keeps the file under the size limit for a committed file.
"""
import contextlib
import dataclasses
import hashlib
import io
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("RVLM_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "vlm_eval", "attacks")):
    sys.exit("set RVLM_REFERENCE to a checkout of the reference (it must hold vlm_eval/attacks/)")
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "token_apgd_tiny.npz")

from vlm_eval.attacks.apgd import apgd as ref_apgd  # noqa: E402
from oracle import vit_ref as V  # noqa: E402
from tests import token_apgd_cases as TC  # noqa: E402

CFG, SEED, B = V.VIT_TINY, 9, 4
# images and pert_init direction.  Seeds 8 and 9 were tried first: each left an image of linf_large_d1patch_n10 whose loss never
# decreased, which the asserts below refuse; 10 is the first at which the reference satisfies them in every case.
DATA_SEED = int(os.environ.get("RVLM_TOKEN_APGD_DATA_SEED", "10"))
RADII = {"linf": {"small": 4 / 255, "large": 32 / 255}, "l2": {"small": 0.5, "large": 6.0}}
SHAPES = (("d1patch", 1, "patch"), ("d2all", 2, "all"))
N_ITERS = (1, 10, 25)


def tokens(w, x, depth, select):
    _, t = V.vit_forward(dataclasses.replace(CFG, layers=depth), w, V.normalize_pixels(x), return_tokens=True)
    return t[:, 1:] if select == "patch" else t


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    w = V.init_weights(CFG, seed=SEED)
    gen = torch.Generator().manual_seed(DATA_SEED)
    # 8-bit images, as a data loader hands them over (k / 255); it also keeps the file small: the L-inf iterates end mostly on x +- eps
    x = torch.randint(0, 256, (B, 3, CFG.image_size, CFG.image_size), generator=gen).float() / 255
    u = torch.rand(x.shape, generator=gen) * 2 - 1
    out, cases = {"x": x.numpy(), "u": u.numpy(), "weights_seed": np.int64(SEED)}, []
    for norm in ("linf", "l2"):
        for radius, eps in RADII[norm].items():
            p0 = torch.from_numpy(TC.pert_init(norm, eps, u.numpy()))
            pe = eps if norm == "linf" else 0.0
            for tag, depth, select in SHAPES:
                with torch.no_grad():
                    ref = tokens(w, x, depth, select)
                for n_iter in N_ITERS:
                    name = f"{norm}_{radius}_{tag}_n{n_iter}"
                    xb, lb, xl, tr, st = [], [], [], [], []
                    for b in range(B):
                        losses = []

                        def model(xa, b=b):
                            loss = ((tokens(w, xa, depth, select) - ref[b:b + 1]) ** 2).sum(dim=(1, 2))
                            losses.append(float(loss.detach()[0]))
                            return loss
                        buf = io.StringIO()
                        with contextlib.redirect_stdout(buf):
                            x_best, loss_best, x_best_adv = ref_apgd(model, x[b:b + 1].clone(), norm=norm, eps=eps, n_iter=n_iter,
                                                                     pert_init=p0[b:b + 1].clone(), verbose=True)
                        steps = [float(s) for s in re.findall(r"step size: ([0-9.]+)", buf.getvalue())]
                        assert len(losses) == n_iter + 1 and steps
                        xb.append(x_best.detach()); lb.append(loss_best.detach()); xl.append(x_best_adv.detach())
                        tr.append(np.array(losses, np.float32)); st.append(steps[-1])
                    xb, xl, lb = torch.cat(xb).numpy(), torch.cat(xl).numpy(), torch.cat(lb).numpy()
                    tr, st = np.stack(tr, axis=1), np.array(st, np.float32)
                    assert np.array_equal(lb, tr.max(axis=0))
                    decreases = (tr[1:] < tr[:-1]).sum(axis=0)
                    if radius == "large" and n_iter >= 10:
                        assert (decreases >= 1).all(), (name, decreases)
                        assert (st < 0.75 * 2 * eps).any(), (name, st)          # a halved step: at most half of alpha * eps
                    diff = [b for b in range(B) if not np.array_equal(xb[b], xl[b])]
                    out[name + "/x_best_sign"], out[name + "/x_best"] = TC.pack(xb, x.numpy(), pe)
                    assert np.array_equal(TC.unpack(out[name + "/x_best_sign"], out[name + "/x_best"], x.numpy(), pe).view(np.uint32),
                                          xb.view(np.uint32))
                    out[name + "/loss_best"], out[name + "/trace"] = lb, tr
                    out[name + "/step_seen"] = st
                    out[name + "/x_last_idx"] = np.array(diff, np.int64)
                    out[name + "/x_last_sign"], out[name + "/x_last_rows"] = TC.pack(xl[diff], x.numpy()[diff], pe)
                    cases.append(dict(name=name, norm=norm, radius=radius, eps=eps, depth=depth, select=select, n_iter=n_iter,
                                      decreases=decreases.tolist(), halved=bool((st < 0.75 * 2 * eps).any())))
                    print(name, "decreases", decreases.tolist(), "step/step0", (st / (2 * eps)).round(3).tolist(),
                          "best != last", diff, file=sys.stderr)
    h = hashlib.sha256()
    with open(os.path.join(REF, "vlm_eval", "attacks", "apgd.py"), "rb") as f:
        h.update(f.read())
    out["reference_sha256"] = np.array(h.hexdigest())
    out["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
