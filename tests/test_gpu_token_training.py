"""Token-level FARE fine-tuning (RVLM_HAS_TOKEN_TRAINING): weight gradients through the token door against torch autograd of the
oracle (oracle/vit_ref.py cut to `depth` blocks), the stage / saved-mode rules, rvlm_tokens_cosine against fp64, and the trainer's
loss="l2-tokens" step against a torch restatement written here."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.trainer import AdversarialTrainer, FlatParams, cosine_lr_value
from oracle import vit_ref as V
from tests.gpu_helpers import dev, cos_sim, rel_max, lib, st

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

# width 1024 / 65 tokens: B = 8 -> 520 rows, the split-K weight-gradient path; B = 3 -> 195 rows, the transposing fallback
VIT_WIDE = V.VitConfig(64, 8, 1024, 2, 16, 64)
CASES = {"tiny": (V.VIT_TINY, 4), "tiny2": (V.VIT_TINY2, 3), "wide520": (VIT_WIDE, 8), "wide195": (VIT_WIDE, 3)}


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


def make_engine(cfg, w, precision, max_batch, **kw):
    return R.VitEngine(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch, **kw)


def oracle_tokens(cfg, w, x, depth, ln_post=False):
    emb, t = V.vit_forward(dataclasses.replace(cfg, layers=depth), w, V.normalize_pixels(x), return_tokens=True)
    if ln_post:
        t = F.layer_norm(t, (cfg.width,), w["ln_post.weight"], w["ln_post.bias"], 1e-5)
    return t, emb


@functools.lru_cache(maxsize=None)
def problem(name):
    cfg, B = CASES[name]
    g = torch.Generator().manual_seed(2)
    w = V.init_weights(cfg, seed=11)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g)
    cot_t = torch.randn(B, cfg.tokens, cfg.width, generator=g)
    cot_e = torch.randn(B, cfg.out_dim, generator=g)
    return cfg, B, w, x, cot_t, cot_e


@functools.lru_cache(maxsize=None)
def autograd_grads(name, depth, ln_post, with_emb):
    """{key: gradient or None} of <cot_t, tokens> (+ <cot_e, emb>) by torch autograd; computed once, shared by both precisions."""
    cfg, B, w, x, cot_t, cot_e = problem(name)
    wr = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    t, emb = oracle_tokens(cfg, wr, x, depth, ln_post)
    loss = (t * cot_t).sum()
    if with_emb:
        loss = loss + (emb * cot_e).sum()
    loss.backward()
    return {k: (None if v.grad is None else v.grad.detach()) for k, v in wr.items()}


def grad_cases():
    out = []
    for name, (cfg, _) in CASES.items():
        Lr = cfg.layers
        for depth in sorted({1, Lr - 1, Lr}):
            for ln_post in (0, 1):
                for with_emb in ((0, 1) if depth == Lr else (0,)):
                    out.append(pytest.param(name, depth, ln_post, with_emb, id=f"{name}-d{depth}-ln{ln_post}-emb{with_emb}"))
    return out


def check_grad(k, got, ref, precision, scale=1.0):
    if precision == "fp32":
        r = rel_max(got, scale * ref)
        assert r < 2e-3, f"{k}: rel {r}"
    else:
        c = cos_sim(got, scale * ref)
        assert c > 0.97, f"{k}: cos {c}"


# ---- 1. gradients vs autograd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name,depth,ln_post,with_emb", grad_cases())
def test_token_weight_gradients_vs_autograd(name, depth, ln_post, with_emb, precision):
    cfg, B, w, x, cot_t, cot_e = problem(name)
    ref = autograd_grads(name, depth, ln_post, with_emb)
    unreached = [k for k, v in ref.items() if v is None]
    assert ("proj" in unreached) == (not with_emb)
    assert ("ln_post.weight" in unreached) == (not (ln_post or with_emb))
    assert any(k.startswith(f"transformer.resblocks.{depth}.") for k in unreached) == (depth < cfg.layers)
    eng = make_engine(cfg, w, precision, B, trainable=True)
    grads = FlatParams(to_cfg(cfg), None, dev())
    grads.flat.fill_(3.0)                                          # accumulate=False overwrites: reached and unreached alike
    xd, dt = x.to(dev()), cot_t.to(dev())
    de = cot_e.to(dev()) if with_emb else None
    eng.forward_tokens(xd, depth=depth, ln_post=bool(ln_post), save=2)
    eng.backward_params_tokens(dt, grads.views, d_emb=de, accumulate=False)
    torch.cuda.synchronize()
    for k, r in ref.items():
        got = grads.views[k].cpu()
        if r is None:
            assert not got.any(), f"{k}: autograd leaves it at None, the pass must zero-fill it"
        else:
            check_grad(k, got, r, precision)
    # accumulate=True: unreached gradients are left alone, reached ones double
    for k in unreached:
        grads.views[k].fill_(7.0)
    eng.forward_tokens(xd, depth=depth, ln_post=bool(ln_post), save=2)
    eng.backward_params_tokens(dt, grads.views, d_emb=de, accumulate=True)
    torch.cuda.synchronize()
    for k, r in ref.items():
        got = grads.views[k].cpu()
        if r is None:
            assert bool((got == 7.0).all()), f"{k}: accumulate=True must not touch an unreached gradient"
        else:
            check_grad(k, got, r, precision, scale=2.0)
    eng.close()


# ---- 2. stages ---------------------------------------------------------------------------------------------------------------
def test_token_backward_stages_in_order_and_equal_to_one_call():
    cfg, B, w, x, cot_t, _ = problem("tiny2")
    depth, n_stages = cfg.layers - 1, cfg.layers + 2
    eng = make_engine(cfg, w, "fp32", B, trainable=True)
    xd, dt = x.to(dev()), cot_t.to(dev())
    one, sliced = FlatParams(to_cfg(cfg), None, dev()), FlatParams(to_cfg(cfg), None, dev())
    one.flat.fill_(5.0); sliced.flat.fill_(-5.0)
    eng.forward_tokens(xd, depth=depth, save=2)
    eng.backward_params_tokens(dt, one.views)
    eng.forward_tokens(xd, depth=depth, save=2)
    with pytest.raises(L.RvlmError, match="in order"):
        eng.backward_params_tokens(dt, sliced.views, stages=(1, 2))            # stage 0 never ran for this forward
    eng.backward_params_tokens(dt, sliced.views, stages=(0, 2))
    with pytest.raises(L.RvlmError, match="in order"):
        eng.backward_params_tokens(dt, sliced.views, stages=(1, 3))            # repeats stage 1
    with pytest.raises(L.RvlmError, match="in order"):
        eng.backward_params_tokens(dt, sliced.views, stages=(3, n_stages))     # skips stage 2
    eng.backward_params_tokens(dt, sliced.views, stages=(0, 1))                # stage 0 restarts the pass
    eng.backward_params_tokens(dt, sliced.views, stages=(1, 3))
    eng.backward_params_tokens(dt, sliced.views, stages=(3, n_stages))
    torch.cuda.synchronize()
    assert torch.equal(one.flat, sliced.flat)
    eng.close()


# ---- 3. state rules ------------------------------------------------------------------------------------------------------------
def test_saved_mode_rules():
    cfg, B, w, x, cot_t, cot_e = problem("tiny2")
    xd, dt, de = x.to(dev()), cot_t.to(dev()), cot_e.to(dev())
    tok = torch.empty(B, cfg.tokens, cfg.width, device=dev())
    plain = make_engine(cfg, w, "fp32", B)
    assert lib().rvlm_vit_forward_tokens(plain._h, xd.data_ptr(), None, B, 2, 0, 2, tok.data_ptr(), None, st()) == L.RVLM_ERR_ARG
    assert b"trainable" in lib().rvlm_last_error()
    plain.close()
    eng = make_engine(cfg, w, "fp32", B, trainable=True)
    grads = FlatParams(to_cfg(cfg), None, dev())

    def status_of_params_tokens(d_tokens, n):
        w_, keep = eng._weights_struct(grads.views, inplace=True)
        import ctypes as C
        rc = lib().rvlm_vit_backward_params_tokens(eng._h, d_tokens.data_ptr(), None, n, C.byref(w_), 0, st())
        del keep
        return rc

    eng.forward(xd, None, False, save=2)
    assert status_of_params_tokens(dt, B) == L.RVLM_ERR_STATE                   # a pooled save=2 forward
    eng.forward_tokens(xd, depth=2, save=True)
    assert status_of_params_tokens(dt, B) == L.RVLM_ERR_STATE                   # a token pass with save=1
    g1 = eng.backward_input_tokens(dt)
    eng.forward_tokens(xd, depth=2, save=2)
    assert status_of_params_tokens(dt[:2].contiguous(), 2) == L.RVLM_ERR_STATE  # another B
    with pytest.raises(L.RvlmError, match="status 3"):
        eng.backward_params(de, grads.views)                                    # the pooled parameter pass after a token save=2
    with pytest.raises(ValueError, match="depth == layers"):
        eng.backward_params_tokens(dt, grads.views, d_emb=de)                   # d_emb below full depth
    assert torch.equal(eng.backward_input_tokens(dt), g1)                       # save=2 is a superset of save=1
    eng.close()


def test_pooled_parameter_pass_is_unchanged_by_token_passes():
    cfg, B, w, x, cot_t, cot_e = problem("tiny2")
    xd, dt, de = x.to(dev()), cot_t.to(dev()), cot_e.to(dev())
    for precision in ("fp32", "bf16"):
        eng = make_engine(cfg, w, precision, B, trainable=True)
        before, after = FlatParams(to_cfg(cfg), None, dev()), FlatParams(to_cfg(cfg), None, dev())
        eng.forward(xd, None, False, save=2)
        eng.backward_params(de, before.views)
        scratch = FlatParams(to_cfg(cfg), None, dev())
        eng.forward_tokens(xd, depth=cfg.layers, ln_post=True, save=2)
        eng.backward_params_tokens(dt, scratch.views, d_emb=de)
        eng.forward(xd, None, False, save=2)
        eng.backward_params(de, after.views)
        torch.cuda.synchronize()
        assert torch.equal(before.flat, after.flat), precision
        eng.close()


# ---- 4. rvlm_tokens_cosine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,W,select", [(3, 5, 64, "all"), (2, 37, 128, "patch"), (2, 257, 1024, "patch")])
def test_tokens_cosine_vs_fp64(B, S, W, select):
    g = torch.Generator().manual_seed(S)
    first = 1 if select == "patch" else 0
    ref = torch.randn(B, S - first, W, generator=g)
    t = torch.randn(B, S, W, generator=g)
    t[:, first:] = 0.6 * ref + 0.8 * t[:, first:]               # cosines around 0.6: O(1), not the ~0 of independent rows
    t[0, first + 1] = 0.0                                       # a zero row: a.b = 0 over sqrt(max(0, 1e-16)) = 0
    t[1, first + 2] = 1e-6; ref[1, 2] = 1e-6                    # |a|^2 |b|^2 < eps^2: the clamp decides, not the norms
    td, rd = t.to(dev()), ref.to(dev())
    outs = []
    for _ in range(2):
        per = torch.empty(B, device=dev()); mean = torch.empty(1, device=dev())
        scratch = torch.empty(B * ((S + 7) // 8), device=dev())
        L.check(lib().rvlm_tokens_cosine(td.data_ptr(), rd.data_ptr(), B, S, W, L.TOKENS_PATCH if first else L.TOKENS_ALL,
                                         per.data_ptr(), mean.data_ptr(), scratch.data_ptr(), st()), "rvlm_tokens_cosine")
        torch.cuda.synchronize()
        outs.append((per.clone(), mean.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    a, b = t[:, first:].double(), ref.double()
    rows = (a * b).sum(-1) / torch.sqrt(torch.clamp((a * a).sum(-1) * (b * b).sum(-1), min=1e-16))
    assert float(rows[0, 1]) == 0.0 and 0 < float(rows[1, 2]) < 0.5
    want = rows.mean(-1)
    err = float((outs[0][0].cpu().double() - want).abs().max())
    err_mean = abs(float(outs[0][1].cpu().double()) - float(want.mean()))
    print(f"tokens_cosine {B}x{S}x{W} {select}: per-image error {err:.3e}, mean error {err_mean:.3e}")
    assert err <= 1e-6 and err_mean <= 1e-6
    # mean-less call: the optional output
    per = torch.empty(B, device=dev())
    L.check(lib().rvlm_tokens_cosine(td.data_ptr(), rd.data_ptr(), B, S, W, L.TOKENS_PATCH if first else L.TOKENS_ALL,
                                     per.data_ptr(), None, scratch.data_ptr(), st()))
    torch.cuda.synchronize()
    assert torch.equal(per, outs[0][0])


# ---- 5. trainer, fp32, vs a torch restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cw", [0.0, 0.3])
def test_token_train_step_fp32_matches_torch(cw):
    cfg = V.VIT_TINY2
    Lr, depth, W = cfg.layers, cfg.layers - 1, cfg.width
    w = V.init_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(4)
    B, lr, wd, warmup, steps = 4, 1e-3, 1e-2, 2, 10
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g)
    xa = (x + 0.02 * torch.rand(x.shape, generator=g)).clamp(0, 1)
    tr = AdversarialTrainer(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, batch_size=B, precision="fp32", lr=lr, wd=wd,
                            warmup=warmup, steps=steps, loss="l2-tokens", inner_loss="l2-tokens", loss_clean="l2-tokens",
                            attack="none", clean_weight=cw, token_depth=-2, token_select="patch")
    assert tr.token_depth == depth
    # torch side: AdamW over ALL parameters (it skips those whose grad is None), the trainer's learning-rate rule
    wr = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    opt = torch.optim.AdamW(list(wr.values()), lr=lr, weight_decay=wd)
    with torch.no_grad():
        ref0 = oracle_tokens(cfg, w, x, depth)[0][:, 1:]

    def token_loss(xx):
        t = oracle_tokens(cfg, wr, xx, depth)[0][:, 1:]
        return ((t - ref0) ** 2).sum(dim=(1, 2)).mean()
    cur_lr = lr                                                   # the first step runs at the base rate
    for it in range(3):
        out = tr.train_step(x.to(dev()), None, data_adv=xa.to(dev()))
        for grp in opt.param_groups:
            grp["lr"] = cur_lr
        opt.zero_grad(set_to_none=True)
        loss = token_loss(xa)
        loss_clean = token_loss(x) if cw > 0 else torch.zeros(())
        (cw * loss_clean + (1 - cw) * loss).backward()
        opt.step()
        assert out["lr"] == cur_lr
        cur_lr = cosine_lr_value(it + 1, lr, warmup, steps)
        for name, got, want in (("loss", out["loss"], loss), ("loss_clean", out["loss_clean"], loss_clean)):
            got, want = float(got.detach()), float(want.detach())
            assert abs(got - want) <= 2e-3 * abs(want) + 1e-7, (it, name, got, want)
        assert out["acc"] is None and out["racc"] is None
        assert -1 < float(out["cos_sim"]) <= 1 and -1 < float(out["cos_sim_clean"]) <= 1
    sd = tr.state_dict()
    osd = tr.optimizer_state_dict()
    unreached = [k for k in w if k.startswith(f"transformer.resblocks.{Lr - 1}.") or k.startswith("ln_post.") or k == "proj"]
    assert len(unreached) == 12 + 3
    for k, v in wr.items():
        got, want = sd[k].cpu(), v.detach()
        if k in unreached:
            assert v.grad is None
            assert torch.equal(got, w[k]), f"{k}: a parameter the token loss cannot reach was touched"
            st_ = osd["state"][osd["param_names"].index(k)]
            assert not st_["exp_avg"].any() and not st_["exp_avg_sq"].any(), k
            continue
        if k.endswith("attn.in_proj_bias"):      # key bias: true gradient 0, Adam turns rounding noise into +-lr steps
            got = torch.cat([got[:W], got[2 * W:]]); want = torch.cat([want[:W], want[2 * W:]])
        r = rel_max(got, want)
        assert r < 2e-2, f"{k}: {r}"
    tr.close()


# ---- 6. trainer runs and learns, bf16 ---------------------------------------------------------------------------------------------
def test_token_train_step_bf16_runs_and_learns():
    cfg = R.CONFIGS["ViT-B-32"]
    sd = R.random_state_dict(cfg, seed=0, device=dev())
    B = 8
    tr = AdversarialTrainer(cfg, sd, batch_size=B, precision="bf16", lr=2e-6, wd=1e-4, warmup=1, steps=100, loss="l2-tokens",
                            inner_loss="l2-tokens", attack="pgd", iterations_adv=2, token_depth=-2)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(B, 3, 224, 224, generator=g, device=dev())
    first = tr.train_step(x, None)                        # full path once: frozen tokens, token PGD, fwd, bwd, AdamW
    assert np.isfinite(float(first["loss"])) and float(first["loss"]) > 0
    assert -1 < float(first["cos_sim"]) <= 1 and -1 < float(first["cos_sim_clean"]) <= 1
    xa = (x + (torch.rand(x.shape, generator=g, device=dev()) * 2 - 1) * (4 / 255)).clamp(0, 1)
    losses = [float(tr.train_step(x, None, data_adv=xa)["loss"]) for _ in range(5)]   # fixed adversarial batch
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    tr.close()


# ---- 7. the bucketed all-reduce over the reached stages, one rank on the real backend ------------------------------------------------
def test_token_bucketed_allreduce_on_rccl_single_rank(tmp_path):
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "rccl_tokens.pt")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "token_rccl_worker.py"), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = torch.load(out)
    assert res["buckets"] == [[2, 3], [3, 4], [4, 5]]     # VIT_TINY2 at depth 2: stage 1 (block 2) is unreached, three reached
    assert res["same"]


# ---- 8. full size, once ------------------------------------------------------------------------------------------------------------
def test_token_train_step_vit_l14():
    cfg = R.CONFIGS["ViT-L-14"]
    sd = R.random_state_dict(cfg, seed=0, device=dev())
    B = 8
    tr = AdversarialTrainer(cfg, sd, batch_size=B, precision="bf16", lr=1e-5, loss="l2-tokens", inner_loss="l2-tokens",
                            attack="pgd", iterations_adv=2, token_depth=-2)
    del sd
    x = torch.rand(B, 3, 224, 224, generator=torch.Generator(device="cuda").manual_seed(6), device=dev())
    lo = tr.params.stage_offsets[2]                       # head + block 23
    assert tr._token_span_lo == lo and lo > 12 * 1024 * 1024
    head = tr.params.flat[:lo].clone()
    body = tr.params.flat[lo:].clone()
    ws = tr.engine.workspace_bytes()
    out = tr.train_step(x, None)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"])) and float(out["loss"]) > 0
    assert tr.engine.workspace_bytes() == ws
    assert torch.equal(tr.params.flat[:lo], head)
    assert not torch.equal(tr.params.flat[lo:], body)
    tr.close()
