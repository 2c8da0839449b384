"""Token-level outputs of the encoder and their input gradient (RVLM_HAS_TOKENS) on the GPU: rvlm_vit_forward_tokens /
rvlm_vit_backward_input_tokens against oracle/vit_ref.py (vit_forward(return_tokens=True) on a config truncated to `depth` blocks,
fp64 autograd for the gradients), the token loss + seed kernel on its own against fp64 torch, the fused loop rvlm_pgd_run_tokens
against pgd()'s generic route through ClipVisionTower and against the oracle's pgd_ref, and one full-size run."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from oracle import vit_ref as V
from oracle import attacks_ref as A
from tests.gpu_helpers import dev, st, lib, cos_sim, rel_max, record

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_336_SLIM = V.VitConfig(336, 14, 128, 2, 2, 64)      # S = 577 (the 336 px towers' sequence) at a width the CPU oracle runs quickly


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


def make_engine(cfg, w, precision, max_batch=4, **kw):
    return R.VitEngine(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch, **kw)


def oracle_tokens(cfg, w, x, depth, ln_post=False, dtype=torch.float32):
    """(tokens [B, S, W], emb) of the first `depth` blocks; x in [0,1] at any size (bicubic to the model's own first)."""
    wd = {k: v.to(dtype) for k, v in w.items()}
    x = x.to(dtype)
    if tuple(x.shape[-2:]) != (cfg.image_size, cfg.image_size):
        x = F.interpolate(x, size=(cfg.image_size, cfg.image_size), mode="bicubic", align_corners=False)
    emb, t = V.vit_forward(dataclasses.replace(cfg, layers=depth), wd, V.normalize_pixels(x), return_tokens=True)
    if ln_post:
        t = F.layer_norm(t, (cfg.width,), wd["ln_post.weight"], wd["ln_post.bias"], 1e-5)
    return t, emb


def oracle_grad(cfg, w, x, depth, ln_post, d_tok, d_emb=None):
    xr = x.double().clone().requires_grad_(True)
    t, emb = oracle_tokens(cfg, w, xr, depth, ln_post, torch.float64)
    loss = (t * d_tok.double()).sum()
    if d_emb is not None:
        loss = loss + (emb * d_emb.double()).sum()
    return torch.autograd.grad(loss, xr)[0]


def sign_agree(a, b):
    return float(np.mean(np.sign(a.cpu().numpy()) == np.sign(b.cpu().numpy())))


def depths(cfg):
    return sorted({1, cfg.layers - 1, cfg.layers})


# ----------------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("cfg", [V.VIT_TINY2, V.VIT_B_32], ids=["tiny2", "b32"])
def test_forward_tokens_vs_oracle(cfg, precision):
    w = V.init_weights(cfg, seed=9)
    maxB = 4
    eng = make_engine(cfg, w, precision, max_batch=maxB)
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for B in (2, maxB):
        x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g)
        for depth in depths(cfg):
            for ln_post in (False, True):
                t_ref, _ = oracle_tokens(cfg, w, x, depth, ln_post)
                tok = eng.forward_tokens(x.to(dev()), depth=depth, ln_post=ln_post).cpu()
                assert tok.shape == (B, cfg.tokens, cfg.width)
                if precision == "bf16":
                    c = cos_sim(tok, t_ref)
                    assert c > 0.999, (B, depth, ln_post, c)
                    worst = max(worst, 1.0 - c)
                else:
                    e = rel_max(tok, t_ref)
                    assert e < (1e-5 if precision == "fp32" else 1e-4), (B, depth, ln_post, e)
                    worst = max(worst, e)
    record(f"forward_tokens_vs_oracle[{cfg.width},{precision}]", worst=worst)
    # LLaVA's select_layer convention and the default depth
    x = torch.rand(2, 3, cfg.image_size, cfg.image_size, generator=g).to(dev())
    assert torch.equal(eng.forward_tokens(x, depth=-2), eng.forward_tokens(x, depth=cfg.layers - 1))
    assert torch.equal(eng.forward_tokens(x), eng.forward_tokens(x, depth=cfg.layers))
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pooled_passes_are_untouched_by_token_passes(precision):
    """out_emb of a full-depth token pass is the pooled forward's embedding bit for bit on the fp32 handle; a pooled forward and its
    input gradient after token passes equal the ones before them bit for bit (the class-token tail of the bf16 handle is back)."""
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, precision)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(4, 3, cfg.image_size, cfg.image_size, generator=g).to(dev())
    cot = torch.randn(4, cfg.out_dim, generator=g).to(dev())
    e0 = eng.forward(x, None, False, save=True)
    g0 = eng.backward_input(cot)
    ws0 = eng.workspace_bytes()
    tok, emb = eng.forward_tokens(x, depth=cfg.layers, return_emb=True)
    if precision == "fp32":
        assert torch.equal(emb, e0)
    else:       # the bf16 handle's pooled pass runs the last block on the class rows only: same value, other kernels
        assert cos_sim(emb.cpu(), e0.cpu()) > 0.9999
    assert eng.workspace_bytes() == ws0, "a token pass without ln_post allocates nothing"
    eng.forward_tokens(x, depth=cfg.layers, ln_post=True, save=True)
    eng.backward_input_tokens(torch.randn(tok.shape, generator=g).to(dev()), d_emb=cot)
    assert eng.workspace_bytes() == ws0 + 2 * 256 * max(1, -(-4 * cfg.tokens // 256)) * 4, "ln_post statistics: 2 floats per row"
    eng.forward_tokens(x, depth=cfg.layers - 1, save=True)
    e1 = eng.forward(x, None, False, save=True)
    g1 = eng.backward_input(cot)
    assert torch.equal(e1, e0) and torch.equal(g1, g0)
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------------
def _cotangents(B, cfg, gen):
    dense = torch.randn(B, cfg.tokens, cfg.width, generator=gen)
    patch = dense.clone(); patch[:, 0] = 0
    cls = torch.zeros_like(dense); cls[:, 0] = dense[:, 0]
    return {"dense": dense, "patch": patch, "cls": cls}


@pytest.mark.parametrize("cfg", [V.VIT_TINY2, V.VIT_B_32], ids=["tiny2", "b32"])
def test_backward_tokens_fp32_vs_fp64_autograd(cfg):
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32")
    gen = torch.Generator().manual_seed(4)
    B = 2
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=gen)
    cots = _cotangents(B, cfg, gen)
    d_emb = torch.randn(B, cfg.out_dim, generator=gen)
    full = cfg.width == V.VIT_TINY2.width
    worst = 0.0
    for depth in depths(cfg):
        for ln_post in (False, True):
            for kind in (("dense", "patch", "cls") if full else ("dense",)):
                for with_emb in ((False, True) if depth == cfg.layers else (False,)):
                    de = d_emb if with_emb else None
                    g_ref = oracle_grad(cfg, w, x, depth, ln_post, cots[kind], de)
                    eng.forward_tokens(x.to(dev()), depth=depth, ln_post=ln_post, save=True)
                    gx = eng.backward_input_tokens(cots[kind].to(dev()), None if de is None else de.to(dev())).cpu()
                    e = rel_max(gx, g_ref)
                    assert e < 1e-4, (depth, ln_post, kind, with_emb, e)
                    worst = max(worst, e)
    record(f"backward_tokens_fp32[{cfg.width}]", worst=worst)
    eng.close()


def test_class_row_cotangent_reproduces_the_pooled_backward():
    """emb = ln_post(tokens[:, 0]) @ proj: the pooled path is the class row of a full-depth token pass."""
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32")
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(3, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev())
    d_emb = torch.randn(3, cfg.out_dim, generator=gen).to(dev())
    eng.forward(x, None, False, save=True)
    g_pooled = eng.backward_input(d_emb)
    zeros = torch.zeros(3, cfg.tokens, cfg.width, device=dev())
    # (a) through d_emb with a zero token cotangent: the same kernels on the same numbers
    eng.forward_tokens(x, depth=cfg.layers, save=True)
    assert torch.equal(eng.backward_input_tokens(zeros, d_emb), g_pooled)
    # (b) as a class-row-only token cotangent of the ln_post form: d_tokens[:, 0] = d_emb @ proj^T
    d_cls = zeros.clone()
    d_cls[:, 0] = d_emb @ w["proj"].to(dev()).T
    eng.forward_tokens(x, depth=cfg.layers, ln_post=True, save=True)
    assert rel_max(eng.backward_input_tokens(d_cls).cpu(), g_pooled.cpu()) < 1e-5
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tokens_at_577_tokens_and_at_an_odd_input_size(precision):
    """S = 577 (LLaVA-1.5's 336 px tower) and a set_input_size handle whose inputs are not the model's resolution."""
    gen = torch.Generator().manual_seed(6)
    for cfg, size in ((VIT_336_SLIM, None), (V.VIT_TINY2, (80, 72))):
        w = V.init_weights(cfg, seed=11)
        eng = make_engine(cfg, w, precision, max_batch=2)
        if size:
            eng.set_input_size(*size)
        hw = size or (cfg.image_size, cfg.image_size)
        x = torch.rand(2, 3, *hw, generator=gen)
        d_tok = torch.randn(2, cfg.tokens, cfg.width, generator=gen)
        depth = cfg.layers
        t_ref, _ = oracle_tokens(cfg, w, x, depth)
        g_ref = oracle_grad(cfg, w, x, depth, False, d_tok)
        tok = eng.forward_tokens(x.to(dev()), depth=depth, save=True).cpu()
        gx = eng.backward_input_tokens(d_tok.to(dev())).cpu()
        assert gx.shape == x.shape
        if precision == "fp32":
            assert rel_max(tok, t_ref) < 1e-5 and rel_max(gx, g_ref) < 1e-4, (cfg.tokens, rel_max(tok, t_ref), rel_max(gx, g_ref))
        else:
            assert cos_sim(tok, t_ref) > 0.999 and cos_sim(gx, g_ref) > 0.98, (cfg.tokens, cos_sim(tok, t_ref), cos_sim(gx, g_ref))
        eng.close()


def _child_bf16_backward():
    """Runs in a fresh process (RVLM_DRES_FP32 is read when a handle is created): the bf16 token backward with a dense seed against
    fp64 autograd and against the fp32 handle, one JSON line."""
    out = {}
    gen = torch.Generator().manual_seed(7)
    for name, cfg in (("tiny2", V.VIT_TINY2), ("b32", V.VIT_B_32)):
        w = V.init_weights(cfg, seed=9)
        B = 2
        x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=gen)
        cots = _cotangents(B, cfg, gen)
        d_emb = torch.randn(B, cfg.out_dim, generator=gen)
        e16, e32 = make_engine(cfg, w, "bf16"), make_engine(cfg, w, "fp32")
        for depth, kind, with_emb in ((cfg.layers - 1, "dense", False), (cfg.layers - 1, "patch", False), (cfg.layers, "dense", True),
                                      (cfg.layers, "cls", False)):
            de = d_emb if with_emb else None
            g_ref = oracle_grad(cfg, w, x, depth, False, cots[kind], de)
            gs = []
            for e in (e16, e32):
                e.forward_tokens(x.to(dev()), depth=depth, save=True)
                gs.append(e.backward_input_tokens(cots[kind].to(dev()), None if de is None else de.to(dev())).cpu())
            out[f"{name}/d{depth}/{kind}{'+emb' if with_emb else ''}"] = dict(
                cos=cos_sim(gs[0], g_ref), rel=rel_max(gs[0], g_ref), sign=sign_agree(gs[0], g_ref.float()),
                sign_vs_fp32=sign_agree(gs[0], gs[1]))
        e16.close(); e32.close()
    # the headline model: what the residual-gradient stream costs when the seed is dense (FARE over LLaVA's patch tokens), against
    # the fp32 handle's backward of the SAME cotangent
    torch.set_num_threads(32)
    cfg = V.VIT_L_14
    w = V.init_weights(cfg, seed=3)
    wd = {k: v.to(dev()) for k, v in w.items()}
    B, depth = 2, cfg.layers - 1
    x = torch.rand(B, 3, 224, 224, generator=gen).to(dev())
    d0 = ((torch.rand(x.shape, generator=gen) * 2 - 1) * (4 / 255)).to(dev())
    e32 = R.VitEngine(to_cfg(cfg), wd, precision="fp32", max_batch=B)
    ref = e32.forward_tokens(x, depth=depth)
    tok = e32.forward_tokens(x, d0, depth=depth, save=True)
    d = (tok - ref) * (2.0 / B)
    d[:, 0] = 0
    g32 = e32.backward_input_tokens(d).cpu()
    e32.close()
    e16 = R.VitEngine(to_cfg(cfg), wd, precision="bf16", max_batch=B)
    e16.forward_tokens(x, d0, depth=depth, save=True)
    g16 = e16.backward_input_tokens(d).cpu()
    e16.close()
    out["l14/d23/fare-patch"] = dict(cos=cos_sim(g16, g32), rel=rel_max(g16, g32), sign=sign_agree(g16, g32), sign_vs_fp32=sign_agree(g16, g32))
    print("TOKENS_CHILD " + json.dumps(out))


@pytest.mark.parametrize("dres_fp32", ["0", "1"])
def test_backward_tokens_bf16_both_residual_gradient_streams(dres_fp32):
    """bf16 handle, dense / patch-rows / class-row seeds: cosine, relative error and sign agreement with fp64 autograd, under the bf16-only
    residual-gradient stream (default) and the fp32 one (RVLM_DRES_FP32=1); on ViT-L/14 against the fp32 handle's backward of the same
    cotangent (what the stream costs when the seed is dense)."""
    env = dict(os.environ, RVLM_DRES_FP32=dres_fp32)
    try:
        r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_tokens import _child_bf16_backward as f; f()"], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        pytest.exit("the child process of the bf16 token backward hung: nothing more is started on this GPU", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139):      # killed by a signal: a GPU fault ends the session
        pytest.exit(f"the child process of the bf16 token backward died ({r.returncode}):\n{r.stderr[-4000:]}", returncode=3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("TOKENS_CHILD ")][-1]
    res = json.loads(line[len("TOKENS_CHILD "):])
    for case, m in res.items():
        record(f"backward_tokens_bf16[dres_fp32={dres_fp32}]/{case}", **m)
        # measured: cosine >= 0.99994, relative error <= 1.0e-2, sign agreement >= 0.9966 (bf16-only stream; ViT-L/14 dense seed against
        # the fp32 handle 0.9978) and >= 0.9969 (fp32 stream; ViT-L/14 0.9992)
        assert m["cos"] > 0.9995, (case, m)
        assert m["rel"] < 0.05, (case, m)
        assert m["sign"] > 0.99 and m["sign_vs_fp32"] > 0.99, (case, m)


# ----------------------------------------------------------------------------------------------------------------------------------
# state
# ----------------------------------------------------------------------------------------------------------------------------------
def test_token_and_pooled_passes_do_not_mix():
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    gen = torch.Generator().manual_seed(8)
    x = torch.rand(3, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev())
    d_tok = torch.randn(3, cfg.tokens, cfg.width, generator=gen).to(dev())
    d_emb = torch.randn(3, cfg.out_dim, generator=gen).to(dev())
    for precision in ("bf16", "fp32"):
        eng = make_engine(cfg, w, precision)
        with pytest.raises(L.RvlmError, match="no saved token forward"):
            eng.backward_input_tokens(d_tok)
        eng.forward_tokens(x, depth=2, save=True)
        with pytest.raises(L.RvlmError, match=r"status 3.*token pass"):
            eng.backward_input(d_emb)
        with pytest.raises(ValueError, match="depth == layers"):          # d_emb needs the head to have run
            eng.backward_input_tokens(d_tok, d_emb)
        with pytest.raises(L.RvlmError, match="no saved token forward"):  # another batch size
            eng.backward_input_tokens(d_tok[:2])
        assert torch.isfinite(eng.backward_input_tokens(d_tok)).all()     # the refusals above left the saved pass alone
        eng.forward(x, None, False, save=True)
        with pytest.raises(L.RvlmError, match=r"status 3.*pooled pass"):
            eng.backward_input_tokens(d_tok)
        eng.forward_tokens(x, depth=2, save=True)
        eng.forward_tokens(x, depth=2, save=False)                        # any later forward invalidates
        with pytest.raises(L.RvlmError, match="no saved token forward"):
            eng.backward_input_tokens(d_tok)
        for bad in (0, cfg.layers + 1):
            assert lib().rvlm_vit_forward_tokens(eng._h, x.data_ptr(), None, 3, bad, 0, 0, d_tok.data_ptr(), None, st()) == L.RVLM_ERR_ARG
        assert lib().rvlm_vit_forward_tokens(eng._h, x.data_ptr(), None, 3, 2, 0, 0, d_tok.data_ptr(), d_emb.data_ptr(),
                                             st()) == L.RVLM_ERR_ARG      # no embedding below full depth
        eng.close()
    # the handoff: an fp32-storage handle's saved token pass is not the bf16 handle's to differentiate
    e16, e32 = make_engine(cfg, w, "bf16"), make_engine(cfg, w, "fp32")
    e32.forward_tokens(x, depth=cfg.layers, save=True)
    gx = torch.empty_like(x)
    assert lib().rvlm_vit_backward_input_from(e16._h, e32._h, d_emb.data_ptr(), 3, gx.data_ptr(), st()) == L.RVLM_ERR_STATE
    e16.close(); e32.close()
    # trainable handles: no weight gradients from a token pass
    et = make_engine(cfg, w, "fp32", trainable=True)
    et.forward_tokens(x, depth=cfg.layers, save=True)
    grads = {k: torch.zeros_like(v).to(dev()) for k, v in w.items()}
    with pytest.raises(L.RvlmError, match="status 3"):
        et.backward_params(d_emb, grads)
    et.close()


def test_provider_and_inference_only_handles_refuse_saving_token_passes():
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev())
    tok = torch.empty(2, cfg.tokens, cfg.width, device=dev())
    gx = torch.empty_like(x)
    mixed = make_engine(cfg, w, "bf16+x3fwd-first")          # its second handle is a forward provider (trainable = -2)
    with pytest.raises(ValueError, match="plain precisions"):
        mixed.forward_tokens(x)
    assert lib().rvlm_vit_forward_tokens(mixed._h32, x.data_ptr(), None, 2, 2, 0, 1, tok.data_ptr(), None, st()) == L.RVLM_ERR_STATE
    assert b"forward-provider" in lib().rvlm_last_error()
    assert lib().rvlm_vit_backward_input_tokens(mixed._h32, tok.data_ptr(), None, 2, gx.data_ptr(), st()) == L.RVLM_ERR_STATE
    assert lib().rvlm_pgd_run_tokens(mixed._h32, x.data_ptr(), None, 2, 2, 0, 0, tok.data_ptr(), 0, 0, 0.01, 1, 0.01, 0.9, 1,
                                     gx.data_ptr(), None, None, st()) == L.RVLM_ERR_STATE
    mixed.close()
    inf = make_engine(cfg, w, "bf16", inference_only=True)
    with pytest.raises(L.RvlmError, match="inference-only"):
        inf.forward_tokens(x, depth=2, save=True)
    with pytest.raises(L.RvlmError, match="inference-only"):
        inf.backward_input_tokens(tok)
    t_ref, _ = oracle_tokens(cfg, w, x.cpu(), 2)
    assert cos_sim(inf.forward_tokens(x, depth=2).cpu(), t_ref) > 0.999      # gradient-free token passes are fine there
    inf.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernels on their own
# ----------------------------------------------------------------------------------------------------------------------------------
def _loss_kernel(t, ref, select, reduction, want32=True, want16=True, seed_rows=0, flags=None):
    B, S, W = t.shape
    rows = seed_rows or B * S
    s32 = torch.full((rows, W), float("nan"), device=dev()) if want32 else None
    s16 = torch.full((rows, W), float("nan"), device=dev(), dtype=torch.bfloat16) if want16 else None
    per = torch.empty(B, device=dev())
    scalar = torch.empty(1, device=dev())
    scratch = torch.empty(B * ((S + 7) // 8), device=dev())
    L.check(lib().rvlm_tokens_l2_loss_grad(t.data_ptr(), ref.data_ptr(), B, S, W, select, reduction, L.ptr(s32), L.ptr(s16), seed_rows,
                                           per.data_ptr(), scalar.data_ptr(), scratch.data_ptr(), L.ptr(flags), st()),
            "rvlm_tokens_l2_loss_grad")
    torch.cuda.synchronize()
    return per, scalar, s32, s16


@pytest.mark.parametrize("B,S,W", [(3, 37, 128), (2, 257, 1024), (5, 50, 768)])
@pytest.mark.parametrize("select", [L.TOKENS_ALL, L.TOKENS_PATCH])
@pytest.mark.parametrize("reduction", [L.RED_MEAN, L.RED_NONE])
def test_token_loss_kernel_vs_fp64(B, S, W, select, reduction):
    gen = torch.Generator().manual_seed(10)
    t = torch.randn(B, S, W, generator=gen)
    ref = t[:, select:] + 0.1 * torch.randn(B, S - select, W, generator=gen)
    rows = -(-B * S // 256) * 256
    per, scalar, s32, s16 = _loss_kernel(t.to(dev()), ref.to(dev()).contiguous(), select, reduction, seed_rows=rows)
    d = t.double()[:, select:] - ref.double()
    per_ref = d.pow(2).sum(dim=(1, 2))
    assert rel_max(per.cpu(), per_ref) < 1e-5
    sc_ref = per_ref.mean() if reduction == L.RED_MEAN else per_ref.sum()
    assert abs(float(scalar) - float(sc_ref)) <= 1e-5 * abs(float(sc_ref))
    seed_ref = torch.zeros(rows, W, dtype=torch.float64)
    full = torch.zeros(B, S, W, dtype=torch.float64)
    full[:, select:] = 2 * d * ((1.0 / B) if reduction == L.RED_MEAN else 1.0)
    seed_ref[:B * S] = full.reshape(B * S, W)
    assert torch.isfinite(s32).all() and torch.isfinite(s16.float()).all(), "every row of the seed is written (pad rows included)"
    assert rel_max(s32.cpu(), seed_ref) < 1e-6
    assert torch.equal(s16, s32.to(torch.bfloat16)), "the bf16 seed is the fp32 one rounded once"
    zero_rows = torch.ones(rows, dtype=torch.bool)
    sel = torch.zeros(B, S, dtype=torch.bool); sel[:, select:] = True
    zero_rows[:B * S] = ~sel.reshape(-1)
    assert (s32.cpu()[zero_rows] == 0).all() and (s16.cpu()[zero_rows] == 0).all()
    # either form alone, and none (loss only), give the same loss bits; a second run gives the same bits everywhere
    per_b, scalar_b, s32_b, s16_b = _loss_kernel(t.to(dev()), ref.to(dev()).contiguous(), select, reduction, seed_rows=rows)
    assert torch.equal(per, per_b) and torch.equal(scalar, scalar_b) and torch.equal(s32, s32_b) and torch.equal(s16, s16_b)
    per_c, _, _, s16_c = _loss_kernel(t.to(dev()), ref.to(dev()).contiguous(), select, reduction, want32=False, seed_rows=rows)
    per_d, _, _, _ = _loss_kernel(t.to(dev()), ref.to(dev()).contiguous(), select, reduction, want32=False, want16=False)
    assert torch.equal(per, per_c) and torch.equal(per, per_d) and torch.equal(s16, s16_c)


def test_token_loss_kernel_flags_a_non_finite_image_and_ends():
    gen = torch.Generator().manual_seed(11)
    t = torch.randn(4, 37, 128, generator=gen)
    ref = torch.randn(4, 37, 128, generator=gen)
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    _loss_kernel(t.to(dev()), ref.to(dev()), L.TOKENS_ALL, L.RED_MEAN, flags=flags)
    assert int(flags) == 0
    t[2, 17, 5] = float("nan")
    per, scalar, _, _ = _loss_kernel(t.to(dev()), ref.to(dev()), L.TOKENS_ALL, L.RED_MEAN, flags=flags)
    assert int(flags) == L.FLAG_TOKENS_NONFINITE
    assert torch.isnan(per[2]) and torch.isfinite(per[[0, 1, 3]]).all() and torch.isnan(scalar).all()
    t[2, 17, 5] = float("inf")
    flags.zero_()
    _loss_kernel(t.to(dev()), ref.to(dev()), L.TOKENS_ALL, L.RED_NONE, flags=flags)
    assert int(flags) == L.FLAG_TOKENS_NONFINITE
    # argument checks
    a = torch.zeros(2, 37, 128, device=dev())
    p = torch.zeros(2, device=dev())
    assert lib().rvlm_tokens_l2_loss_grad(a.data_ptr(), a.data_ptr(), 2, 37, 128, 2, 0, None, None, 0, p.data_ptr(), None, a.data_ptr(), None,
                                          st()) == L.RVLM_ERR_ARG
    assert lib().rvlm_tokens_l2_loss_grad(a.data_ptr(), a.data_ptr(), 2, 37, 128, 0, 0, a.data_ptr(), None, 5, p.data_ptr(), None,
                                          a.data_ptr(), None, st()) == L.RVLM_ERR_ARG      # seed_rows < B * S


@pytest.mark.parametrize("M,Mp,S,W", [(74, 256, 37, 128), (514, 768, 257, 1024)])
def test_token_seed_kernel(M, Mp, S, W):
    gen = torch.Generator().manual_seed(12)
    d = torch.randn(M, W, generator=gen).to(dev())
    cls = torch.randn(M // S, W, generator=gen).to(dev())
    for add in (None, cls):
        s32 = torch.full((Mp, W), float("nan"), device=dev())
        s16 = torch.full((Mp, W), float("nan"), device=dev(), dtype=torch.bfloat16)
        L.check(lib().rvlm_k_tokens_seed(d.data_ptr(), L.ptr(add), s32.data_ptr(), s16.data_ptr(), M, Mp, S, W, st()))
        torch.cuda.synchronize()
        want = torch.zeros(Mp, W, device=dev())
        want[:M] = d
        if add is not None:
            want[0:M:S] += add
        assert torch.equal(s32, want) and torch.equal(s16, want.to(torch.bfloat16))
        only16 = torch.full((Mp, W), float("nan"), device=dev(), dtype=torch.bfloat16)
        L.check(lib().rvlm_k_tokens_seed(d.data_ptr(), L.ptr(add), None, only16.data_ptr(), M, Mp, S, W, st()))
        torch.cuda.synchronize()
        assert torch.equal(only16, s16)


# ----------------------------------------------------------------------------------------------------------------------------------
# the fused step and loop
# ----------------------------------------------------------------------------------------------------------------------------------
def _token_l2(ref):
    return lambda out, targets: ((out - ref) ** 2).sum(dim=(1, 2)).mean()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("ln_post", [False, True])
def test_tokens_fwd_inputgrad_equals_the_separate_calls(precision, ln_post):
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, precision)
    gen = torch.Generator().manual_seed(13)
    x = torch.rand(4, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev())
    d0 = ((torch.rand(x.shape, generator=gen) * 2 - 1) * (4 / 255)).to(dev())
    for depth, select in ((cfg.layers - 1, "patch"), (cfg.layers, "all")):
        first = 1 if select == "patch" else 0
        ref = eng.forward_tokens(x, depth=depth, ln_post=ln_post)[:, first:].contiguous()
        for reduction in ("mean", "none"):
            tok, per, scalar, gx = eng.tokens_fwd_inputgrad(x, d0, ref, depth=depth, ln_post=ln_post, select=select,
                                                            reduction=reduction, want_tokens=True)
            tok2 = eng.forward_tokens(x, d0, depth=depth, ln_post=ln_post, save=True)
            assert torch.equal(tok, tok2)
            d = torch.zeros_like(tok2)
            d[:, first:] = 2 * (tok2[:, first:] - ref) * ((1.0 / 4) if reduction == "mean" else 1.0)
            gx2 = eng.backward_input_tokens(d)
            per_ref = (tok2[:, first:].double() - ref.double()).pow(2).sum(dim=(1, 2))
            assert rel_max(per.cpu(), per_ref.cpu()) < 1e-5
            sc = per_ref.mean() if reduction == "mean" else per_ref.sum()
            assert abs(float(scalar) - float(sc)) <= 1e-5 * abs(float(sc))
            if precision == "fp32":
                assert rel_max(gx.cpu(), gx2.cpu()) < 1e-5, (depth, reduction, rel_max(gx.cpu(), gx2.cpu()))
            else:
                assert cos_sim(gx.cpu(), gx2.cpu()) > 0.999
    eng.close()


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("iters", [3, 10])
@pytest.mark.parametrize("select_layer,select_feature", [(-2, "patch"), (-1, "cls_patch")])
def test_pgd_run_tokens_vs_generic_route_and_oracle(norm, iters, select_layer, select_feature):
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32")
    tower = R.ClipVisionTower(eng, select_layer=select_layer, select_feature=select_feature).eval()
    gen = torch.Generator().manual_seed(14)
    B = 4
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=gen)
    eps, step = (4 / 255, 1 / 255) if norm == "linf" else (1.5, 0.4)
    d0 = (torch.rand(x.shape, generator=gen) * 2 - 1) * (4 / 255)
    xd, d0d = x.to(dev()), d0.to(dev())
    with torch.no_grad():
        ref = tower(xd).clone()
    assert ref.shape == (B, cfg.tokens - (select_feature == "patch"), cfg.width)
    wrap = R.ComputeLossWrapper(ref, None, "mean", "l2")
    xadv = R.pgd(tower, wrap, xd, None, norm, eps, iters, step, False, perturbation=d0d.clone(), mode="max")
    loss_expr = _token_l2(ref)
    xadv2 = R.pgd(lambda v, output_normalize: tower(v), loss_expr, xd, None, norm, eps, iters, step, False, perturbation=d0d.clone(),
                  mode="max")
    got, got2 = xadv.cpu().numpy(), xadv2.cpu().numpy()
    delta = got - x.numpy()
    assert got.min() >= 0.0 and got.max() <= 1.0
    if norm == "linf":
        assert np.abs(delta).max() <= np.float32(eps)
        same = float(np.mean(got == got2))
        assert same > 0.999, same
    else:
        assert np.sqrt((delta.reshape(B, -1) ** 2).sum(1)).max() <= eps * (1 + 1e-5)
        same = float(np.mean(np.abs(got - got2) <= 1e-6))
        assert same > 0.999, same
    with torch.no_grad():
        lf, lf2 = float(loss_expr(tower(xadv), None)), float(loss_expr(tower(xadv2), None))
        assert abs(lf - float(wrap(tower(xadv), None))) <= 1e-5 * lf        # the wrapper's l2 on tokens is the same loss
    assert abs(lf - lf2) <= 1e-5 * abs(lf2), (lf, lf2)
    # the oracle's pgd on the oracle's tower
    depth, first = cfg.layers + 1 + select_layer, int(select_feature == "patch")
    ref_o = oracle_tokens(cfg, w, x, depth)[0][:, first:].detach()
    x_o = A.pgd_ref(lambda v, output_normalize: oracle_tokens(cfg, w, v, depth)[0][:, first:], _token_l2(ref_o), x, None, norm, eps,
                    iters, step, False, perturbation=d0.clone(), mode="max").numpy()
    lo = float(_token_l2(ref_o)(oracle_tokens(cfg, w, torch.from_numpy(x_o), depth)[0][:, first:], None))
    if norm == "linf":
        same_o = float(np.mean(got == x_o))
        assert same_o > 0.95, f"only {same_o:.3f} of the pixels identical to the oracle's x_adv"
    else:
        same_o = 1.0 - float(np.linalg.norm(got - x_o) / np.linalg.norm(x_o - x.numpy()))
        assert same_o > 0.95, same_o
    assert abs(lf - lo) <= 0.05 * abs(lo), (lf, lo)
    record(f"pgd_run_tokens[{norm},{iters},{select_layer},{select_feature}]", same_generic=same, same_oracle=same_o, loss=lf, loss_oracle=lo)
    eng.close()


def test_pgd_on_tokens_rejects_what_does_not_fit():
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32")
    tower = R.ClipVisionTower(eng)
    x = torch.rand(2, 3, cfg.image_size, cfg.image_size).to(dev())
    bad_ref = torch.zeros(2, cfg.tokens, cfg.width, device=dev())           # 'patch' towers return S - 1 rows
    with pytest.raises(ValueError, match="reference tokens"):
        R.pgd(tower, R.ComputeLossWrapper(bad_ref, None, "mean", "l2"), x, None, "linf", 4 / 255, 2, 1 / 255, False, mode="max")
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    out = torch.empty_like(x)
    ref = torch.full((2, cfg.tokens - 1, cfg.width), float("nan"), device=dev())
    L.check(lib().rvlm_pgd_run_tokens(eng._h, x.data_ptr(), None, 2, 2, 0, L.TOKENS_PATCH, ref.data_ptr(), L.RED_MEAN, 0, 4 / 255, 2,
                                      1 / 255, 0.9, 1, out.data_ptr(), None, flags.data_ptr(), st()))
    assert int(flags) & L.FLAG_TOKENS_NONFINITE
    with pytest.raises(AssertionError, match="non-finite token loss"):
        R.pgd(tower, R.ComputeLossWrapper(ref, None, "mean", "l2"), x, None, "linf", 4 / 255, 2, 1 / 255, False, mode="max")
    assert lib().rvlm_pgd_run_tokens(eng._h, x.data_ptr(), None, 2, 2, 0, L.TOKENS_PATCH, ref.data_ptr(), L.RED_MEAN, 1, 4 / 255, 2,
                                     1 / 255, 0.9, 1, out.data_ptr(), None, flags.data_ptr(), st()) == L.RVLM_ERR_UNSUPPORTED
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# autograd through the tower
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select_layer,select_feature", [(-2, "patch"), (-1, "cls_patch")])
def test_tower_autograd(select_layer, select_feature):
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32")
    tower = R.ClipVisionTower(eng, select_layer=select_layer, select_feature=select_feature)
    gen = torch.Generator().manual_seed(15)
    x = torch.rand(2, 3, cfg.image_size, cfg.image_size, generator=gen).to(dev()).requires_grad_(True)
    (g1,) = torch.autograd.grad(tower(x).square().sum(), x)
    tok = eng.forward_tokens(x.detach(), depth=tower.depth, save=True)
    d = 2 * tok
    if select_feature == "patch":
        d[:, 0] = 0
    g2 = eng.backward_input_tokens(d)
    assert rel_max(g1.cpu(), g2.cpu()) < 1e-6
    # one live graph per engine
    out = tower(x)
    with torch.no_grad():
        tower(x.detach())
    with pytest.raises(RuntimeError, match="overwritten"):
        out.sum().backward()
    # central differences on the three pixels with the largest gradient
    cot = torch.randn(tower(x.detach()).shape, generator=gen).to(dev())
    (g,) = torch.autograd.grad((tower(x) * cot).sum(), x)
    flat = g.flatten()
    h = 1e-2
    for idx in flat.abs().topk(3).indices.tolist():
        xp, xm = x.detach().clone().flatten(), x.detach().clone().flatten()
        xp[idx] += h; xm[idx] -= h
        with torch.no_grad():
            fp = float((tower(xp.view_as(x)).double() * cot.double()).sum())
            fm = float((tower(xm.view_as(x)).double() * cot.double()).sum())
        fd = (fp - fm) / (2 * h)
        assert abs(fd - float(flat[idx])) <= 0.05 * abs(float(flat[idx])) + 0.02, (idx, fd, float(flat[idx]))
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------------------
# full size
# ----------------------------------------------------------------------------------------------------------------------------------
def test_full_size_token_fare_pgd_vit_l14_bf16():
    """ViT-L/14, bf16, B = 8, LLaVA's tower (depth 23, patch rows): 10 steps of the token-FARE attack, then two at full depth."""
    torch.set_num_threads(32)
    cfg = V.VIT_L_14
    w = V.init_weights(cfg, seed=3)
    torch.set_num_threads(8)
    wd = {k: v.to(dev()) for k, v in w.items()}
    B, depth = 8, cfg.layers - 1
    eng = R.VitEngine(to_cfg(cfg), wd, precision="bf16", max_batch=B)
    gen = torch.Generator().manual_seed(16)
    x = torch.rand(B, 3, 224, 224, generator=gen).to(dev())
    eps = 4 / 255
    d0 = ((torch.rand(x.shape, generator=gen) * 2 - 1) * eps).to(dev())
    ref = eng.forward_tokens(x, depth=depth)[:, 1:].contiguous()
    xadv, flags, trace = eng.pgd_run_tokens(x, d0, ref, eps, 10, eps / 4, 0.9, "max", depth=depth, select="patch", want_trace=True)
    torch.cuda.synchronize()
    tr = trace.cpu().numpy()
    assert int(flags) == 0
    assert torch.isfinite(xadv).all() and np.isfinite(tr).all()
    assert float((xadv - x).abs().max()) <= float(np.float32(eps)) and float(xadv.min()) >= 0 and float(xadv.max()) <= 1
    assert tr[0] < tr[1] < tr[2], tr[:4]
    assert tr[-1] > tr[0]
    # the same at full depth (OpenFlamingo's tower: the class-token tail bypassed), two iterations
    ref_l = eng.forward_tokens(x, depth=cfg.layers)[:, 1:].contiguous()
    xadv_l, flags_l, tr_l = eng.pgd_run_tokens(x, d0, ref_l, eps, 2, eps / 4, 0.9, "max", depth=cfg.layers, select="patch", want_trace=True)
    assert int(flags_l) == 0 and torch.isfinite(xadv_l).all() and float(tr_l[0]) < float(tr_l[1])
    record("tokens_l14_bf16_pgd", loss_first=float(tr[0]), loss_last=float(tr[-1]), loss_full_depth_first=float(tr_l[0]))
    eng.close()
