"""Engine sweep over widths and sequence lengths no other test builds (2 layers each, against oracle/vit_ref.py on the CPU).

On ONE handle with max_batch 8 every precision runs B = 3, then B = 8, then B = 3 again: the first and the third result must be bit
identical (stale pad rows of a 256-row GEMM tile, a stale split copy), and each is held to the suite's bars for its precision.  Between
them the configurations make an x3 handle's linears all take the split-bf16 GEMM (W % 256 == 0, M >= 256), none take it (other widths:
the handle then equals the fp32 handle bit for bit at any M), and put M on either side of 256 on one handle (S = 65: 195 / 520 rows)."""
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd.trainer import FlatParams
from oracle import vit_ref as V
from tests.gpu_helpers import dev, cos_sim, rel_max, record

pytestmark = pytest.mark.gpu

# (width, image, patch, clip-like weights): S = 65 (64 px / 8), 197 (224 / 16), 257 (224 / 14)
SHAPES = [(128, 64, 8, False), (384, 224, 16, False), (384, 224, 14, False), (512, 64, 8, False), (512, 224, 14, True),
          (640, 64, 8, False), (640, 224, 14, False), (768, 64, 8, False), (768, 224, 16, False), (1536, 64, 8, False)]


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


def run_sequence(eng, x, cot, handoff):
    """(embedding, input gradient) for B = 3, 8, 3 on one handle."""
    out = []
    for B in (3, 8, 3):
        xb, cb = x[:B].to(dev()), cot[:B].to(dev())
        if handoff:
            emb, gx = eng.handoff_inputgrad(xb, None, output_normalize=False, cot=cb)
        else:
            emb = eng.forward(xb, None, False, save=True)
            gx = eng.backward_input(cb)
        torch.cuda.synchronize()
        out.append((emb.clone(), gx.clone()))
    return out


@pytest.mark.parametrize("W,img,P,clip_like", SHAPES)
def test_engine_shape_sweep(W, img, P, clip_like):
    cfg = V.VitConfig(img, P, W, 2, W // 64, 64)
    S = (img // P) ** 2 + 1
    w = V.init_weights(cfg, seed=W + S, clip_like=clip_like)
    ref = V.ClipVisionModelRef(cfg, w).eval()
    g = torch.Generator().manual_seed(S)
    x = torch.rand(8, 3, img, img, generator=g)
    cot = torch.randn(8, cfg.out_dim, generator=g)
    xr = x.clone().requires_grad_(True)
    e_ref = ref(xr, False)
    (g_ref,) = torch.autograd.grad((e_ref * cot).sum(), xr)         # per image: rows [:3] are the B = 3 oracle
    e_ref = e_ref.detach()
    wd = {k: v.to(dev()) for k, v in w.items()}
    res, err = {}, {}
    for prec in ("fp32", "x3", "bf16", "bf16+x3fwd-first"):
        eng = R.VitEngine(to_cfg(cfg), wd, precision=prec, max_batch=8)
        try:
            res[prec] = run_sequence(eng, x, cot, prec == "bf16+x3fwd-first")
        finally:
            eng.close()
        (e3, g3), (e8, g8), (e3b, g3b) = res[prec]
        assert torch.equal(e3, e3b) and torch.equal(g3, g3b), f"{prec}: B = 3 after B = 8 differs from B = 3 on a fresh handle"
        err[prec] = [(rel_max(e.cpu(), e_ref[:n]), rel_max(gx.cpu(), g_ref[:n])) for n, (e, gx) in ((3, (e3, g3)), (8, (e8, g8)))]
    for i, B in enumerate((3, 8)):
        tag = f"W {W} S {S} B {B}"
        e32, ex3, e16, eho = (err[p][i] for p in ("fp32", "x3", "bf16", "bf16+x3fwd-first"))
        assert e32[0] < 1e-4 and e32[1] < 1e-3, (tag, e32)
        takes = W % 256 == 0 and B * S >= 256                 # linear.h x3_takes for every encoder linear of these shapes
        if takes:
            assert ex3[0] < 5e-5 and ex3[1] < 2e-4, (tag, ex3)
            assert ex3[0] < 0.05 * e16[0] and ex3[1] < 0.05 * e16[1], (tag, ex3, e16)
        else:                                                  # everything on the fp32 tiles: the fp32 handle, bit for bit
            assert torch.equal(res["x3"][i][0], res["fp32"][i][0]) and torch.equal(res["x3"][i][1], res["fp32"][i][1]), tag
        n = (3, 8)[i]
        assert cos_sim(res["bf16"][i][0].cpu(), e_ref[:n]) > 0.999 and cos_sim(res["bf16"][i][1].cpu(), g_ref[:n]) > 0.98, (tag, e16)
        # the handoff: the forward is the x3 handle's, the gradient agrees with the oracle like the bf16 engine's own backward does
        assert eho[0] < 1e-4, (tag, eho)
        assert eho[1] < 3e-2 and eho[1] < 1.5 * e16[1] + 1e-3, (tag, eho, e16)
        record("engine_shape_sweep", W=W, S=S, B=B, takes=takes, fp32_emb=e32[0], fp32_grad=e32[1], x3_emb=ex3[0], x3_grad=ex3[1],
               bf16_emb=e16[0], bf16_grad=e16[1], handoff_grad=eho[1])


@pytest.mark.parametrize("W", [384, 512])
def test_weight_gradients_at_untested_widths(W):
    """backward_params of the trainable bf16 engine where W % 256 != 0 sends every linear's weight gradient through the transposing
    fallback (W = 384), and at the smallest width the copy-free form takes (W = 512); bars of tests/test_gpu_trainer.py."""
    cfg = V.VitConfig(64, 8, W, 2, W // 64, 64)
    B = 8
    w = V.init_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g)
    cot = torch.randn(B, cfg.out_dim, generator=g)
    wr = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    e = torch.nn.functional.normalize(V.vit_forward(cfg, wr, V.normalize_pixels(x)), dim=-1)
    (e * cot).sum().backward()
    eng = R.VitEngine(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, precision="bf16", max_batch=B, trainable=True)
    try:
        grads = FlatParams(to_cfg(cfg), None, dev())
        eng.forward(x.to(dev()), None, True, save=2)
        eng.backward_params(cot.to(dev()), grads.views, accumulate=False)
        torch.cuda.synchronize()
        for k, v in wr.items():
            c = cos_sim(grads.views[k].cpu(), v.grad)
            assert c > 0.97, f"{k}: cos {c}"
    finally:
        eng.close()


def test_bf16_engine_refuses_sequences_beyond_the_attention_kernels():
    """400 px / 16: 626 tokens - inside the bf16 forward's limit (640), beyond the backward's (608).  A handle that may be asked for a
    gradient is refused at creation; an inference-only handle is built and runs."""
    cfg = V.VitConfig(400, 16, 64, 1, 1, 32)
    w = V.init_weights(cfg, seed=1)
    wd = {k: v.to(dev()) for k, v in w.items()}
    with pytest.raises(NotImplementedError):
        R.VitEngine(to_cfg(cfg), wd, precision="bf16", max_batch=2)
    with pytest.raises(NotImplementedError):
        R.VitEngine(to_cfg(cfg), wd, precision="bf16", max_batch=2, trainable=True)
    eng = R.VitEngine(to_cfg(cfg), wd, precision="bf16", max_batch=2, inference_only=True)
    try:
        x = torch.rand(2, 3, 400, 400, generator=torch.Generator().manual_seed(3))
        emb = eng.forward(x.to(dev()), None, False, save=False)
        torch.cuda.synchronize()
        assert cos_sim(emb.cpu(), V.ClipVisionModelRef(cfg, w).eval()(x, False).detach()) > 0.999
    finally:
        eng.close()
    big = V.VitConfig(416, 16, 64, 1, 1, 32)                      # 677 tokens: beyond the forward's limit too
    with pytest.raises(NotImplementedError):
        R.VitEngine(to_cfg(big), {k: v.to(dev()) for k, v in V.init_weights(big, seed=1).items()}, precision="bf16", max_batch=2,
                    inference_only=True)
