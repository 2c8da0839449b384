"""The CLIP text tower on the GPU: causal flash attention (both storage forms), the token-embedding front end, TextEngine against the
CPU oracle (oracle/text_ref.py), causality / active length / chunking as the user sees them, and the zero-shot head end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from oracle import text_ref as T
from tests.gpu_helpers import dev, st, lib, record

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# --------------------------------------------------------------------------------------------------------------------------
# causal attention
# --------------------------------------------------------------------------------------------------------------------------
def causal_ref(qkv, B, H, S):
    W = 64 * H
    q, k, v = (t.reshape(B, S, H, 64).transpose(1, 2).double() for t in qkv.split(W, dim=1))
    o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    return o.transpose(1, 2).reshape(B * S, W)


def run_causal(form, qkv, B, H, S, active=0, o=None):
    l = lib()
    W = 64 * H
    if form == "bf16":
        qkv = qkv.bfloat16()
        o = torch.full((B * S, W), float("nan"), dtype=torch.bfloat16, device=dev()) if o is None else o
        L.check(l.rvlm_k_attn_causal_fwd_bf16(qkv.data_ptr(), o.data_ptr(), B, H, S, active, st()))
    else:
        o = torch.full((B * S, W), float("nan"), device=dev()) if o is None else o
        L.check(l.rvlm_k_attn_causal_fwd_f32(qkv.data_ptr(), o.data_ptr(), B, H, S, active, st()))
    torch.cuda.synchronize()
    return qkv, o


# fp32: the bar of the fp32 flash forward of the image tower (test_attn_fwd_f32_flash); bf16: the bar of the existing bf16 forward
# tests (bf16 storage of q, k, v, P and o)
BARS = {"f32": 2e-6, "bf16": 2e-2}


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("H", [2, 8, 12])
@pytest.mark.parametrize("S", [77, 2, 31, 32, 33, 64, 96])
def test_causal_attention(form, S, H):
    B = 3
    W = 64 * H
    g = torch.Generator(device=dev()).manual_seed(100 * S + H)
    qkv = torch.randn(B * S, 3 * W, generator=g, device=dev())
    qkv[:, :W] *= 2.0                                   # logits with a spread of a few units
    qkv_used, o = run_causal(form, qkv, B, H, S)
    want = causal_ref(qkv_used.float(), B, H, S)
    err = float((o.double() - want).abs().max() / want.abs().max())
    record(f"causal_attention_{form}", S=S, H=H, err=err)
    assert err < BARS[form], err


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("qi,ki", [(76, 70), (76, 3), (40, 33), (33, 32), (70, 64)])
def test_causal_attention_forced_large_scores(form, qi, ki):
    """One key dominates a query late in the sequence (the online-softmax rescale across key tiles and inside the diagonal tile)."""
    B, H, S = 1, 1, 77
    g = torch.Generator(device=dev()).manual_seed(11 + qi + ki)
    qkv = torch.randn(S, 192, generator=g, device=dev())
    qkv[qi, 0:64] = 6.0 * qkv[ki, 64:128]              # q_qi . k_ki >> the others
    qkv_used, o = run_causal(form, qkv, B, H, S)
    want = causal_ref(qkv_used.float(), B, H, S)
    err = float((o.double() - want).abs().max() / want.abs().max())
    assert err < BARS[form], err


@pytest.mark.parametrize("form", ["f32", "bf16"])
@pytest.mark.parametrize("active", [1, 9, 32, 33, 76])
def test_causal_attention_active_length(form, active):
    """Rows >= active_len are neither evaluated nor written (the output buffer is poisoned first); the rows in front of it are bit for bit
    what the full-length call gives."""
    B, H, S = 3, 2, 77
    W = 64 * H
    g = torch.Generator(device=dev()).manual_seed(active)
    qkv = torch.randn(B * S, 3 * W, generator=g, device=dev())
    qkv_used, full = run_causal(form, qkv, B, H, S)
    poison = 12345.0
    o = torch.full((B * S, W), poison, dtype=full.dtype, device=dev())
    run_causal(form, qkv, B, H, S, active=active, o=o)
    o3, f3 = o.reshape(B, S, W), full.reshape(B, S, W)
    assert torch.equal(o3[:, :active], f3[:, :active])
    assert bool((o3[:, active:] == poison).all())


def test_causal_attention_argument_checks():
    l = lib()
    buf = torch.zeros(97 * 192, device=dev())
    assert l.rvlm_k_attn_causal_fwd_f32(buf.data_ptr(), buf.data_ptr(), 1, 1, 97, 0, st()) == L.RVLM_ERR_UNSUPPORTED
    assert l.rvlm_k_attn_causal_fwd_f32(buf.data_ptr(), buf.data_ptr(), 1, 1, 77, 78, st()) == L.RVLM_ERR_UNSUPPORTED
    assert l.rvlm_k_attn_causal_fwd_bf16(None, buf.data_ptr(), 1, 1, 77, 0, st()) == L.RVLM_ERR_ARG


# --------------------------------------------------------------------------------------------------------------------------
# token embedding
# --------------------------------------------------------------------------------------------------------------------------
def run_embed(tok, E, P, active=0):
    l = lib()
    N, ctx = tok.shape
    A = active or ctx
    x = torch.full((N * A, E.shape[1]), float("nan"), device=dev())
    eot = torch.full((N,), -1, dtype=torch.int32, device=dev())
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    L.check(l.rvlm_k_text_embed(tok.data_ptr(), E.data_ptr(), P.data_ptr(), x.data_ptr(), eot.data_ptr(), flags.data_ptr(), N, ctx, active,
                                E.shape[0], E.shape[1], st()))
    torch.cuda.synchronize()
    return x, eot, int(flags.item())


def test_token_embedding_bit_exact_and_eot():
    vocab, ctx, W = 1000, 77, 128
    g = torch.Generator(device=dev()).manual_seed(5)
    E = torch.randn(vocab, W, generator=g, device=dev())
    P = torch.randn(ctx, W, generator=g, device=dev())
    tok = torch.randint(0, vocab - 1, (9, ctx), generator=g, device=dev(), dtype=torch.int32)
    tok[0, 10] = vocab - 1
    tok[1, 76] = vocab - 1
    tok[2, 0] = vocab - 1
    tok[3, 5] = vocab - 1; tok[3, 50] = vocab - 1; tok[3, 70] = vocab - 1      # ties: the first occurrence (one of them in the second lane pass)
    tok[4, 64] = vocab - 1; tok[4, 65] = vocab - 1
    x, eot, flags = run_embed(tok, E, P)
    assert flags == 0
    assert torch.equal(x.reshape(9, ctx, W), E[tok.long()] + P)
    assert torch.equal(eot.long(), tok.argmax(-1)) and eot[3] == 5 and eot[4] == 64
    A = 71
    x, eot2, flags = run_embed(tok, E, P, active=A)
    assert torch.equal(x.reshape(9, A, W), (E[tok.long()] + P)[:, :A])
    assert torch.equal(eot2, eot) and flags == L.FLAG_EOT_ACTIVE                # prompt 1's EOT sits at 76 >= 71


def test_token_embedding_flags_bad_ids():
    vocab, ctx, W = 100, 77, 64
    E = torch.randn(vocab, W, device=dev())
    P = torch.randn(ctx, W, device=dev())
    for bad in (vocab, -1, 2 ** 30):
        tok = torch.zeros(2, ctx, dtype=torch.int32, device=dev())
        tok[:, 3] = vocab - 1
        tok[1, 2] = bad
        x, eot, flags = run_embed(tok, E, P)
        assert flags & L.FLAG_TOKEN_RANGE
        assert bool(torch.isfinite(x).all())           # reported, never dereferenced: the row is built from id 0


# --------------------------------------------------------------------------------------------------------------------------
# TextEngine against the oracle
# --------------------------------------------------------------------------------------------------------------------------
CFGS = {"tiny": T.TEXT_TINY, "b32": T.TEXT_B_32, "l14": T.TEXT_L_14}
# un-normalised embeddings, relative L2 against the fp32 CPU oracle.  fp32 / x3: the bars asked of the text tower (the vision tower
# measures 1.0e-6 / 3.8e-6; here: 0.6e-6 .. 1.8e-6 / 4.1e-6 .. 1.3e-5).  bf16: measured 5.0e-3 (tiny) .. 7.1e-3 (ViT-L/14 text) on seeded
# weights - 8 mantissa bits of storage through 12 blocks; the bar is about three times the largest measurement.
ENGINE_BARS = {"fp32": 1e-5, "x3": 2e-5, "bf16": 2e-2}


_ORACLE_CACHE = {}


def oracle(name, seed, tok, normalize=False):
    """The CPU oracle on the first active-length positions (equal to the full context: tests/test_oracle_text.py), cached across the
    precisions of a parametrised test."""
    key = (name, seed, normalize, tok.shape, int(tok.sum()))
    if key not in _ORACLE_CACHE:
        A = int(tok.argmax(-1).max()) + 1
        _ORACLE_CACHE[key] = T.text_forward(CFGS[name], T.init_text_weights(CFGS[name], seed=seed), tok[:, :A], normalize=normalize)
    return _ORACLE_CACHE[key]


def make_engine(name, precision, seed=1, max_batch=64):
    cfg = CFGS[name]
    w = T.init_text_weights(cfg, seed=seed)
    rcfg = R.TextConfig(cfg.vocab, cfg.context, cfg.width, cfg.layers, cfg.heads, cfg.out_dim, cfg.act)
    return cfg, w, R.TextEngine(rcfg, {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch)


def corner_prompts(cfg, n, seed):
    """Seeded prompts plus the corner cases: EOT at the last position, (SOT, EOT) alone, garbage non-zero ids behind EOT."""
    tok = T.random_prompts(n, cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    sot, eot = cfg.vocab - 2, cfg.vocab - 1
    tok[1] = torch.randint(1, sot, (cfg.context,), generator=g); tok[1, 0] = sot; tok[1, cfg.context - 1] = eot
    tok[2] = 0; tok[2, 0] = sot; tok[2, 1] = eot
    tok[3] = torch.randint(1, sot, (cfg.context,), generator=g); tok[3, 0] = sot; tok[3, 11] = eot
    return tok


@pytest.mark.parametrize("precision", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("name,n", [("tiny", 7), ("b32", 40), ("l14", 40)])
def test_text_engine_matches_oracle(name, n, precision):
    """tiny: every linear on the fp32 tiles (x3) / the 128x128 kernel (bf16); b32 / l14 at 40 x 77 = 3080 rows: the persistent GEMM."""
    cfg, w, eng = make_engine(name, precision)
    tok = corner_prompts(cfg, n, seed=2)
    want = oracle(name, 1, tok)
    got = eng.encode(tok)                               # active length 77 (prompt 1)
    err = rel_l2(got, want)
    short = T.random_prompts(n, cfg, seed=3)            # "a photo of a {}"-sized prompts: active length ~20
    err_short = rel_l2(eng.encode(short), oracle(name, 1, short))
    gotn = eng.encode(tok, normalize=True)
    record(f"text_engine_{name}_{precision}", err=err, err_short=err_short)
    eng.close()
    assert err < ENGINE_BARS[precision] and err_short < ENGINE_BARS[precision], (err, err_short)
    assert rel_l2(gotn, F.normalize(want, dim=-1)) < ENGINE_BARS[precision]
    assert float((gotn.norm(dim=-1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("precision", ["fp32", "x3", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "b32"])
def test_text_engine_causality_active_length_and_chunking(name, precision):
    """Every kernel of the tower treats a row independently of how many rows there are (LayerNorm, a query row of the causal
    attention, the GEMMs' k-ordered accumulation - the engine passes them no split-K scratch), so neither the active length nor the
    chunking changes a bit of a prompt - measured bit-identical on all three precisions.  The one exception is the ROUTING of x3:
    a call of fewer than 256 rows runs its linears on the fp32 tiles instead of the split-bf16 product (the vision engine's rule),
    and the two differ by the x3 error itself (~1e-5); the x3 comparisons here therefore stay on one side of that threshold, and the
    few-row calls at the end are held to the x3 bar instead."""
    cfg, w, eng = make_engine(name, precision, max_batch=20)
    tok = T.random_prompts(40, cfg, seed=7)
    A = R.TextEngine.active_length(tok)
    assert 20 * A >= 256
    e0 = eng.encode(tok)                                # 2 chunks of 20 prompts, automatic active length
    # ids behind EOT (below the EOT id) cannot reach the EOT row: bit-identical
    tok2 = tok.clone()
    g = torch.Generator().manual_seed(8)
    for i in range(tok.shape[0]):
        k = int(tok[i].argmax())
        tok2[i, k + 1:] = torch.randint(1, cfg.vocab - 2, (cfg.context - k - 1,), generator=g)
    assert torch.equal(eng.encode(tok2), e0)
    # full context against the automatic active length
    e_full = eng.encode(tok, active_len=0)
    record(f"text_active_len_{name}_{precision}", rel_l2_full_vs_active=rel_l2(e_full, e0))
    assert torch.equal(e_full, e0)
    assert torch.equal(eng.encode(tok2, active_len=0), e0)
    eng.close()
    # chunking over max_batch equals one call
    cfg, w, big = make_engine(name, precision, max_batch=64)
    e_one = big.encode(tok)
    record(f"text_chunking_{name}_{precision}", rel_l2_chunked_vs_one=rel_l2(e_one, e0))
    assert torch.equal(e_one, e0)
    for n in (1, 7):                                    # 20 / 140 rows: x3 routes these to the fp32 tiles
        d = rel_l2(big.encode(tok[:n], active_len=A), e0[:n])
        assert d <= (ENGINE_BARS["x3"] if precision == "x3" else 0.0), d
    big.close()


def test_text_engine_n1000_and_input_forms():
    cfg, w, eng = make_engine("tiny", "x3", max_batch=256)
    tok = T.random_prompts(1000, cfg, seed=9)           # 1000 = 3 x 256 + 232
    e = eng.encode(tok)
    assert e.shape == (1000, cfg.out_dim)
    assert rel_l2(e, oracle("tiny", 1, tok)) < ENGINE_BARS["x3"]
    for t in (tok.to(torch.int32), tok.to(dev()), tok.to(dev()).to(torch.int32)):
        assert torch.equal(eng.encode(t), e)
    m = R.ClipTextModel(eng)
    assert torch.equal(m.encode_text(tok[:5]), eng.encode(tok[:5]))
    assert torch.equal(m.encode_text(tok[:5], normalize=True), eng.encode(tok[:5], normalize=True))
    # errors, not faults
    bad = tok[:4].clone(); bad[2, 1] = cfg.vocab
    with pytest.raises(ValueError, match="token id"):
        eng.encode(bad)
    bad32 = tok[:4].to(torch.int32); bad32[2, 1] = -5
    with pytest.raises(ValueError, match="token id"):
        eng.encode(bad32)
    with pytest.raises(ValueError, match="active_len"):
        eng.encode(tok[:4], active_len=3)
    with pytest.raises(ValueError):
        eng.encode(tok[:4, :50])
    with pytest.raises(TypeError):
        eng.encode(tok[:4].float())
    assert rel_l2(eng.encode(tok[:5]), e[:5]) < ENGINE_BARS["x3"]      # the handle is still usable (5 prompts: the fp32-tile routing)
    assert eng.workspace_bytes > 0
    eng.close()


def test_text_engine_create_refuses_oversized_x3_batch():
    cfg = T.TEXT_L_14
    rcfg = R.TextConfig(cfg.vocab, cfg.context, cfg.width, 1, cfg.heads, cfg.out_dim)
    sd = R.random_text_state_dict(rcfg, seed=0, device=dev())
    with pytest.raises(NotImplementedError, match="max_batch"):
        R.TextEngine(rcfg, sd, precision="x3", max_batch=1600)
    with pytest.raises(ValueError, match="head_dim"):
        R.TextEngine(R.TextConfig(cfg.vocab, 77, 768, 1, 8, 768), sd, precision="fp32", max_batch=8)


# --------------------------------------------------------------------------------------------------------------------------
# end to end: the zero-shot / TeCoA head
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "x3", "bf16"])
def test_zero_shot_head_end_to_end(precision):
    """T from get_text_embeddings (1000 seeded prompts, ViT-B/32 text tower) is column-normalised, matches the oracle's T, and gives
    the oracle's arg-max class through ClassificationModel and through the fused CE loss on seeded images."""
    cfg, w, eng = make_engine("b32", precision, seed=4, max_batch=500)
    model = R.ClipTextModel(eng)
    tok = T.random_prompts(1000, cfg, seed=10)
    T_got = R.get_text_embeddings(model, tok)
    T_ref = oracle("b32", 4, tok, normalize=True).T.contiguous()
    assert T_got.shape == (cfg.out_dim, 1000)
    assert float((T_got.norm(dim=0) - 1).abs().max()) < 1e-6
    err_T = rel_l2(T_got, T_ref)
    # a tiny vision tower into the same embedding space
    vcfg = R.VitConfig(32, 8, 64, 2, 1, cfg.out_dim)
    veng = R.VitEngine(vcfg, R.random_state_dict(vcfg, seed=3, device=dev()), precision="fp32", max_batch=64)
    x = torch.rand(64, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(dev())
    with torch.no_grad():
        lg = R.ClassificationModel(veng, T_got)(x)
        lr = R.ClassificationModel(veng, T_ref.to(dev()))(x)
        emb = R.ClipVisionModel(veng)(x, True)
        y = lr.argmax(-1)
        ce_g = R.compute_loss("ce", emb, y, None, 100., T_got, reduction="none")
        ce_r = R.compute_loss("ce", emb, y, None, 100., T_ref.to(dev()), reduction="none")
    dlogit = float((lg - lr).abs().max())
    top2 = lr.topk(2, dim=-1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    record(f"text_head_e2e_{precision}", rel_l2_T=err_T, max_logit_diff_at_100x=dlogit, min_top2_margin=margin,
           max_ce_diff=float((ce_g - ce_r).abs().max()))
    assert err_T < ENGINE_BARS[precision]
    decided = (top2[:, 0] - top2[:, 1]) > 2 * dlogit     # (an image whose two best classes are closer than the head's error is a tie)
    assert int(decided.sum()) >= 48
    assert torch.equal(lg.argmax(-1)[decided], lr.argmax(-1)[decided])
    assert float((ce_g - ce_r).abs().max()) < 4 * dlogit + 1e-4
    # the template ensemble: 20 classes x 80 templates
    tok_e = T.random_prompts(20 * 80, cfg, seed=11).reshape(20, 80, cfg.context)
    T_ens = R.get_text_embeddings_ensemble(model, tok_e)
    ref = F.normalize(oracle("b32", 4, tok_e.reshape(-1, cfg.context)), dim=-1).reshape(20, 80, -1).mean(1)
    ref = (ref / ref.norm(dim=-1, keepdim=True)).T
    err_ens = rel_l2(T_ens, ref)
    record(f"text_head_ensemble_{precision}", rel_l2_T=err_ens)
    assert T_ens.shape == (cfg.out_dim, 20) and err_ens < ENGINE_BARS[precision]
    veng.close(); eng.close()
