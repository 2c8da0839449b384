"""CPU oracle: CLIP text tower (open_clip 2.19.0 ``CLIP.encode_text``) in plain torch fp32.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Restates, op by op, what the reference calls on the frozen ``model_orig`` to
build the zero-shot / TeCoA head (train/adversarial_training_clip.py:166-170, CLIP_eval/eval_utils.py:74-78,
CLIP_eval/clip_robustbench.py:216-222); the third-party
source is pinned at requirements.txt:91:

    x = token_embedding(text) + positional_embedding
    L x { x += out_proj(SDPA(in_proj(ln_1(x)), attn_mask)) ; x += c_proj(act(c_fc(ln_2(x)))) }     (the vision tower's block)
    x = ln_final(x) ; x = x[arange(N), text.argmax(dim=-1)] @ text_projection ; F.normalize(x, dim=-1) iff normalize

with attn_mask = build_attention_mask(): additive, -inf strictly above the diagonal (causal).  ln_final acts per row, so
applying it to the pooled rows only is the same arithmetic.  Weights are keyed like the non-``visual.`` part of
``CLIP.state_dict()``.

Pinned by tests/golden/text_hf_*.npz: outputs of the independent HF ``transformers`` CLIPTextModelWithProjection on the same
weights (tests/golden/make_golden_text.py).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from .vit_ref import quick_gelu


@dataclass
class TextConfig:
    vocab: int = 49408
    context: int = 77
    width: int = 768
    layers: int = 12
    heads: int = 12
    out_dim: int = 768
    act: str = "quick_gelu"

    @property
    def mlp(self) -> int:
        return 4 * self.width


TEXT_L_14 = TextConfig(49408, 77, 768, 12, 12, 768)
TEXT_B_32 = TextConfig(49408, 77, 512, 12, 8, 512)
TEXT_TINY = TextConfig(512, 77, 128, 2, 2, 48)      # head_dim is always 64


def param_shapes(cfg: TextConfig) -> dict:
    W = cfg.width
    shapes = {"token_embedding.weight": (cfg.vocab, W), "positional_embedding": (cfg.context, W),
              "ln_final.weight": (W,), "ln_final.bias": (W,), "text_projection": (W, cfg.out_dim)}
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        shapes.update({p + "ln_1.weight": (W,), p + "ln_1.bias": (W,),
                       p + "attn.in_proj_weight": (3 * W, W), p + "attn.in_proj_bias": (3 * W,),
                       p + "attn.out_proj.weight": (W, W), p + "attn.out_proj.bias": (W,),
                       p + "ln_2.weight": (W,), p + "ln_2.bias": (W,),
                       p + "mlp.c_fc.weight": (cfg.mlp, W), p + "mlp.c_fc.bias": (cfg.mlp,),
                       p + "mlp.c_proj.weight": (W, cfg.mlp), p + "mlp.c_proj.bias": (W,)})
    return shapes


def init_text_weights(cfg: TextConfig, seed: int = 0, ln_jitter: float = 0.1) -> dict:
    """Seeded random weights at open_clip's initialisation scales (CLIP.init_parameters: token embedding std 0.02, positional
    embedding std 0.01, text_projection std width^-0.5); LayerNorm affine parameters jittered away from (1, 0)."""
    g = torch.Generator().manual_seed(seed)
    W, L = cfg.width, cfg.layers
    attn_std, proj_std, fc_std = W ** -0.5, (W ** -0.5) * ((2 * L) ** -0.5), (2 * W) ** -0.5
    out = {}
    for k, shp in param_shapes(cfg).items():
        r = torch.randn(shp, generator=g)
        if "ln_" in k and k.endswith(".weight"):
            t = 1.0 + ln_jitter * r
        elif "ln_" in k:
            t = ln_jitter * r
        elif k.endswith("bias"):
            t = 0.02 * r
        elif k == "token_embedding.weight":
            t = 0.02 * r
        elif k == "positional_embedding":
            t = 0.01 * r
        elif k.endswith("out_proj.weight") or k.endswith("c_proj.weight"):
            t = r * proj_std
        elif k.endswith("c_fc.weight"):
            t = r * fc_std
        else:      # in_proj_weight, text_projection
            t = r * attn_std
        out[k] = t.float().contiguous()
    return out


def build_attention_mask(context: int) -> torch.Tensor:
    """open_clip CLIP.build_attention_mask: additive mask, -inf strictly above the diagonal."""
    mask = torch.empty(context, context)
    mask.fill_(float("-inf"))
    mask.triu_(1)
    return mask


def text_forward(cfg: TextConfig, w: dict, text: torch.Tensor, normalize: bool = False, dtype=torch.float32) -> torch.Tensor:
    """``CLIP.encode_text(text, normalize)``: text [N, context] integer ids -> [N, out_dim]."""
    W, H = cfg.width, cfg.heads
    dh = W // H
    act = quick_gelu if cfg.act == "quick_gelu" else F.gelu
    w = {k: v.to(dtype) for k, v in w.items()}
    text = text.long()
    N, S = text.shape
    t = w["token_embedding.weight"][text] + w["positional_embedding"][:S]
    mask = build_attention_mask(S).to(dtype)
    for i in range(cfg.layers):
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(t, (W,), w[p + "ln_1.weight"], w[p + "ln_1.bias"], 1e-5)
        qkv = F.linear(h, w[p + "attn.in_proj_weight"], w[p + "attn.in_proj_bias"])
        q, k, v = (u.reshape(N, S, H, dh).transpose(1, 2) for u in qkv.split(W, dim=-1))
        s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(dh)) + mask
        a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(N, S, W)
        t = t + F.linear(a, w[p + "attn.out_proj.weight"], w[p + "attn.out_proj.bias"])
        h = F.layer_norm(t, (W,), w[p + "ln_2.weight"], w[p + "ln_2.bias"], 1e-5)
        h = act(F.linear(h, w[p + "mlp.c_fc.weight"], w[p + "mlp.c_fc.bias"]))
        t = t + F.linear(h, w[p + "mlp.c_proj.weight"], w[p + "mlp.c_proj.bias"])
    t = F.layer_norm(t, (W,), w["ln_final.weight"], w["ln_final.bias"], 1e-5)
    out = t[torch.arange(N), text.argmax(dim=-1)] @ w["text_projection"]
    return F.normalize(out, dim=-1) if normalize else out


def random_prompts(n: int, cfg: TextConfig, seed: int = 0, min_len: int = 4, max_len: int = 20) -> torch.Tensor:
    """Seeded stand-ins for ``open_clip.tokenize`` output (no BPE vocabulary offline): [SOT, ids ..., EOT, 0 ...] with SOT =
    vocab - 2, EOT = vocab - 1 (49406 / 49407 at the CLIP vocabulary) as the largest id, prompt lengths min_len..max_len."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(n, cfg.context, dtype=torch.int64)
    lens = torch.randint(min_len, max_len + 1, (n,), generator=g)
    body = torch.randint(1, cfg.vocab - 2, (n, cfg.context), generator=g)
    for i in range(n):
        ln = int(lens[i])
        tok[i, 0] = cfg.vocab - 2
        tok[i, 1:ln - 1] = body[i, 1:ln - 1]
        tok[i, ln - 1] = cfg.vocab - 1
    return tok


def hf_to_openclip_text(sd: dict, cfg: TextConfig) -> dict:
    """HF CLIPTextModelWithProjection state_dict -> open_clip text keys."""
    o = {"token_embedding.weight": sd["text_model.embeddings.token_embedding.weight"],
         "positional_embedding": sd["text_model.embeddings.position_embedding.weight"],
         "ln_final.weight": sd["text_model.final_layer_norm.weight"], "ln_final.bias": sd["text_model.final_layer_norm.bias"],
         "text_projection": sd["text_projection.weight"].t()}
    for i in range(cfg.layers):
        s, p = f"text_model.encoder.layers.{i}.", f"transformer.resblocks.{i}."
        o[p + "ln_1.weight"], o[p + "ln_1.bias"] = sd[s + "layer_norm1.weight"], sd[s + "layer_norm1.bias"]
        o[p + "ln_2.weight"], o[p + "ln_2.bias"] = sd[s + "layer_norm2.weight"], sd[s + "layer_norm2.bias"]
        o[p + "attn.in_proj_weight"] = torch.cat([sd[s + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        o[p + "attn.in_proj_bias"] = torch.cat([sd[s + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
        o[p + "attn.out_proj.weight"], o[p + "attn.out_proj.bias"] = sd[s + "self_attn.out_proj.weight"], sd[s + "self_attn.out_proj.bias"]
        o[p + "mlp.c_fc.weight"], o[p + "mlp.c_fc.bias"] = sd[s + "mlp.fc1.weight"], sd[s + "mlp.fc1.bias"]
        o[p + "mlp.c_proj.weight"], o[p + "mlp.c_proj.bias"] = sd[s + "mlp.fc2.weight"], sd[s + "mlp.fc2.bias"]
    return {k: v.detach().float().contiguous().clone() for k, v in o.items()}
