"""Golden vectors of the text tower: outputs of HF ``transformers`` CLIPTextModelWithProjection (random-init from a
CLIPTextConfig, the oracle's seeded weights loaded into it) for tests/test_oracle_text.py - the independent pin of
oracle/text_ref.py, the way vit_hf_*.npz pins the vision tower.  Only token ids and outputs are stored: the test regenerates
the weights from the seed and checks their digest.

    python tests/golden/make_golden_text.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from oracle import text_ref as T  # noqa: E402
from tests.helpers import weights_digest  # noqa: E402


def openclip_to_hf_text(w, cfg):
    W = cfg.width
    sd = {"text_model.embeddings.token_embedding.weight": w["token_embedding.weight"],
          "text_model.embeddings.position_embedding.weight": w["positional_embedding"],
          "text_model.final_layer_norm.weight": w["ln_final.weight"], "text_model.final_layer_norm.bias": w["ln_final.bias"],
          "text_projection.weight": w["text_projection"].t().contiguous()}
    for i in range(cfg.layers):
        s, p = f"text_model.encoder.layers.{i}.", f"transformer.resblocks.{i}."
        sd[s + "layer_norm1.weight"], sd[s + "layer_norm1.bias"] = w[p + "ln_1.weight"], w[p + "ln_1.bias"]
        sd[s + "layer_norm2.weight"], sd[s + "layer_norm2.bias"] = w[p + "ln_2.weight"], w[p + "ln_2.bias"]
        for j, n in enumerate("qkv"):
            sd[s + f"self_attn.{n}_proj.weight"] = w[p + "attn.in_proj_weight"][j * W:(j + 1) * W]
            sd[s + f"self_attn.{n}_proj.bias"] = w[p + "attn.in_proj_bias"][j * W:(j + 1) * W]
        sd[s + "self_attn.out_proj.weight"], sd[s + "self_attn.out_proj.bias"] = w[p + "attn.out_proj.weight"], w[p + "attn.out_proj.bias"]
        sd[s + "mlp.fc1.weight"], sd[s + "mlp.fc1.bias"] = w[p + "mlp.c_fc.weight"], w[p + "mlp.c_fc.bias"]
        sd[s + "mlp.fc2.weight"], sd[s + "mlp.fc2.bias"] = w[p + "mlp.c_proj.weight"], w[p + "mlp.c_proj.bias"]
    return sd


def token_batch(cfg, seed):
    """A short prompt, EOT at position 76, a prompt of length 2 (SOT, EOT), garbage non-zero ids behind EOT, plus seeded prompts."""
    tok = T.random_prompts(6, cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    sot, eot = cfg.vocab - 2, cfg.vocab - 1
    tok[0] = 0; tok[0, 0] = sot; tok[0, 1:6] = torch.randint(1, sot, (5,), generator=g); tok[0, 6] = eot       # short prompt
    tok[1] = torch.randint(1, sot, (cfg.context,), generator=g); tok[1, 0] = sot; tok[1, cfg.context - 1] = eot  # EOT at 76
    tok[2] = 0; tok[2, 0] = sot; tok[2, 1] = eot                                                              # length 2
    tok[3] = torch.randint(1, sot, (cfg.context,), generator=g); tok[3, 0] = sot; tok[3, 11] = eot              # garbage behind EOT
    return tok


def main():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    for name, cfg, seed in (("tiny", T.TEXT_TINY, 11), ("b32", T.TEXT_B_32, 12)):
        w = T.init_text_weights(cfg, seed=seed)
        hcfg = CLIPTextConfig(vocab_size=cfg.vocab, hidden_size=cfg.width, intermediate_size=cfg.mlp, projection_dim=cfg.out_dim,
                              num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, max_position_embeddings=cfg.context,
                              hidden_act=cfg.act, layer_norm_eps=1e-5, pad_token_id=0, bos_token_id=cfg.vocab - 2,
                              eos_token_id=cfg.vocab - 1, attn_implementation="eager")
        hf = CLIPTextModelWithProjection(hcfg).eval()
        missing = hf.load_state_dict(openclip_to_hf_text(w, cfg), strict=False)
        assert not missing.unexpected_keys, missing
        assert all("position_ids" in k for k in missing.missing_keys), missing
        tok = token_batch(cfg, seed)
        with torch.no_grad():
            emb = hf(input_ids=tok).text_embeds
        p = os.path.join(HERE, f"text_hf_{name}.npz")
        np.savez_compressed(p, tokens=tok.numpy().astype(np.int32), emb=emb.numpy(), weights_seed=np.int64(seed),
                            weights_sha256=np.array(weights_digest(w)),
                            cfg=np.array([cfg.vocab, cfg.context, cfg.width, cfg.layers, cfg.heads, cfg.out_dim]), act=np.array(cfg.act))
        print(f"wrote {os.path.basename(p)}: {os.path.getsize(p) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
