"""Host-side checks of the text tower's Python surface and C ABI declarations (no GPU), in the style of tests/test_cabi_and_host.py."""
import os
import re

import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.config import TEXT_CONFIGS, CONFIGS, TextConfig, text_state_dict_shapes
from robustvlm_amd.checkpoint import load_text_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(rvlm_[a-z0-9_]+)\s*\(", txt))


def test_text_entry_points_are_declared_exported_and_bound():
    """The text tower's additions to the C ABI: declared in include/, exported by librvlm.so, bound in _lib, and announced by
    RVLM_HAS_TEXT (they are additions only: RVLM_VERSION does not move, tests/test_cabi_and_host.py keeps checking it)."""
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    top, kern = _declared("rvlm.h"), _declared("rvlm_kernels.h")
    for sym in ("rvlm_text_create", "rvlm_text_destroy", "rvlm_text_workspace_bytes", "rvlm_text_encode"):
        assert sym in top and sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    for sym in ("rvlm_k_attn_causal_fwd_bf16", "rvlm_k_attn_causal_fwd_f32", "rvlm_k_text_embed"):
        assert sym in kern and sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    hdr = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    assert re.search(r"#define\s+RVLM_HAS_TEXT\s+1", hdr)
    assert lib.rvlm_version() == int(re.search(r"#define\s+RVLM_VERSION\s+(\d+)", hdr).group(1))


def test_text_configs_and_shapes():
    assert set(TEXT_CONFIGS) == set(CONFIGS)
    l14, b32 = TEXT_CONFIGS["ViT-L-14"], TEXT_CONFIGS["ViT-B-32"]
    assert (l14.vocab, l14.context, l14.width, l14.layers, l14.heads, l14.out_dim) == (49408, 77, 768, 12, 12, 768)
    assert (b32.width, b32.layers, b32.heads, b32.out_dim) == (512, 12, 8, 512)
    for name, c in TEXT_CONFIGS.items():
        assert c.width == 64 * c.heads and c.out_dim == CONFIGS[name].out_dim      # the two towers meet in one embedding space
    sh = text_state_dict_shapes(l14)
    assert len(sh) == 5 + 12 * 12
    assert sh["token_embedding.weight"] == (49408, 768) and sh["positional_embedding"] == (77, 768)
    assert sh["text_projection"] == (768, 768) and sh["ln_final.bias"] == (768,)
    assert sh["transformer.resblocks.11.mlp.c_fc.weight"] == (3072, 768)
    assert sh["transformer.resblocks.0.attn.in_proj_weight"] == (2304, 768)
    tiny = TextConfig(64, 77, 64, 1, 1, 16)
    sd = R.random_text_state_dict(tiny, seed=1, device="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == text_state_dict_shapes(tiny)
    sd2 = R.random_text_state_dict(tiny, seed=1, device="cpu")
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    # the C structs mirror include/rvlm.h field for field
    assert [f for f, _ in L.TextConfigC._fields_] == ["vocab", "context", "width", "layers", "heads", "out_dim", "act", "precision", "max_batch"]
    assert [f for f, _ in L.TextWeightsC._fields_] == L.TEXT_TOP_FIELDS + ["blocks_host"]
    hdr = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} rvlm_text_weights;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*\s*([a-z_]+);", body) == L.TEXT_TOP_FIELDS + ["blocks_host"]
    assert (L.FLAG_TOKEN_RANGE, L.FLAG_EOT_ACTIVE) == (16, 32)
    assert "RVLM_FLAG_TOKEN_RANGE = 16" in hdr and "RVLM_FLAG_EOT_ACTIVE = 32" in hdr


def test_load_text_state_dict_filters_and_validates(tmp_path):
    tiny = TextConfig(64, 77, 64, 1, 1, 16)
    text = R.random_text_state_dict(tiny, seed=2, device="cpu")
    full = dict(text)
    full["visual.conv1.weight"] = torch.zeros(64, 3, 8, 8)
    full["visual.proj"] = torch.zeros(64, 16)
    full["logit_scale"] = torch.tensor(4.6)
    full["attn_mask"] = torch.zeros(77, 77)
    sd = load_text_state_dict(full, tiny)
    assert set(sd) == set(text) and all(sd[k] is text[k] for k in text)
    p = tmp_path / "clip.pt"
    torch.save(full, p)
    sd = load_text_state_dict(str(p), tiny)
    assert set(sd) == set(text) and all(torch.equal(sd[k], text[k]) for k in text)
    assert set(load_text_state_dict({"state_dict": full})) == set(text)
    bad = dict(full); del bad["ln_final.weight"]
    with pytest.raises(KeyError, match="missing"):
        load_text_state_dict(bad, tiny)
    bad = dict(full); bad["text_projection"] = torch.zeros(64, 32)
    with pytest.raises(ValueError, match="text_projection"):
        load_text_state_dict(bad, tiny)
    bad = dict(full); bad["transformer.resblocks.1.ln_1.weight"] = torch.zeros(64)
    with pytest.raises(KeyError, match="unexpected"):
        load_text_state_dict(bad, tiny)


def test_text_engine_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    tiny = TextConfig(64, 77, 64, 1, 1, 16)
    with pytest.raises(L.RvlmError, match="no CPU fallback"):
        R.TextEngine(tiny, R.random_text_state_dict(tiny, device="cpu"))
    with pytest.raises(ValueError, match="precision"):
        R.TextEngine(tiny, {}, precision="fp16")
    with pytest.raises(TypeError):
        R.ClipTextModel(object())
