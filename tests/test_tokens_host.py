"""Token-level door of the encoder (RVLM_HAS_TOKENS), host side: the entries are declared in include/rvlm.h, exported by the
library and bound in robustvlm_amd/_lib.py; the ABI number has not moved; the Python wrappers check their arguments and raise the
package's own error where there is no device."""
import os
import re
import types

import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rvlm_vit_forward_tokens", "rvlm_vit_backward_input_tokens", "rvlm_tokens_l2_loss_grad",
           "rvlm_vit_tokens_fwd_inputgrad", "rvlm_pgd_run_tokens"]


def _header():
    return open(os.path.join(ROOT, "include", "rvlm.h")).read()


def test_entries_are_declared_exported_and_bound():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/rvlm.h"
        assert name in L.EXPORTED_SYMBOLS, f"{name} is not bound in robustvlm_amd/_lib.py"
        fn = getattr(lib, name)
        assert fn.restype is not None and fn.argtypes, name
    # every declaration names the reference lines it serves
    block = txt[txt.index("Token-level outputs and their input gradient"):txt.index("int rvlm_pgd_run_tokens")]
    for where in ("clip_encoder.py:55-65", "factory.py:41", "flamingo.py:217", "vlm_eval/attacks/pgd.py"):
        assert where in block, where
    # the kernel-level hook of the seed kernel
    assert "rvlm_k_tokens_seed" in open(os.path.join(ROOT, "include", "rvlm_kernels.h")).read()
    assert "rvlm_k_tokens_seed" in L.EXPORTED_SYMBOLS


def test_abi_number_stays_and_the_feature_macro_announces_the_entries():
    txt = _header()
    assert re.search(r"#define\s+RVLM_VERSION\s+109\b", txt)
    assert re.search(r"#define\s+RVLM_HAS_TOKENS\s+1\b", txt)
    if os.path.exists(L.LIB_PATH):
        assert L.load().rvlm_version() == 109
    assert re.search(r"RVLM_FLAG_TOKENS_NONFINITE\s*=\s*128\b", txt) and L.FLAG_TOKENS_NONFINITE == 128
    assert re.search(r"RVLM_TOKENS_ALL\s*=\s*0\s*,\s*RVLM_TOKENS_PATCH\s*=\s*1", txt)
    assert (L.TOKENS_ALL, L.TOKENS_PATCH) == (0, 1)
    # no existing struct changed: the ctypes mirrors still have the fields they had
    assert [f for f, _ in L.LossSpecC._fields_] == ["loss_kind", "reduction", "output_normalize", "n_classes", "logit_scale", "ref",
                                                    "targets", "y_target"]
    assert [f for f, _ in L.VitConfigC._fields_][-1] == "trainable" and len(L.VitConfigC._fields_) == 12


def test_token_kernels_are_part_of_the_library_build():
    mk = open(os.path.join(ROOT, "robustvlm_amd", "csrc", "Makefile")).read()
    assert "token_kernels.hip" in mk
    src = open(os.path.join(ROOT, "robustvlm_amd", "csrc", "token_kernels.hip")).read()
    assert "atomicAdd" not in src, "the token loss sums in a fixed order: no float atomics"


def _fake_engine(layers=3, precision="fp32"):
    """A VitEngine without a device behind it: enough for the wrappers' argument checks."""
    eng = object.__new__(R.VitEngine)
    eng.cfg = R.VitConfig(96, 16, 128, layers, 2, 48)
    eng.mean, eng.std = tuple(R.CLIP_MEAN), tuple(R.CLIP_STD)
    eng.precision = precision
    eng.mixed = "+" in precision
    eng.max_batch = 4
    eng.input_size = (96, 96)
    eng.device = torch.device("cpu")
    eng.generation = 0
    eng._h = None
    eng._h32 = None
    return eng


def test_clip_vision_tower_argument_checks():
    eng = _fake_engine()
    with pytest.raises(TypeError):
        R.ClipVisionTower(object())
    with pytest.raises(ValueError, match="select_layer"):
        R.ClipVisionTower(eng, select_layer=-3)
    with pytest.raises(ValueError, match="Unexpected select feature"):
        R.ClipVisionTower(eng, select_feature="cls")
    with pytest.raises(ValueError, match="two blocks"):
        R.ClipVisionTower(_fake_engine(layers=1), select_layer=-2)
    with pytest.raises(ValueError, match="plain precisions"):
        R.ClipVisionTower(_fake_engine(precision="bf16+x3fwd-first"))
    with pytest.raises(ValueError, match="normalize constants"):
        R.ClipVisionTower(eng, normalize=types.SimpleNamespace(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)))
    llava = R.ClipVisionTower(eng, normalize=types.SimpleNamespace(mean=R.CLIP_MEAN, std=R.CLIP_STD))
    assert (llava.select_layer, llava.select_feature, llava.depth, llava.ln_post) == (-2, "patch", 2, False)
    flamingo = R.ClipVisionTower(eng, select_layer=-1, select_feature="cls_patch")
    assert flamingo.depth == 3 and flamingo.hidden_size == 128 and flamingo.num_patches == 36
    t = torch.zeros(2, 37, 128)
    assert llava.feature_select(t).shape == (2, 36, 128) and flamingo.feature_select(t).shape == (2, 37, 128)
    with pytest.raises(ValueError, match="output_normalize"):
        llava(torch.zeros(2, 3, 96, 96), output_normalize=True)


def test_depth_convention():
    eng = _fake_engine(layers=3)
    assert [eng._depth(d) for d in (None, -1, -2, 1, 2, 3)] == [3, 3, 2, 1, 2, 3]
    assert eng.n_tokens == 37
    for bad in (0 - 4, 4):
        with pytest.raises(ValueError, match="depth"):
            eng._depth(bad)


def test_without_a_device_the_wrappers_raise_the_package_error():
    eng = _fake_engine()
    x = torch.zeros(2, 3, 96, 96)
    with pytest.raises(L.RvlmError, match="CUDA"):
        eng.forward_tokens(x)
    with pytest.raises(L.RvlmError, match="CUDA"):
        eng.backward_input_tokens(torch.zeros(2, 37, 128))
    with pytest.raises(L.RvlmError, match="CUDA"):
        eng.tokens_fwd_inputgrad(x, None, torch.zeros(2, 37, 128))
    with pytest.raises(L.RvlmError, match="CUDA"):
        eng.pgd_run_tokens(x, None, torch.zeros(2, 36, 128), 4 / 255, 2, 1 / 255, 0.9, "max", select="patch")
    with pytest.raises(L.RvlmError, match="CUDA"):
        R.ClipVisionTower(eng)(x)
    with pytest.raises(L.RvlmError, match="CUDA"):
        R.pgd(R.ClipVisionTower(eng), R.ComputeLossWrapper(torch.zeros(2, 36, 128), None, "mean", "l2"), x, None, "linf", 4 / 255, 2,
              1 / 255, False)
    # the handoff precisions refuse token passes instead of running on mixed tensors
    with pytest.raises(ValueError, match="plain precisions"):
        _fake_engine(precision="bf16+x3fwd-first").forward_tokens(x)
