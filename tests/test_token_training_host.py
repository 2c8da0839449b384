"""Token-level training (RVLM_HAS_TOKEN_TRAINING), host side: the feature macro, the three new entries (declared in include/rvlm.h,
exported by the library, bound in robustvlm_amd/_lib.py), and the trainer's refusals, which fire before any device work."""
import os
import re

import pytest

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.trainer import AdversarialTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rvlm_vit_backward_params_tokens", "rvlm_vit_backward_params_tokens_stages", "rvlm_tokens_cosine"]


def _header():
    return open(os.path.join(ROOT, "include", "rvlm.h")).read()


def test_feature_macro_is_announced_and_the_abi_number_stays():
    txt = _header()
    assert re.search(r"#define\s+RVLM_HAS_TOKEN_TRAINING\s+1\b", txt)
    assert re.search(r"#define\s+RVLM_VERSION\s+109\b", txt)


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_exported_and_bound(name):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/rvlm.h"
    assert name in L.EXPORTED_SYMBOLS, f"{name} is not bound in robustvlm_amd/_lib.py"
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    fn = getattr(L.load(), name)
    assert fn.restype is not None and fn.argtypes, name


def test_signatures_of_the_bindings():
    import ctypes as C
    args = L._SIGS["rvlm_vit_backward_params_tokens"][1]
    assert len(args) == 7 and args[4] == C.POINTER(L.VitWeightsC)
    staged = L._SIGS["rvlm_vit_backward_params_tokens_stages"][1]
    assert len(staged) == 9 and staged[:6] == args[:6] and staged[6:8] == [C.c_int, C.c_int]
    assert len(L._SIGS["rvlm_tokens_cosine"][1]) == 10


def test_cosine_kernel_sums_in_a_fixed_order():
    src = open(os.path.join(ROOT, "robustvlm_amd", "csrc", "token_kernels.hip")).read()
    assert "tokens_cosine_kernel" in src
    assert "atomicAdd" not in src, "the token metric sums in a fixed order: no float atomics"


def test_new_keyword_arguments_go_at_the_end_of_the_signature():
    import inspect
    names = list(inspect.signature(AdversarialTrainer.__init__).parameters)
    assert names[-2:] == ["token_depth", "token_select"]
    p = inspect.signature(AdversarialTrainer.__init__).parameters
    assert p["token_depth"].default == -2 and p["token_select"].default == "patch"
    e = inspect.signature(R.VitEngine.backward_params_tokens).parameters
    assert list(e) == ["self", "d_tokens", "grads", "d_emb", "accumulate", "stages"]


CFG = R.VitConfig(96, 16, 128, 3, 2, 48)
OK = dict(loss="l2-tokens", inner_loss="l2-tokens", loss_clean="l2-tokens")


@pytest.mark.parametrize("kw,match", [
    (dict(OK, inner_loss="l2"), "inner_loss"),                           # another inner loss while attacking
    (dict(OK, loss_clean="l2", clean_weight=0.3), "loss_clean"),         # another clean loss that would be used
    (dict(OK, output_normalize=True), "output_normalize"),
    (dict(OK, token_depth=0), "token_depth"),
    (dict(OK, token_depth=4), "token_depth"),
    (dict(OK, token_depth=-4), "token_depth"),
    (dict(OK, token_select="cls"), "token_select"),
    (dict(OK, attack="apgd"), "apgd"),                                   # no batched token APGD
])
def test_trainer_refuses_before_any_device_work(kw, match):
    # state_dict None: anything past the argument checks would fail differently (and need a device)
    with pytest.raises(ValueError, match=match):
        AdversarialTrainer(CFG, None, 4, **kw)


def test_refusals_leave_what_is_allowed_alone():
    # an unused clean loss / an unused inner loss are not refused: the checks pass and construction goes on to the device work
    chk = AdversarialTrainer._check_token_options
    assert chk(CFG, "l2-tokens", "l2", "l2", "none", 0.0, False, -2, "patch") == (2, "patch")
    assert chk(CFG, "l2-tokens", "l2-tokens", "l2", "pgd", 0.0, False, 3, "all") == (3, "all")
    assert chk(CFG, "l2-tokens", "l2-tokens", "l2-tokens", "pgd", 0.3, False, -1, "patch") == (3, "patch")
    assert chk("ViT-L-14", "l2-tokens", "l2-tokens", "l2", "pgd", 0.0, False, -2, "patch") == (23, "patch")
