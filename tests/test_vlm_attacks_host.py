"""VLM-side attacks (RVLM_HAS_VLM_ATTACKS), host side: the entry points are declared in include/rvlm.h, exported by the library
and bound in _lib; RVLM_VERSION did not move; PGD / APGD carry the reference's constructor attributes; what the native path does
not cover is refused before anything touches a device."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.vlm_attacks import APGD, PGD, TokenLossModel, apgd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rvlm_mask_grad", "rvlm_pgd_masked_update", "rvlm_apgd_masked_step", "rvlm_apgd_masked_bookkeeping")


def test_symbols_declared_exported_bound_and_announced():
    hdr = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, code), f"{sym} is not declared in include/rvlm.h"
        assert sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define\s+RVLM_HAS_VLM_ATTACKS\s+1\b", hdr)
    assert re.search(r"#define\s+RVLM_VERSION\s+109\b", hdr) and lib.rvlm_version() == 109
    src = open(os.path.join(ROOT, "robustvlm_amd", "csrc", "Makefile")).read()
    assert "vlm_attack_kernels.hip" in src


def test_package_exports():
    assert R.vlm_attacks.PGD is PGD and R.vlm_attacks.APGD is APGD and R.vlm_attacks.apgd is apgd
    assert R.TokenLossModel is TokenLossModel and "vlm_attacks" in R.__all__ and "TokenLossModel" in R.__all__


def test_signatures_are_the_references():
    """pgd.py:10,21 and apgd.py:6,23,163-164, parameter for parameter with the same defaults."""
    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]
    E = inspect.Parameter.empty
    assert sig(PGD.__init__) == [("forward", E), ("norm", E), ("eps", E), ("mode", "min"), ("mask_out", "context"),
                                 ("image_space", True)]
    assert sig(PGD.perturb) == [("data_clean", E), ("iterations", E), ("stepsize", E), ("perturbation", None), ("verbose", False),
                                ("return_loss", False)]
    assert sig(APGD.__init__) == [("model", E), ("norm", E), ("eps", E), ("mask_out", "context"), ("initial_stepsize", None),
                                  ("decrease_every", None), ("decrease_every_max", None), ("random_init", False)]
    assert sig(APGD.perturb) == [("data_clean", E), ("iterations", E), ("pert_init", None), ("verbose", False)]
    assert sig(apgd) == [("model", E), ("x", E), ("norm", E), ("eps", E), ("n_iter", 10), ("use_rs", False), ("mask", None),
                         ("alpha", None), ("n_iter_2", None), ("n_iter_min", None), ("pert_init", None), ("verbose", False),
                         ("is_train", True)]


def test_constructor_attributes():
    f = lambda x: x.sum()   # noqa: E731
    p = PGD(f, "linf", 0.25, mode="max", mask_out="query", image_space=False)
    assert vars(p) == dict(model=f, norm="linf", eps=0.25, momentum=0.9, mode="max", mask_out="query", image_space=False)
    a = APGD(f, "linf", 0.5, mask_out="none", initial_stepsize=1.0, decrease_every=0.3, decrease_every_max=0.1, random_init=True)
    assert vars(a) == dict(model=f, norm="linf", eps=0.5, initial_stepsize=1.0, decrease_every=0.3, decrease_every_max=0.1,
                           random_init=True, mask_out=None)
    assert APGD(f, "l2", 0.5).mask_out == "context" and APGD(f, "l2", 0.5, mask_out=2).mask_out == 2
    assert str(a) == "APGD"


def test_masks_are_one_byte_per_image():
    x = torch.zeros(1, 5, 1, 3, 2, 2)
    f = lambda v: v.sum()   # noqa: E731
    want = {"context": [0, 0, 0, 0, 1], "query": [1, 1, 1, 1, 0], 1: [1, 0, 1, 1, 1], -2: [1, 1, 1, 0, 1], None: [1] * 5}
    for mask_out, m in want.items():
        for atk in (PGD(f, "linf", 0.1, mask_out=mask_out), APGD(f, "linf", 0.1, mask_out=mask_out)):
            got = atk._set_mask(x)
            assert got.dtype == torch.uint8 and got.tolist() == m, (mask_out, got)
    assert APGD(f, "linf", 0.1, mask_out="none")._set_mask(x).tolist() == [1] * 5
    assert PGD(f, "linf", 0.1, mask_out="context")._set_mask(torch.zeros(1, 1, 1, 3, 2, 2)).tolist() == [1]   # [:, :-1] is empty


def test_refusals_before_any_device_work():
    x = torch.rand(1, 3, 1, 3, 4, 4)
    f = lambda v: v.sum().reshape(1)   # noqa: E731
    for norm in ("L1", "l1", "L0"):
        with pytest.raises(NotImplementedError, match="L1|L0"):
            apgd(f, x, norm, 0.1)
        with pytest.raises(NotImplementedError, match="L1|L0"):
            APGD(f, norm, 0.1).perturb(x, 3)
    with pytest.raises(NotImplementedError, match="l1"):
        PGD(f, "l1", 0.1).perturb(x, 3, 0.01)
    for bad in ("all", "Context", 1.5):
        with pytest.raises(NotImplementedError, match="Unknown mask_out"):
            PGD(f, "linf", 0.1, mask_out=bad).perturb(x, 3, 0.01)
        with pytest.raises(NotImplementedError, match="Unknown mask_out"):
            APGD(f, "linf", 0.1, mask_out=bad).perturb(x, 3)
    with pytest.raises(ValueError, match="Unknown mode"):
        PGD(f, "linf", 0.1, mode="ascend").perturb(x, 3, 0.01)
    with pytest.raises(AssertionError):                       # apgd.py:166: batch size 1 only
        apgd(f, torch.rand(2, 3, 1, 3, 4, 4), "linf", 0.1)
    with pytest.raises(AssertionError):
        APGD(f, "linf", 0.1).perturb(torch.rand(2, 3, 1, 3, 4, 4), 3)
    # CPU tensors: no CPU fallback anywhere in this package
    with pytest.raises(L.RvlmError, match="no CPU fallback"):
        PGD(f, "linf", 0.1).perturb(x, 3, 0.01)
    with pytest.raises(L.RvlmError, match="no CPU fallback"):
        APGD(f, "linf", 0.1).perturb(x, 3)
    with pytest.raises(L.RvlmError, match="no CPU fallback"):
        apgd(f, x, "l2", 0.1)
    with pytest.raises(TypeError):
        TokenLossModel(torch.nn.Identity(), x)


def test_golden_file_holds_arrays_of_every_case(golden_dir):
    path = os.path.join(golden_dir, "vlm_attacks.npz")
    assert os.path.getsize(path) < 600 * 1024
    z = np.load(path)
    cases = json.loads(str(z["cases"]))
    assert len(str(z["reference_sha256"])) == 64
    pgd = [c for c in cases if c["kind"] == "pgd"]
    ap = [c for c in cases if c["kind"] == "apgd"]
    for norm in ("linf", "l2"):
        combos = {(c["mask_out"], c["mode"]) for c in pgd if c["norm"] == norm and c["image_space"]}
        assert combos >= {(m, mode) for m in ("context", "query", 1, None) for mode in ("min", "max")}
        assert any(not c["image_space"] for c in pgd if c["norm"] == norm)
        assert {(c["n_iter"], c["pert"]) for c in ap if c["norm"] == norm} == {(10, False), (10, True), (50, False), (50, True)}
    assert any(c["nan"] for c in pgd)
    for c in cases:
        n_calls = z[c["name"] + "/losses"].shape[0]
        assert z[c["name"] + "/grads"].shape == (n_calls,) + z["x"].shape
        assert n_calls == (c["iterations"] if c["kind"] == "pgd" else c["n_iter"] + 1)
