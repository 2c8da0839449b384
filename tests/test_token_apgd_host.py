"""Batched token APGD (RVLM_HAS_TOKEN_APGD), host side: the entry is declared in include/rvlm.h, exported by the library and bound in
robustvlm_amd/_lib.py with the ABI number unchanged; the Python surface has the documented signatures and refuses CPU tensors, unknown
norms and a pooled trainer before any device work; and the fixture tests/golden/token_apgd_tiny.npz (the reference's own apgd() runs)
holds what the GPU tests rely on."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.trainer import AdversarialTrainer
from tests import token_apgd_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rvlm_apgd_run_tokens"


def _header():
    return open(os.path.join(ROOT, "include", "rvlm.h")).read()


def test_entry_is_declared_announced_exported_and_bound():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code), f"{NAME} is not declared in include/rvlm.h"
    assert re.search(r"#define\s+RVLM_HAS_TOKEN_APGD\s+1\b", hdr)
    assert re.search(r"#define\s+RVLM_VERSION\s+109\b", hdr)
    assert re.search(r"still 109, additions only:.*%s \(announced by RVLM_HAS_TOKEN_APGD\)" % NAME, hdr, flags=re.S)
    assert NAME in L.EXPORTED_SYMBOLS
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    assert hasattr(lib, NAME) and lib.rvlm_version() == 109


def test_prototype_of_the_binding_matches_the_header():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, code, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    res, args = L._SIGS[NAME]
    assert res is C.c_int and len(args) == len(params) == 20
    for p, a in zip(params, args):
        if "*" in p or p.startswith("rvlm_stream_t"):
            assert a is C.c_void_p, p
        elif p.startswith("float "):
            assert a is C.c_float, p
        else:
            assert p.startswith("int ") and a is C.c_int, p
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["h", "x", "x_init", "B", "depth", "ln_post", "select", "ref_tokens", "norm_kind", "eps", "n_iter", "step0", "rho",
                     "x_best_out", "loss_best_out", "x_last_out", "loss_trace_out", "step_out", "flags", "stream"]


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]


def test_python_signatures():
    E = inspect.Parameter.empty
    assert R.apgd_tokens is R.token_attacks.apgd_tokens and "apgd_tokens" in R.__all__
    assert _sig(R.apgd_tokens) == [("tower", E), ("x", E), ("ref_tokens", E), ("norm", E), ("eps", E), ("n_iter", 10),
                                   ("pert_init", None), ("alpha", None), ("rho", 0.75), ("return_trace", False)]
    assert _sig(AdversarialTrainer.eval_step_tokens) == [("data_eval", E), ("n_iter", 50), ("pert_init", None)]
    names = [n for n, _ in _sig(R.VitEngine.apgd_run_tokens)]
    assert names[:6] == ["x", "x_init", "ref_tokens", "eps", "n_iter", "step0"]
    assert {"depth", "ln_post", "select", "norm_kind", "rho"} <= set(names)


def test_cpu_tensors_raise():
    x, ref = torch.zeros(2, 3, 32, 32), torch.zeros(2, 16, 64)
    with pytest.raises(L.RvlmError, match="CUDA"):
        R.apgd_tokens(None, x, ref, "linf", 4 / 255)


@pytest.mark.parametrize("norm", ["L1", "l1", "L0", "inf", 2, None])
def test_unknown_norm_raises_before_anything_else(norm):
    with pytest.raises(NotImplementedError):
        R.apgd_tokens(None, None, None, norm, 0.1)


def test_eval_step_tokens_needs_the_token_loss():
    chk = AdversarialTrainer._check_token_options
    assert chk(R.VitConfig(96, 16, 128, 3, 2, 48), "l2", "l2", "l2", "pgd", 0.0, False, -2, "patch")[0] is None   # a pooled trainer
    t = AdversarialTrainer.__new__(AdversarialTrainer)       # ... whose eval_step_tokens refuses before it touches anything else
    t.token_mode = False
    with pytest.raises(ValueError, match="l2-tokens"):
        t.eval_step_tokens(None)


def test_the_training_time_attack_still_refuses_apgd():
    with pytest.raises(ValueError, match="apgd"):
        AdversarialTrainer(R.VitConfig(96, 16, 128, 3, 2, 48), None, 4, loss="l2-tokens", inner_loss="l2-tokens", attack="apgd")


# ---- the fixture ------------------------------------------------------------------------------------------------------------
CASES, GET = TC.load()


def test_fixture_covers_the_case_grid_and_is_small():
    assert os.path.getsize(TC.PATH) < 1_000_000
    grid = {(c["norm"], c["radius"], c["depth"], c["select"], c["n_iter"]) for c in CASES}
    want = {(n, r, d, s, k) for n in ("linf", "l2") for r in ("small", "large") for d, s in ((1, "patch"), (2, "all"))
            for k in (1, 10, 25)}
    assert grid == want and len(CASES) == 24
    eps = {(c["norm"], c["radius"]): c["eps"] for c in CASES}
    assert eps == {("linf", "small"): 4 / 255, ("linf", "large"): 32 / 255, ("l2", "small"): 0.5, ("l2", "large"): 6.0}


def test_packing_round_trips():
    rng = np.random.default_rng(0)
    x = rng.random((2, 3, 5, 7), dtype=np.float32)
    a = np.clip(x + rng.choice([-0.1, 0.1, 0.03], x.shape).astype(np.float32), 0, 1).astype(np.float32)
    for eps in (0.1, 0.0):
        s, p = TC.pack(a, x, eps)
        assert np.array_equal(TC.unpack(s, p, x, eps).view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_conditions(case):
    g = GET(case["name"])
    x, eps, tr = g["x"], case["eps"], g["trace"]
    B = x.shape[0]
    assert B == 4 and tr.shape == (case["n_iter"] + 1, B) and np.isfinite(tr).all()
    assert np.array_equal(g["loss_best"], tr.max(axis=0))                      # loss_best == max of each image's trace
    decreases = (tr[1:] < tr[:-1]).sum(axis=0)
    if case["radius"] == "large" and case["n_iter"] >= 10:
        assert (decreases >= 1).all(), decreases                                # the controller's restart path is exercised ...
        assert (g["step_seen"] < 0.75 * 2 * eps).any(), g["step_seen"]          # ... and a step was halved
    if case["radius"] == "small":
        assert (decreases == 0).all(), decreases
    start = np.clip(x + g["pert_init"], 0, 1)
    for it in (start, g["x_best"], g["x_last"]):                                # every stored iterate: in the ball and in [0, 1]
        assert it.min() >= 0 and it.max() <= 1
        d = it.astype(np.float64) - x
        if case["norm"] == "linf":
            # the ball in the arithmetic that made it: fl(x - eps) <= x_adv <= fl(x + eps) in float32, exactly
            assert (it <= x + np.float32(eps)).all() and (it >= x - np.float32(eps)).all()
        else:
            assert np.sqrt((d ** 2).reshape(B, -1).sum(1)).max() <= eps * (1 + 1e-5)
