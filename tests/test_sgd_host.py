"""SGD with momentum (``--opt sgd``), the part that needs no GPU: the C ABI announces and exports rvlm_sgd_step, the trainer refuses
an unknown optimizer before it touches a device, and tests/golden/train_step_sgd_tiny.npz (the reference's own train_one_epoch
under torch.optim.SGD, tests/golden/make_golden_train_sgd.py) is self-consistent and can tell a wrong update from a right one."""
import os
import re

import numpy as np
import pytest

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.trainer import AdversarialTrainer, cosine_lr_value
from tests.helpers import GOLDEN, load_golden, weights_from_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "train_step_sgd_tiny.npz"
CASES = ("fare_pgd", "none_cw", "tecoa_pgd")
W_STEPS, BUF_STEPS = (1, 3, 5), (3, 5)


def snapshot_file(name, s):
    return f"train_step_sgd_tiny_{name}_s{s}.npz"


def test_sgd_entry_is_declared_exported_bound_and_announced():
    header = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+rvlm_sgd_step\s*\(", code), "rvlm_sgd_step is not declared in include/rvlm.h"
    assert re.search(r"^#define\s+RVLM_HAS_SGD\s+1\s*$", code, flags=re.M), "RVLM_HAS_SGD is not 1"
    assert re.search(r"^#define\s+RVLM_VERSION\s+109\s*$", code, flags=re.M)
    assert "rvlm_sgd_step" in L.EXPORTED_SYMBOLS
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    fn = lib.rvlm_sgd_step                                     # exported (AttributeError otherwise) ...
    assert fn.restype is not None and len(fn.argtypes) == 10   # ... and bound with the ten arguments of the declaration
    assert lib.rvlm_version() == 109


def test_unknown_optimizer_is_refused_before_any_device_work():
    cfg = R.VitConfig(32, 8, 64, 2, 1, 32)
    with pytest.raises(ValueError, match="Optimizer rmsprop not supported."):
        AdversarialTrainer(cfg, {}, batch_size=2, opt="rmsprop", device="cuda:0")
    with pytest.raises(ValueError, match="Optimizer rmsprop not supported."):
        AdversarialTrainer(cfg, {}, batch_size=2, opt="rmsprop")           # not even torch.cuda.current_device()


def test_fixture_size_and_contents():
    files = [FIXTURE] + [snapshot_file(name, s) for name in CASES for s in W_STEPS]
    assert sorted(f for f in os.listdir(GOLDEN) if f.startswith("train_step_sgd_tiny")) == sorted(files)
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 2 ** 20, f
    z = load_golden(FIXTURE)
    assert tuple(z["cases"]) == CASES and float(z["momentum"]) == 0.9 and float(z["wd"]) == 1e-2
    w = weights_from_golden(load_golden("train_step_tiny.npz"))           # the inputs are that fixture's (same seeds)
    assert list(z["keys"]) == list(w)
    for name in CASES:
        for key in ("lr_used", "lr_after", "loss", "loss_total", "cos_sim_clean", "cos_sim", "acc", "racc"):
            assert z[f"{name}::{key}"].shape == (5,), (name, key)
        assert (f"{name}::x_adv" in z.files) == (name != "none_cw")
        for s in W_STEPS:                                                   # EVERY parameter, a momentum buffer for EVERY parameter
            snap = load_golden(snapshot_file(name, s))
            want = ["w::" + k for k in w] + (["buf::" + k for k in w] if s in BUF_STEPS else [])
            assert sorted(snap.files) == sorted(want), (name, s)
            for k, v in w.items():
                assert snap["w::" + k].shape == tuple(v.shape) and snap["w::" + k].dtype == np.float32, (name, s, k)
                if s in BUF_STEPS:
                    buf = snap["buf::" + k]
                    assert buf.shape == tuple(v.shape) and np.isfinite(buf).all() and np.abs(buf).max() > 0, (name, s, k)


@pytest.mark.parametrize("name", CASES)
def test_fixture_learning_rates_follow_the_schedule(name):
    """Step 1 runs at the base LR (the reference calls its scheduler only after a step), step s + 1 at cosine_lr(s)."""
    z = load_golden(FIXTURE)
    lr, warmup, steps = float(z[f"{name}::lr"]), int(z["warmup"]), int(z["steps"])
    used, after = z[f"{name}::lr_used"], z[f"{name}::lr_after"]
    assert used[0] == lr
    for s in range(1, len(used)):
        assert used[s] == cosine_lr_value(s, lr, warmup, steps), (s, used[s])
    for s in range(len(after)):
        assert after[s] == cosine_lr_value(s + 1, lr, warmup, steps), (s, after[s])


@pytest.mark.parametrize("name", CASES)
def test_fixture_updates_are_neither_rounding_noise_nor_a_collapse(name):
    """SGD's update is not normalised: for every tensor max|w_5 - w_0| / max|w_0| has to lie in [3e-5, 5e-2] - two orders above five
    fp32 roundings of a parameter, and small enough that a 2e-3 gradient difference is not amplified along the trajectory."""
    z = load_golden(FIXTURE)
    assert float(z["ratio_min"]) == 3e-5 and float(z["ratio_max"]) == 5e-2
    w = weights_from_golden(load_golden("train_step_tiny.npz"))
    w5 = load_golden(snapshot_file(name, 5))
    for k, v in w.items():
        ratio = float(np.abs(w5["w::" + k].astype(np.float64) - v.numpy().astype(np.float64)).max()) / float(v.abs().max())
        assert 3e-5 <= ratio <= 5e-2, (name, k, ratio)
