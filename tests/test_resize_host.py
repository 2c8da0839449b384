"""Host-side checks of the in-model bicubic resizer: the tap tables (no device needed), ``BicubicResize``'s Python surface, the
C ABI declarations and the golden fixture (no GPU), in the style of tests/test_fab_host.py."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.resize import resize_taps
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_SYMBOLS = ("rvlm_vit_set_input_size", "rvlm_resize_bicubic", "rvlm_resize_bicubic_adjoint", "rvlm_resize_taps")
KERNEL_SYMBOLS = ("rvlm_k_resize_im2col_normalize", "rvlm_k_col2im_resize_grad")
SIZE_PAIRS = [(32, 224), (96, 224), (12, 32), (224, 224), (5, 13)]


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(rvlm_[a-z0-9_]+)\s*\(", txt))


def _built():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def taps_float64(n_in, n_out, A=-0.75):
    """Restatement of the operator's definition in float64: src = (in / out) (o + 0.5) - 0.5, taps floor(src) - 1 .. + 2 clamped,
    cubic-convolution weights."""
    idx = np.empty((n_out, 4), np.int64)
    w = np.empty((n_out, 4), np.float64)
    near = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0          # noqa: E731
    far = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A     # noqa: E731
    for o in range(n_out):
        src = (n_in / n_out) * (o + 0.5) - 0.5
        i = int(np.floor(src))
        t = src - i
        idx[o] = np.clip(np.arange(i - 1, i + 3), 0, n_in - 1)
        w[o] = (far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t))
    return idx, w


def dense(idx, w, n_in):
    Rm = np.zeros((idx.shape[0], n_in))
    for k in range(4):
        np.add.at(Rm, (np.arange(idx.shape[0]), idx[:, k]), w[:, k])
    return Rm


@pytest.mark.parametrize("n_in,n_out", SIZE_PAIRS)
def test_resize_taps_match_definition_and_torch(n_in, n_out):
    _built()
    idx, w = resize_taps(n_in, n_out)
    assert idx.shape == w.shape == (n_out, 4) and idx.dtype == np.int32 and w.dtype == np.float32
    ridx, rw = taps_float64(n_in, n_out)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(w, rw.astype(np.float32)), "weights are the float64 values rounded to fp32"
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 2e-7
    # the operator itself: F.interpolate applied to unit vectors (rows of the identity, resized along the last axis)
    eye = torch.eye(n_in, dtype=torch.float64)[None, None]
    cols = F.interpolate(eye, size=(n_in, n_out), mode="bicubic", align_corners=False)[0, 0].numpy()     # [i, o] = R[o, i]
    assert np.abs(dense(idx, w.astype(np.float64), n_in) - cols.T).max() < 1e-7
    assert np.abs(dense(ridx, rw, n_in) - cols.T).max() < 1e-14
    if n_in == n_out:
        assert np.array_equal(idx[:, 1], np.arange(n_in)) and np.array_equal(w, np.tile(np.float32([0, 1, 0, 0]), (n_in, 1)))


def test_resize_taps_refuses_bad_arguments():
    lib = _built()
    import ctypes as C
    idx, w = (C.c_int32 * 16)(), (C.c_float * 16)()
    assert lib.rvlm_resize_taps(0, 4, idx, w) == L.RVLM_ERR_ARG
    assert lib.rvlm_resize_taps(4, 0, idx, w) == L.RVLM_ERR_ARG
    assert lib.rvlm_resize_taps(4, 4, None, w) == L.RVLM_ERR_ARG
    assert lib.rvlm_resize_taps(4, 4, idx, w) == L.RVLM_OK


def test_bicubic_resize_constructor_size_rule_and_refusals():
    r = R.BicubicResize(224)
    assert r.size == 224 and r.antialias is False and isinstance(r, torch.nn.Module)
    assert r.output_size(32, 32) == (224, 224) and r.output_size(96, 96) == (224, 224)
    # torchvision: the smaller edge becomes `size`, the other int(size * long / short)
    assert r.output_size(32, 48) == (224, 336) and r.output_size(48, 32) == (336, 224)
    assert R.BicubicResize(100).output_size(30, 47) == (100, int(100 * 47 / 30))
    assert R.BicubicResize([224]).size == 224
    assert R.BicubicResize((5, 7)).output_size(3, 9) == (5, 7) and R.BicubicResize([5, 7]).size == (5, 7)
    for bad in (0, -3, 2.5, (1, 2, 3), (0, 4), "224", True):
        with pytest.raises(ValueError):
            R.BicubicResize(bad)
    with pytest.raises(NotImplementedError):
        R.BicubicResize(224, antialias=True)
    with pytest.raises(L.RvlmError):                      # no CPU fallback
        r(torch.rand(2, 3, 8, 8))
    assert "BicubicResize" in R.__all__


def test_resize_entry_points_are_declared_exported_and_bound():
    lib = _built()
    top, kern = _declared("rvlm.h"), _declared("rvlm_kernels.h")
    for sym in TOP_SYMBOLS:
        assert sym in top and sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    for sym in KERNEL_SYMBOLS:
        assert sym in kern and sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    hdr = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    assert re.search(r"#define\s+RVLM_HAS_INPUT_RESIZE\s+1", hdr)
    assert lib.rvlm_version() == int(re.search(r"#define\s+RVLM_VERSION\s+(\d+)", hdr).group(1)) == 109
    # header argument counts agree with the ctypes signatures
    flat = re.sub(r"/\*.*?\*/", "", hdr + open(os.path.join(ROOT, "include", "rvlm_kernels.h")).read(), flags=re.S)
    for sym in TOP_SYMBOLS + KERNEL_SYMBOLS:
        args = re.search(r"\b" + sym + r"\s*\(([^)]*)\)", flat).group(1)
        assert len(args.split(",")) == len(L._SIGS[sym][1]), sym
    assert lib.rvlm_vit_set_input_size(None, 32, 32) == L.RVLM_ERR_ARG


def test_classification_model_accepts_only_what_the_engine_can_resize():
    """engine_input_size: the rule that decides between the fused route and the generic one, on a stand-in engine (no device)."""
    from robustvlm_amd.clip_model import ClassificationModel

    class Eng:
        cfg = R.CONFIGS["ViT-B-32"]
        trainable = False

    def stand_in(resizer):
        m = ClassificationModel.__new__(ClassificationModel)
        torch.nn.Module.__init__(m)
        m.model, m.resizer, m._identity_resizer = Eng(), resizer, False
        return m
    m = stand_in(R.BicubicResize(224))
    assert m.engine_input_size(torch.empty(2, 3, 32, 32)) == (32, 32)
    assert m.engine_input_size(torch.empty(2, 3, 96, 96)) == (96, 96)
    assert m.engine_input_size(torch.empty(2, 3, 224, 224)) == (224, 224)
    assert m.engine_input_size(torch.empty(2, 3, 32, 48)) is None          # result is not the model's square
    assert m.engine_input_size(torch.empty(2, 3, 448, 448)) is None        # down-sampling stays outside the engine
    assert m.engine_input_size(torch.empty(2, 1, 32, 32)) is None
    m = stand_in(lambda v: v)
    assert m.engine_input_size(torch.empty(2, 3, 32, 32)) is None          # any other callable: the generic route, as before


def test_resize_golden_is_small_and_complete():
    z = load_golden("attacks_resize_tiny.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "attacks_resize_tiny.npz")) < 1 << 20
    assert list(z["sizes"]) == [16, 12]
    for size in (16, 12):
        t = f"s{size}_"
        assert z[t + "x"].shape == (7, 3, size, size) and z[t + "apgd_adv"].shape == (7, 3, size, size)
        eps = np.float32(float(z[t + "eps"]))
        for key in ("apgd_adv", "aa_x_adv", "pgd_xadv", "run_x_best_adv"):
            a = z[t + key]
            assert np.abs(a - z[t + "x"]).max() <= eps + 1e-7 and a.min() >= 0 and a.max() <= 1, key
        assert 0 < z[t + "apgd_robust"].sum() < 7, "a fixture whose robust set is trivial shows nothing"
        assert float(z[t + "pgd_loss_final"]) > float(z[t + "pgd_loss_start"])
