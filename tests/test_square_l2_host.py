"""Square Attack, L2 (RVLM_HAS_SQUARE_L2), host side: the entry point is declared in include/rvlm.h, exported by the library and
bound in _lib (an addition: RVLM_VERSION does not move); eta_window / l2_window_size against what the reference itself produced
(tests/golden/square_l2_tiny.npz, made by tests/golden/make_golden_square_l2.py); which norms SquareAttack and AutoAttack build."""
import os
import re

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd import square as S
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA_SIZES = (2, 3, 5, 6, 7, 9, 21, 44, 45)


def test_symbols_are_additions_only():
    with open(os.path.join(ROOT, "include", "rvlm.h")) as f:
        hdr = f.read()
    lib = L.load()
    assert re.search(r"\bint\s+rvlm_square_l2_propose\s*\(", hdr)
    assert "rvlm_square_l2_propose" in L.EXPORTED_SYMBOLS and hasattr(lib, "rvlm_square_l2_propose")
    assert len(L._SIGS["rvlm_square_l2_propose"][1]) == 18
    assert re.search(r"#define\s+RVLM_HAS_SQUARE_L2\s+1\b", hdr)
    assert re.search(r"RVLM_FLAG_SQUARE_NONFINITE\s*=\s*256\b", hdr) and L.FLAG_SQUARE_NONFINITE == 256
    assert re.search(r"#define\s+RVLM_VERSION\s+109\b", hdr) and lib.rvlm_version() == 109


@pytest.mark.parametrize("s", ETA_SIZES)
def test_eta_window_is_the_references_eta_bit_for_bit(s):
    z = load_golden("square_l2_tiny.npz")
    want = z[f"eta_{s}"].T if bool(z[f"eta_{s}_transposed"]) else z[f"eta_{s}"]
    got = S.eta_window(s)
    assert got.dtype == torch.float32 and tuple(got.shape) == (s, s) and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), want)
    assert S.eta_window(s) is got                                        # cached per s


def test_eta_coin_is_drawn_on_the_cpu_generator():
    z = load_golden("square_l2_tiny.npz")
    assert len({bool(z[f"eta_{s}_transposed"]) for s in ETA_SIZES}) == 2     # the fixture holds both outcomes
    atk = R.SquareAttack(lambda v: v, norm='L2', eps=.5)
    torch.random.manual_seed(123)                                        # the generator's seed: the same coins, in its order
    for s in ETA_SIZES:
        assert np.array_equal(atk.eta(s).contiguous().numpy(), z[f"eta_{s}"])


def test_l2_window_size_reproduces_the_references_schedule():
    z = load_golden("square_l2_tiny.npz")
    want = z["schedule_224"]
    assert want.shape == (5000,)
    got = [S.l2_window_size(it, 5000, .8, False, 3, 224, 224) for it in range(5000)]
    assert got == want.tolist()
    assert S.l2_window_size(0, 50, .8, False, 3, 32, 32) == 29           # sqrt(.8 * 1024) = 28.6 -> 29, odd
    assert S.l2_window_size(0, 50, .8, False, 3, 32, 20) == 20           # at most the image (22.6 -> 23 -> 20)
    assert S.l2_window_size(4999, 5000, .05, False, 3, 8, 8) == 3        # at least 3
    assert S.l2_window_size(0, 50, .8, False, 3, 33, 33) == 31           # 29.5 -> 30 -> made odd


def test_which_norms_are_built():
    f = lambda v: v.flatten(1)[:, :10]      # noqa: E731
    atk = R.SquareAttack(f, norm='L2', eps=.5)
    assert (atk.norm, atk.eps, atk.n_queries, atk.p_init, atk.loss) == ('L2', .5, 5000, .8, 'margin')
    with pytest.raises(NotImplementedError):
        R.SquareAttack(f, norm='L1', eps=.5)
    aa = R.AutoAttack(f, norm='L2', eps=.5, verbose=False, version='custom', attacks_to_run=['square'])
    assert isinstance(aa.square, R.SquareAttack) and aa.square.norm == 'L2' and aa._unavailable('square') == ''
    assert (aa.square.n_queries, aa.square.p_init, aa.square.n_restarts, aa.square.rescale_schedule) == (5000, .8, 1, False)
    assert not isinstance(aa.fab, R.FABAttack)
    with pytest.raises(NotImplementedError):                             # L1: no attack of the ensemble is built, APGD refuses first
        R.AutoAttack(f, norm='L1', eps=12., verbose=False, version='custom', attacks_to_run=['square'])
    std = R.AutoAttack(f, norm='L2', eps=.5, verbose=False)              # version='standard' holds fab-t, which has no L2 form
    assert std._unavailable('square') == '' and std._unavailable('fab-t') != ''
    with pytest.raises(NotImplementedError, match="norm='Linf' only"):
        std.run_standard_evaluation(torch.rand(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), bs=2)


def test_start_point_refuses_what_the_references_slicing_refuses():
    atk = R.SquareAttack(lambda v: v, norm='L2', eps=.5)
    with pytest.raises(ValueError):
        atk._l2_start(2, 3, 4, 32)                                      # h // 5 == 0
    with pytest.raises(ValueError):
        atk._l2_start(2, 3, 24, 24)                                     # tiles of side 4 from row 2: the sixth ends at 26
    torch.random.manual_seed(0)
    d = atk._l2_start(2, 3, 21, 27)                                     # non-square, the reference's arithmetic
    assert tuple(d.shape) == (2, 3, 21, 27)
    assert torch.allclose((d.double() ** 2).flatten(1).sum(1), torch.ones(2, dtype=torch.float64), atol=1e-5)
    assert float(d[:, :, 20:].abs().max()) == 0.0 and float(d[:, :, :, 24:].abs().max()) == 0.0
