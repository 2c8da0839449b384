"""Host-side checks of the FAB attack's Python surface, C ABI declarations and golden fixture (no GPU), in the style of
tests/test_text_host.py."""
import os
import re

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from tests.fab_cases import hashed_row, closed_form_lambda
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAB_SYMBOLS = ("rvlm_fab_projection_linf", "rvlm_fab_linf_step", "rvlm_fab_track_best", "rvlm_fab_jacobian_argmin")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(rvlm_[a-z0-9_]+)\s*\(", txt))


def test_fab_entry_points_are_declared_exported_and_bound():
    """Additions only: declared in include/rvlm.h, exported by librvlm.so, bound in _lib, announced by RVLM_HAS_FAB;
    RVLM_VERSION does not move."""
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    top = _declared("rvlm.h")
    for sym in FAB_SYMBOLS:
        assert sym in top and sym in L.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    hdr = open(os.path.join(ROOT, "include", "rvlm.h")).read()
    assert re.search(r"#define\s+RVLM_HAS_FAB\s+1", hdr)
    assert re.search(r"RVLM_LOSS_LOGIT_DIFF\s*=\s*4\b", hdr) and L.LOSS_LOGIT_DIFF == 4
    assert re.search(r"RVLM_FLAG_FAB_NONFINITE\s*=\s*64\b", hdr) and L.FLAG_FAB_NONFINITE == 64
    assert lib.rvlm_version() == int(re.search(r"#define\s+RVLM_VERSION\s+(\d+)", hdr).group(1)) == 109


def test_fabattack_constructor_and_refusals():
    f = lambda v: v.flatten(1)[:, :10]      # noqa: E731
    atk = R.FABAttack(f, eps=8 / 255, n_restarts=3, n_iter=7, seed=5, targeted=True, n_target_classes=4)
    assert (atk.predict, atk.norm, atk.n_restarts, atk.n_iter, atk.eps) == (f, 'Linf', 3, 7, 8 / 255)
    assert (atk.alpha_max, atk.eta, atk.beta, atk.seed, atk.targeted, atk.n_target_classes) == (0.1, 1.05, 0.9, 5, True, 4)
    assert atk.target_class is None and atk.device is None and atk.verbose is False
    assert R.FABAttack(f).eps == 0.3                       # DEFAULT_EPS_DICT_BY_NORM['Linf']
    for norm in ('L2', 'L1'):
        with pytest.raises(NotImplementedError):
            R.FABAttack(f, norm=norm, eps=0.5)
    if not torch.cuda.is_available():
        x, y = torch.rand(3, 3, 8, 8), torch.zeros(3, dtype=torch.long)
        with pytest.raises(L.RvlmError):
            atk.perturb(x, y)
        with pytest.raises(L.RvlmError):
            atk.attack_single_run(x, y)


def test_autoattack_builds_fab_and_reports_where_it_cannot_run():
    f = lambda v: v.flatten(1)[:, :10]      # noqa: E731
    aa = R.AutoAttack(f, norm='Linf', eps=4 / 255, seed=1, verbose=False)           # the default version, device='cuda'
    assert isinstance(aa.fab, R.FABAttack) and aa.attacks_to_run == ['apgd-ce', 'apgd-t', 'fab-t', 'square']
    assert (aa.fab.n_restarts, aa.fab.n_target_classes, aa.fab.n_iter, aa.fab.eps, aa.fab.seed) == (1, 9, 100, 4 / 255, 1)
    assert all(aa._unavailable(a) == '' for a in aa.attacks_to_run)
    plus = R.AutoAttack(f, norm='Linf', eps=4 / 255, verbose=False, version='plus')
    assert plus.fab.n_restarts == 5 and all(plus._unavailable(a) == '' for a in plus.attacks_to_run)
    cpu = R.AutoAttack(f, norm='Linf', eps=4 / 255, verbose=False, version='custom', attacks_to_run=['fab'], device='cpu')
    assert 'GPU' in cpu._unavailable('fab')
    with pytest.raises(NotImplementedError, match='no CPU fallback'):
        cpu.run_standard_evaluation(torch.rand(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), bs=2)
    l2 = R.AutoAttack(f, norm='L2', eps=0.5, verbose=False, version='custom', attacks_to_run=['fab-t'])
    assert not isinstance(l2.fab, R.FABAttack) and l2.fab.n_restarts == 5
    with pytest.raises(NotImplementedError, match="norm='Linf' only"):
        l2.run_standard_evaluation(torch.rand(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), bs=2)


def _check_row(t, w, b, d, lam):
    """The projection's contract in float64: box, hyperplane (where it meets the box), w_i = 0 -> d_i = 0, max|d| = lambda."""
    t64, w64, d64 = t.astype(np.float64), w.astype(np.float64), d.astype(np.float64)
    want, feasible = closed_form_lambda(t, w, b)
    assert abs(lam - want) <= 1e-9 + 1e-9 * want
    assert abs(np.abs(d64).max() - want) <= 1e-7                      # d is stored as float32
    assert (t64 + d64 >= -1e-7).all() and (t64 + d64 <= 1 + 1e-7).all()
    assert (d64[w64 == 0] == 0).all()
    if feasible:
        assert abs(np.dot(w64, t64 + d64) - float(b)) <= 1e-4 * (1 + abs(float(b)))


def test_fab_golden_is_self_consistent():
    z = load_golden("fab_tiny.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fab_tiny.npz")) < 1 << 20
    kinds = set()
    for tag in ("p1003", "p3000"):
        t, w, b, d, lam = (z[f"{tag}_{k}"] for k in ("t", "w", "b", "d", "lambda"))
        assert t.shape[1] % 256 != 0
        for r in range(t.shape[0]):
            _check_row(t[r], w[r], b[r], d[r], float(lam[r]))
            want, feasible = closed_form_lambda(t[r], w[r], b[r])
            room_min = np.where(w[r] == 0, np.inf, np.minimum(t[r], 1 - t[r]).astype(np.float64)).min()
            kinds.add("allzero" if not w[r].any() else "miss" if not feasible else "below" if want < room_min else "middle")
            kinds.add("cpos" if float(b[r]) > float(np.dot(w[r].astype(np.float64), t[r])) else "cneg")
    assert kinds == {"allzero", "miss", "below", "middle", "cpos", "cneg"}
    D = int(z["big_D"])
    for i, (salt, off) in enumerate(z["big_salt_offset"]):
        t, w, b = hashed_row(D, int(salt), float(off))
        want, _ = closed_form_lambda(t, w, b)
        assert abs(float(z["big_lambda"][i]) - want) <= 1e-9 * want
        up = (w > 0) if float(b) > float(np.dot(w.astype(np.float64), t)) else (w < 0)
        room = np.where(w == 0, 0.0, np.where(up, 1.0 - t.astype(np.float64), t.astype(np.float64)))
        d = np.where(up, 1.0, -1.0) * np.sign(np.abs(w)) * np.minimum(want, room)
        assert np.abs(d[::997] - z["big_d_stride997"][i]).max() <= 1e-7
    # the attack part: FAB's results count only inside eps, and the golden's points keep clear of it
    eps = float(z["eps"])
    for tag in ("fabt", "fab", "aa_fabt"):
        dist, fooled = z[f"{tag}_dist"], z[f"{tag}_fooled"]
        assert fooled.any() and not fooled.all()
        assert (dist[fooled] <= 0.9 * eps).all() and (dist[~fooled] == 0).all()
    assert np.array_equal(z["aa_std_fooled"], z["aa_std_y_adv"] != z["y"])
