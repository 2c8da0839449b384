"""Host-side anchor of tests/loss_cases.py (no GPU): the restatements the GPU tests of csrc/loss_kernels.hip compare against
reproduce what the reference itself recorded in tests/golden/, and the case builders keep the properties they promise."""
import numpy as np
import pytest
import torch

from tests import loss_cases as LC
from tests.helpers import load_golden

DLR_CLASSES = (3, 4, 5, 63, 64, 65, 127, 128, 129, 256, 257, 1000, 1024)


def test_dlr_restatements_reproduce_the_reference_golden_bit_for_bit():
    """fp32 on the CPU, as tests/golden/make_golden.py ran the reference: values and autograd gradients of both DLR forms."""
    z = load_golden("dlr_losses.npz")
    x, y, yt = (torch.from_numpy(z[k]) for k in ("logits", "y", "y_target"))
    val, grad = LC.grad_of_sum(LC.dlr_ref, x, y)
    assert np.array_equal(val.numpy(), z["dlr"]) and np.array_equal(grad.numpy(), z["dlr_grad"])
    val, grad = LC.grad_of_sum(LC.dlr_targeted_ref, x, y, yt)
    assert np.array_equal(val.numpy(), z["dlr_targeted"]) and np.array_equal(grad.numpy(), z["dlr_targeted_grad"])
    assert np.array_equal(LC.argmax_first(x), z["logits"].argmax(1))


def test_ce_and_l2_restatements_reproduce_the_reference_golden():
    """losses.npz (compute_loss of the reference, fp32) within the tolerances test_losses_vs_golden holds the kernels to."""
    z = load_golden("losses.npz")
    emb, e0, T, y = (torch.from_numpy(z[k]) for k in ("emb", "e0", "T", "y"))
    B = emb.shape[0]
    ce_val, ce_grad = LC.head_ce_ref(emb, T, y, 100.)
    logits = emb.double() @ (100. * T.double())
    val2, dlogits = LC.ce_ref(logits, y)                     # the per-element form agrees with autograd of F.cross_entropy
    np.testing.assert_allclose(val2.numpy(), ce_val.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose((dlogits @ (100. * T.double()).t()).numpy(), ce_grad.numpy(), rtol=1e-10, atol=1e-12)
    l2_val = LC.l2_ref(emb, e0)
    l2_grad = 2.0 * (emb.double() - e0.double())
    for name, val, grad in (("ce", ce_val, ce_grad), ("l2", l2_val, l2_grad)):
        np.testing.assert_allclose(val.numpy(), z[f"{name}_none"], rtol=2e-5, atol=1e-5)
        np.testing.assert_allclose(val.mean().numpy(), z[f"{name}_mean"], rtol=2e-5, atol=1e-5)
        np.testing.assert_allclose(grad.numpy(), z[f"{name}_none_grad"], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose((grad / B).numpy(), z[f"{name}_mean_grad"], rtol=2e-4, atol=2e-5)
    assert float(np.mean(LC.argmax_first(logits) == z["y"])) * 100 == float(z["acc"])


def test_cosine_restatement_is_torch_cosine_similarity_off_the_clamp():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(7, 65, generator=g), torch.randn(7, 65, generator=g)
    ref = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1, eps=1e-8)
    np.testing.assert_allclose(LC.cosine_ref(a, b).numpy(), ref.numpy(), rtol=1e-13, atol=0)
    a[2] = 0
    assert float(LC.cosine_ref(a, b)[2]) == 0.0


def _ranks(x, idx):
    """1-based rank of x[b, idx[b]] in its row (distinct values)."""
    return (x > x.gather(1, idx[:, None])).sum(1) + 1


@pytest.mark.parametrize("C", DLR_CLASSES)
def test_dlr_families_keep_their_promises(C):
    for B in (2, 9):
        for fam in LC.dlr_families(C):
            case = LC.dlr_case(fam, C, B, seed=C)
            again = LC.dlr_case(fam, C, B, seed=C)
            x, y, yt = case["x"], case["y"], case["y_target"]
            assert torch.equal(x, again["x"]) and torch.equal(y, again["y"]) and torch.equal(yt, again["y_target"])
            assert x.dtype == torch.float32 and x.shape == (B, C) and bool(torch.isfinite(x).all())
            assert bool(((y >= 0) & (y < C) & (yt >= 0) & (yt < C) & (y != yt)).all())
            top = x.argsort(dim=1, descending=True, stable=True)[:, :4]
            lanes = top % LC.LANES
            if fam == "one_lane":
                assert bool((lanes == lanes[:, :1]).all()) and bool((x.gather(1, top[:, 3:4]) > 15.0).all())
            elif fam == "two_two":
                assert bool((lanes[:, 0] == lanes[:, 2]).all()) and bool((lanes[:, 1] == lanes[:, 3]).all())
                assert bool((lanes[:, 0] != lanes[:, 1]).all())
            elif fam == "ends":
                assert bool((top[:, 0] == C - 1).all()) and bool((top[:, 1] == 0).all())
            elif fam == "ranks":
                want_y = [min(b % 5 + 1, C) for b in range(B)]
                assert _ranks(x, y).tolist() == want_y
                rt = _ranks(x, yt).tolist()
                assert all(1 <= r <= 4 for r in rt)
                if B == 9 and C >= 5:
                    assert set(rt) == {1, 2, 3, 4}
            elif fam == "ties":
                assert bool((x * 2 == (x * 2).round()).all())
                s = x.sort(dim=1, descending=True).values[:, :5]
                tied = [tuple(r + 1 for r in range(s.shape[1] - 1) if s[b, r] == s[b, r + 1]) for b in range(B)]
                assert all(len(t) in (1, 2) for t in tied)                      # one two-way tie, or the three-way one
                assert [len(t) == 2 for t in tied] == case["value_only"].tolist()
                if B == 9 and C >= 5:
                    assert {t for t in tied} == {(1,), (2,), (3,), (4,), (1, 2)}
                    inside = [bool(x[b, y[b]] == s[b, tied[b][0] - 1]) for b in range(B)]
                    for r in (1, 2, 3, 4):                                       # y inside and outside every tied pair
                        assert {inside[b] for b in range(B) if tied[b] == (r,)} == {True, False}
            if fam != "ties":
                assert not bool(case["value_only"].any()) and not case["ties"]


@pytest.mark.parametrize("C", (1, 2, 63, 64, 65, 1000, 1024))
def test_ce_families_keep_their_promises(C):
    for fam in LC.ce_families(C):
        x, y = LC.ce_case(fam, C, 9, seed=C)
        assert x.dtype == torch.float32 and x.shape == (9, C) and bool(((y >= 0) & (y < C)).all())
        if fam == "offset":
            assert not bool(torch.isfinite(torch.exp(x)).any())                 # expf(l) alone overflows ...
            assert bool(torch.isfinite(LC.ce_ref(x, y)[0]).all())               # ... the loss itself is ordinary
        elif fam == "dominant" and C > 1:
            assert bool((x[torch.arange(9), y][:, None] - x >= 40.0).sum(1).eq(C - 1).all())
        elif fam == "ties":
            first = torch.from_numpy(LC.argmax_first(x))
            assert bool((first < y).all()) and bool((x[torch.arange(9), y] == x.max(1).values).all())
        elif fam == "scaled":
            assert float(x.abs().max()) <= 100.0
