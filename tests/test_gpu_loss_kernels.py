"""The loss and head kernels (csrc/loss_kernels.hip) at every class-count regime, through the public C ABI of include/rvlm.h.

Every kernel here gives one 64-lane wave to a row, four rows to a block, and lane i reads elements i, i + 64, ...: the sweeps cross
C (or D) = 63 / 64 / 65, several elements per lane (C = 1000: the ImageNet regime), B not a multiple of 4 and B > 256 (the second
stride of the loss reduction).  Exact outputs (DLR and logit-difference values, L2 gradients, arg-max flags, zero patterns) are
compared bit for bit; the others against fp64 restatements (tests/loss_cases.py, anchored to the reference's recorded outputs by
tests/test_loss_host.py).  Every output is a view inside a sentinel-filled buffer whose guards are checked by value afterwards:
B = 9 leaves three idle waves in the last block, which must write nothing."""
import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from tests import loss_cases as LC
from tests.gpu_helpers import dev, st, lib, record, assert_elems

pytestmark = pytest.mark.gpu

GUARD = 64                       # guard rows (elements of a 1-D buffer) in front of and behind every output
SENT_F, SENT_U8 = -12345.0, 0xA5
U = 2.0 ** -23

# Bars against fp64.  Each is at most 3x the worst value seen over every case of its test on an MI355X (in the comment) and never
# above what the format allows (the cap, in brackets; u = 2^-23):
#   ce value [8 u max(1, max|logit|): the rounding of l - m and of m + log(sum) at the logits' magnitude], in units of
#       max(1, max|logit|) of the row; ce gradient [the same x gscale, absolute per element], in units of gscale max(1, max|logit|)
#   row sums (L2 value, cosine) [(D / 64 + 8) u of the sum of absolute terms], as a fraction of that cap
#   reduction (every loss scalar, the cosine mean) [(B / 256 + 8) u of the sum of absolute per-sample values], as a fraction of it
#   head products, per shape [a K-long ordered fp32 fma chain and the multiplication by alpha: (K / 2 + 1) u of the sum of absolute
#       terms <= (K / 2 + 1) sqrt(K) u of their L2 norm, the floor assert_elems is documented for]
#   d_emb of CE through a head, per shape [none relative to that floor: the error of p - onehot is absolute, 2 x 8 u x 100 per
#       logit gradient - the exponent is rounded at the logits' magnitude in the logits GEMM and in l - lse - and the floor shrinks
#       with a saturating softmax, (2, 64, 3) below; the test holds every element to that absolute cap as well: chain + softmax]
CE_CAP = 8 * U
BARS = {
    "ce_value": 4.0e-7,            # measured 1.46e-7 (C 63, B 300)
    "ce_grad": 2.5e-7,             # measured 9.3e-8 (C 2, B 300)
    "head_ce_value": CE_CAP,       # measured 3.7e-7 at (2, 64, 3), 1.6e-7 at C = 1000: 3x is above the cap, so the cap
    "l2_value": 0.45,              # measured 0.158 of the cap (D 64, B 300)
    "cosine": 0.35,                # measured 0.125 of the cap (D 1, B 300)
    "reduce": 0.28,                # measured 0.097 of the cap (the DLR scalar at C 128, B 9; 0.096 for L2 at B 300)
}


def row_cap(D):
    return (D / 64 + 8) * U


def chain_cap(K):
    return (K / 2 + 1) * K ** 0.5 * U


# (B, D, C): d_emb of CE through the head; measured 1.72e-4, 2.7e-6, 2.6e-6, 3.5e-6
HEAD_CE_BARS = {(2, 64, 3): 5.0e-4, (9, 512, 1000): 8.0e-6, (5, 768, 1000): 7.5e-6, (9, 1024, 1024): 1.0e-5}
# (B, D, C): (logits, backward); measured (worse of scale 1 and 100) 7.6e-7 / 2.8e-7, 4.3e-8 / 8.5e-8, 1.18e-6 / 4.3e-7, 1.28e-6 / 4.5e-7
HEAD_BARS = {(1, 512, 1000): (2.2e-6, 8.4e-7), (2, 64, 1): (1.2e-7, min(2.5e-7, chain_cap(1))), (9, 768, 1000): (3.5e-6, 1.3e-6),
             (5, 1024, 1024): (3.8e-6, 1.3e-6)}
assert all(f <= chain_cap(k[1]) and b <= chain_cap(k[2]) for k, (f, b) in HEAD_BARS.items())
assert max(BARS["ce_value"], BARS["ce_grad"], BARS["head_ce_value"]) <= CE_CAP and max(BARS["l2_value"], BARS["cosine"], BARS["reduce"]) <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# guarded buffers and the two entry points
# ---------------------------------------------------------------------------------------------------------------------------
class Fenced:
    """Output buffers of one call: each a view inside a larger sentinel-filled buffer; check() asserts the guards by value."""

    def __init__(self):
        self.bufs = []

    def new(self, name, shape, dtype=torch.float32, fill=SENT_F, init=None):
        rows = shape[0]
        buf = torch.full((rows + 2 * GUARD,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
        view = buf[GUARD:GUARD + rows]
        if init is not None:
            view.copy_(init)
        self.bufs.append((name, buf, rows, fill))
        return view

    def check(self, tag):
        for name, buf, rows, fill in self.bufs:
            assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + rows:] == fill).all()), f"{tag}: {name} overrun"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def loss_grad(kind, red, emb, ref, y, yt, C, scale, want=("per", "scalar", "d_emb", "pred"), tag=""):
    """rvlm_loss_grad on guarded outputs -> dict of the outputs asked for (on the device); scratch is guarded as well."""
    B, D = emb.shape
    f = Fenced()
    o = {}
    if "per" in want:
        o["per"] = f.new("per_sample", (B,))
    if "scalar" in want:
        o["scalar"] = f.new("loss_scalar", (1,))
    if "d_emb" in want:
        o["d_emb"] = f.new("d_emb", (B, D))
    if "pred" in want:
        o["pred"] = f.new("pred_eq", (B,), torch.uint8, SENT_U8)
    scratch = f.new("scratch", (B * C + D * C,)) if C else None
    rc = lib().rvlm_loss_grad(kind, red, emb.data_ptr(), ref.data_ptr(), L.ptr(y), L.ptr(yt), B, D, C, scale, L.ptr(o.get("per")),
                              L.ptr(o.get("scalar")), L.ptr(o.get("d_emb")), L.ptr(o.get("pred")), L.ptr(scratch), st())
    torch.cuda.synchronize()
    f.check(tag)
    if rc != L.RVLM_OK:                                       # a refused call has launched nothing
        for name, buf, rows, fill in f.bufs:
            assert bool((buf == fill).all()), f"{tag}: {name} written by a refused call"
    L.check(rc, tag)
    return o


def check_scalar(tag, scalar, per, red, worst):
    """The reduction kernel against the fp64 sum of its own input, the per-sample buffer (which every test holds to its
    reference separately): mean or sum per `red`, within the reduction bar."""
    B = per.shape[0]
    p = per.detach().cpu().double()
    scale = 1.0 / B if red == L.RED_MEAN else 1.0
    err = abs(float(scalar.cpu().double()[0]) - float(p.sum()) * scale) / max(float(p.abs().sum()) * scale, 1e-300)
    frac = err / ((B / 256 + 8) * U)
    assert frac <= BARS["reduce"], f"{tag}: scalar off by {err:.3e} of the summed magnitude ({frac:.2f} of the cap)"
    worst["reduce"] = max(worst.get("reduce", 0.0), frac)


_EYE = {}


def eye(C):
    if C not in _EYE:
        _EYE[C] = torch.eye(C, device=dev())
    return _EYE[C]


def gscale_of(red, B):
    return np.float32(1.0) / np.float32(B) if red == L.RED_MEAN else np.float32(1.0)


REDS = ((L.RED_MEAN, "mean"), (L.RED_NONE, "none"))


# ---------------------------------------------------------------------------------------------------------------------------
# a. DLR and DLR-targeted through the identity head: logits = emb and d_emb = d logits exactly
# ---------------------------------------------------------------------------------------------------------------------------
DLR_CLASSES = (3, 4, 5, 63, 64, 65, 127, 128, 129, 256, 257, 1000, 1024)
DLR_PARAMS = [(t, C) for t in (False, True) for C in DLR_CLASSES if C >= (4 if t else 3)]


def per_value_sums(x_row, g_row):
    """A row's gradient summed over the elements that hold the same logit value."""
    _, inv = np.unique(x_row, return_inverse=True)
    return np.bincount(inv, weights=g_row)


@pytest.mark.parametrize("B", [2, 9])
@pytest.mark.parametrize("targeted,C", DLR_PARAMS)
def test_dlr_kernels(targeted, C, B):
    """Values bit-equal to the fp32 restatement in the reference's operation order (tie rows included: the value does not depend on
    how a tie breaks); pred_eq by the first-index rule; the gradient against fp64 autograd of the restatement on the same fp32 logits
    at the bar test_dlr_loss_kernels_vs_reference_golden uses, and exactly 0 outside {y, y_target, the selected four}.  On tie rows
    the sort and the kernel may route gradient to different members of a tied pair: there it is compared summed per distinct logit
    value.  The three-way tie at the top (den = 1e-12) is checked for its value only."""
    kind = L.LOSS_DLR_TARGETED if targeted else L.LOSS_DLR
    worst = {}
    for fam in LC.dlr_families(C):
        case = LC.dlr_case(fam, C, B, seed=C)
        x, y, yt = case["x"], case["y"], case["y_target"]
        tag0 = f"{'dlr-t' if targeted else 'dlr'} C{C} B{B} {fam}"
        fn, args = (LC.dlr_targeted_ref, (y, yt)) if targeted else (LC.dlr_ref, (y,))
        val_ref = fn(x, *args)
        _, g64 = LC.grad_of_sum(fn, x.double(), *args)
        pred_ref = LC.argmax_first(x) == y.numpy()
        xs = x.sort(dim=1, descending=True).values
        allowed = x >= xs[:, 3 if C >= 4 else C - 1][:, None]        # the four selected indices (or a tied stand-in)
        allowed[torch.arange(B), y] = True
        if targeted:
            allowed[torch.arange(B), yt] = True
        xd, yd = x.to(dev()), y.to(dev())
        ytd = yt.to(dev()) if targeted else None
        for red, rname in REDS:
            tag = f"{tag0} {rname}"
            o = loss_grad(kind, red, xd, eye(C), yd, ytd, C, 1.0, tag=tag)
            assert torch.equal(bits(o["per"]), bits(val_ref)), \
                f"{tag}: value differs from the restatement: {o['per'].cpu().tolist()} vs {val_ref.tolist()}"
            assert np.array_equal(o["pred"].cpu().numpy().astype(bool), pred_ref), f"{tag}: pred_eq"
            got = o["d_emb"].cpu().double().numpy()
            ref = (g64 / (B if red == L.RED_MEAN else 1)).numpy()
            assert bool((got[~allowed.numpy()] == 0).all()), f"{tag}: gradient outside y, y_target and the selected four"
            for b in range(B):
                if case["value_only"][b]:
                    continue
                a, r = (per_value_sums(x[b].numpy(), v[b]) for v in (got, ref)) if case["ties"] else (got[b], ref[b])
                np.testing.assert_allclose(a, r, rtol=1e-6, atol=1e-7, err_msg=f"{tag} row {b}")
                worst["grad_x_tol"] = max(worst.get("grad_x_tol", 0.0), float((np.abs(a - r) / (1e-7 + 1e-6 * np.abs(r))).max()))
            check_scalar(tag, o["scalar"], o["per"], red, worst)
        # d_emb = NULL: the same values; per_sample = loss_scalar = NULL: the same gradient
        full = loss_grad(kind, L.RED_NONE, xd, eye(C), yd, ytd, C, 1.0, tag=tag0)
        vals = loss_grad(kind, L.RED_NONE, xd, eye(C), yd, ytd, C, 1.0, want=("per", "scalar", "pred"), tag=tag0 + " no d_emb")
        assert torch.equal(bits(vals["per"]), bits(full["per"])) and torch.equal(vals["pred"], full["pred"])
        assert torch.equal(bits(vals["scalar"]), bits(full["scalar"]))
        grad = loss_grad(kind, L.RED_NONE, xd, eye(C), yd, ytd, C, 1.0, want=("d_emb",), tag=tag0 + " gradient only")
        assert torch.equal(bits(grad["d_emb"]), bits(full["d_emb"]))
    record("loss_kernels_dlr", targeted=targeted, C=C, B=B, **worst)


def test_dlr_refusals():
    """checks.check_n_classes: DLR needs 3 logits, its targeted form 4 and a y_target; a refused call launches nothing."""
    y = torch.zeros(2, dtype=torch.int64, device=dev())
    yt = torch.ones(2, dtype=torch.int64, device=dev())
    for kind, C, tgt in ((L.LOSS_DLR, 2, None), (L.LOSS_DLR_TARGETED, 3, yt), (L.LOSS_DLR_TARGETED, 4, None)):
        x = torch.randn(2, C, device=dev())
        with pytest.raises(ValueError):
            loss_grad(kind, L.RED_NONE, x, eye(C), y, tgt, C, 1.0, tag=f"kind {kind} C{C}")


# ---------------------------------------------------------------------------------------------------------------------------
# b. cross entropy on given logits (rvlm_ce_logits) and through the identity head (rvlm_loss_grad)
# ---------------------------------------------------------------------------------------------------------------------------
def ce_logits(x, y, red, in_place, tag):
    B, C = x.shape
    f = Fenced()
    per, scalar = f.new("per_sample", (B,)), f.new("loss_scalar", (1,))
    pred = f.new("pred_eq", (B,), torch.uint8, SENT_U8)
    if in_place:
        src = out = f.new("logits", (B, C), init=x)
    else:
        src, out = x.clone(), f.new("d_logits", (B, C))
    L.check(lib().rvlm_ce_logits(src.data_ptr(), y.data_ptr(), B, C, red, per.data_ptr(), scalar.data_ptr(), out.data_ptr(),
                                 pred.data_ptr(), st()), tag)
    torch.cuda.synchronize()
    f.check(tag)
    if not in_place:
        assert torch.equal(bits(src), bits(x)), f"{tag}: the input logits changed"
    return dict(per=per, scalar=scalar, d=out, pred=pred)


def check_ce(tag, o, x, y, val_ref, g_ref, red, worst, vkey="ce_value", gkey="ce_grad"):
    """per-sample value and per-element gradient against fp64, in units of max(1, max|logit|) of the row (x gscale)."""
    B = x.shape[0]
    mag = x.double().abs().max(dim=1).values.clamp_min(1.0)
    e_val = float(((o["per"].cpu().double() - val_ref).abs() / mag).max())
    assert e_val <= BARS[vkey], f"{tag}: value off by {e_val:.3e} max(1, max|logit|) > {BARS[vkey]:.1e}"
    worst[vkey] = max(worst.get(vkey, 0.0), e_val)
    if g_ref is not None:
        e_g = float(((o["d"].cpu().double() * (B if red == L.RED_MEAN else 1) - g_ref).abs() / mag[:, None]).max())
        assert e_g <= BARS[gkey], f"{tag}: gradient off by {e_g:.3e} gscale max(1, max|logit|) > {BARS[gkey]:.1e}"
        worst[gkey] = max(worst.get(gkey, 0.0), e_g)


@pytest.mark.parametrize("B", [1, 2, 9, 300])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 1000, 1024])
def test_ce_kernel(C, B):
    """Value and gradient per element against fp64, pred_eq by the first-index rule, the scalar under both reductions, on given
    logits (in place and out of place) and through rvlm_loss_grad with the identity head (B > 1: the reference's assert)."""
    worst = {}
    for fam in LC.ce_families(C):
        x, y = LC.ce_case(fam, C, B, seed=C)
        val_ref, g_ref = LC.ce_ref(x, y)
        pred_ref = LC.argmax_first(x) == y.numpy()
        if fam == "ties":
            assert not pred_ref.any()
        xd, yd = x.to(dev()), y.to(dev())
        for red, rname in REDS:
            runs = [("in place", ce_logits(xd, yd, red, True, f"ce C{C} B{B} {fam} {rname} in place")),
                    ("out of place", ce_logits(xd, yd, red, False, f"ce C{C} B{B} {fam} {rname} out of place"))]
            if B > 1:
                o = loss_grad(L.LOSS_CE, red, xd, eye(C), yd, None, C, 1.0, tag=f"ce C{C} B{B} {fam} {rname} identity head")
                runs.append(("identity head", dict(per=o["per"], scalar=o["scalar"], d=o["d_emb"], pred=o["pred"])))
            for how, o in runs:
                tag = f"ce C{C} B{B} {fam} {rname} {how}"
                check_ce(tag, o, x, y, val_ref, g_ref, red, worst)
                assert np.array_equal(o["pred"].cpu().numpy().astype(bool), pred_ref), f"{tag}: pred_eq"
                check_scalar(tag, o["scalar"], o["per"], red, worst)
            assert torch.equal(bits(runs[0][1]["d"]), bits(runs[1][1]["d"])) and torch.equal(bits(runs[0][1]["per"]), bits(runs[1][1]["per"]))
    record("loss_kernels_ce", C=C, B=B, **worst)


# ---------------------------------------------------------------------------------------------------------------------------
# c. cross entropy through a real head: the two fp32 GEMMs inside rvlm_loss_grad at M = 2, 5, 9 and K = 1000
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,C", list(HEAD_CE_BARS))
def test_ce_through_a_real_head(B, D, C):
    emb, T, y = LC.head_case(B, D, C)
    val_ref, g_ref = LC.head_ce_ref(emb, T, y, 100.0)
    logits = emb.double() @ (100.0 * T.double())
    _, dl = LC.ce_ref(logits, y)
    S = 100.0 * T.double()
    floor = torch.sqrt((dl ** 2) @ (S ** 2).t())                          # L2 norm of the C terms of every d_emb element
    abs_cap = (C / 2 + 1) * U * (dl.abs() @ S.abs().t()) + 2 * CE_CAP * 100 * S.abs().sum(dim=1)[None, :]
    pred_ref = LC.argmax_first(logits) == y.numpy()
    top2 = logits.topk(2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3                  # an arg-max fp32 logits cannot flip
    worst = {}
    for red, rname in REDS:
        tag = f"head ce B{B} D{D} C{C} {rname}"
        o = loss_grad(L.LOSS_CE, red, emb.to(dev()), T.to(dev()), y.to(dev()), None, C, 100.0, tag=tag)
        check_ce(tag, dict(per=o["per"]), logits, y, val_ref, None, red, worst, vkey="head_ce_value")
        s = B if red == L.RED_MEAN else 1
        w = assert_elems(f"d_emb {tag}", o["d_emb"].cpu() * s, g_ref, floor, HEAD_CE_BARS[B, D, C])
        assert bool(((o["d_emb"].cpu().double() * s - g_ref).abs() <= abs_cap).all()), f"{tag}: d_emb beyond what fp32 allows"
        worst["head_ce_d_emb"] = max(worst.get("head_ce_d_emb", 0.0), w)
        assert np.array_equal(o["pred"].cpu().numpy().astype(bool), pred_ref), f"{tag}: pred_eq"
        check_scalar(tag, o["scalar"], o["per"], red, worst)
    record("loss_kernels_head_ce", B=B, D=D, C=C, **worst)


# ---------------------------------------------------------------------------------------------------------------------------
# d. L2
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 9, 300])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 512, 768, 1000, 1024])
def test_l2_kernel(D, B):
    """d_emb bit-equal to fp32 (2 (e - r)) gscale, gscale = float32(1 / B) or 1: the doubling is exact and both products round
    once; the per-sample value against fp64 as a row sum; row 0 has e == r (loss and gradient exactly 0)."""
    g = torch.Generator().manual_seed(7000 + 31 * D + B)
    e, r = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    r[0] = e[0]
    val_ref = LC.l2_ref(e, r)
    worst = {}
    for red, rname in REDS:
        tag = f"l2 D{D} B{B} {rname}"
        o = loss_grad(L.LOSS_L2, red, e.to(dev()), r.to(dev()), None, None, 0, 1.0, want=("per", "scalar", "d_emb"), tag=tag)
        g_ref = (2.0 * (e - r)) * torch.tensor(gscale_of(red, B))
        assert torch.equal(bits(o["d_emb"]), bits(g_ref)), f"{tag}: gradient is not the two single roundings"
        per = o["per"].cpu().double()
        assert float(per[0]) == 0.0
        frac = float(((per - val_ref).abs() / val_ref.clamp_min(1e-300)).max()) / row_cap(D)
        assert frac <= BARS["l2_value"], f"{tag}: value off by {frac:.2f} of the row-sum cap {row_cap(D):.2e}"
        worst["l2_value"] = max(worst.get("l2_value", 0.0), frac)
        check_scalar(tag, o["scalar"], o["per"], red, worst)
        only = loss_grad(L.LOSS_L2, red, e.to(dev()), r.to(dev()), None, None, 0, 1.0, want=("d_emb",), tag=tag + " gradient only")
        assert torch.equal(bits(only["d_emb"]), bits(g_ref))
    record("loss_kernels_l2", D=D, B=B, **worst)


def test_l2_refuses_a_batch_of_one():
    e = torch.randn(1, 64, device=dev())
    with pytest.raises(ValueError):
        loss_grad(L.LOSS_L2, L.RED_NONE, e, e.clone(), None, None, 0, 1.0, want=("per", "scalar", "d_emb"), tag="l2 B1")


# ---------------------------------------------------------------------------------------------------------------------------
# e. logit difference (FAB-T)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 64, 65, 1000])
def test_logit_diff_kernel(C):
    B = 9
    g = torch.Generator().manual_seed(8000 + C)
    x = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    y[::2] = x[::2].argmax(1)
    yt = torch.where(torch.arange(B) == 4, y, (y + 1 + torch.randint(0, C - 1, (B,), generator=g)) % C)   # row 4: y == y_target
    assert bool((yt[torch.arange(B) != 4] != y[torch.arange(B) != 4]).all())
    u = torch.arange(B)
    val_ref = -(x[u, y] - x[u, yt])
    pred_ref = LC.argmax_first(x) == y.numpy()
    for red, rname in REDS:
        tag = f"logit-diff C{C} {rname}"
        o = loss_grad(L.LOSS_LOGIT_DIFF, red, x.to(dev()), eye(C), y.to(dev()), yt.to(dev()), C, 1.0, tag=tag)
        assert torch.equal(bits(o["per"]), bits(val_ref)), tag
        gs = torch.tensor(gscale_of(red, B))
        g_ref = torch.zeros(B, C)
        g_ref[u, yt] += gs
        g_ref[u, y] -= gs
        got = o["d_emb"].cpu()
        assert torch.equal(got, g_ref), f"{tag}: gradient entries are not exactly -gscale, +gscale, 0"
        assert bool((got[4] == 0).all())
        assert np.array_equal(o["pred"].cpu().numpy().astype(bool), pred_ref), f"{tag}: pred_eq"
        check_scalar(tag, o["scalar"], o["per"], red, {})


# ---------------------------------------------------------------------------------------------------------------------------
# f. rvlm_argmax_eq
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["randn", "ends", "equal", "minus_inf_head"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 1000])
def test_argmax_eq(C, family):
    """Exactly numpy's first-index arg-max: the largest value in the last lane's last element, a row of equal values (index 0) and
    a row whose first 64 entries are -inf (all of it when C <= 64: still index 0)."""
    B = 9
    g = torch.Generator().manual_seed(9000 + C)
    x = torch.randn(B, C, generator=g) * 3
    if family == "ends":
        x[:, C - 1] = 40.0
        x[:, 0] = 36.5 if C > 1 else 40.0
    elif family == "equal":
        x[:] = 1.25
    elif family == "minus_inf_head":
        x[:, :64] = float("-inf")
    first = LC.argmax_first(x)
    y = torch.randint(0, C, (B,), generator=g)
    y[::2] = torch.from_numpy(first)[::2]
    f = Fenced()
    out = f.new("out", (B,), torch.uint8, SENT_U8)
    xd, yd = x.to(dev()), y.to(dev())
    L.check(lib().rvlm_argmax_eq(xd.data_ptr(), yd.data_ptr(), B, C, out.data_ptr(), st()))
    torch.cuda.synchronize()
    f.check(f"argmax_eq C{C} {family}")
    assert np.array_equal(out.cpu().numpy(), (first == y.numpy()).astype(np.uint8)), (C, family, first, y)


# ---------------------------------------------------------------------------------------------------------------------------
# g. rvlm_cosine_rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 9, 300])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 512, 768])
def test_cosine_rows(D, B):
    """a.b / sqrt(max(|a|^2 |b|^2, 1e-16)) per row and its mean: an all-zero `a` row gives exactly 0.0 (not NaN), rows scaled by 1e-6
    sit on the clamp; off the clamp it is also the installed torch's F.cosine_similarity in fp64."""
    g = torch.Generator().manual_seed(10000 + 31 * D + B)
    a, b = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    plain = torch.ones(B, dtype=torch.bool)
    if B >= 2:
        a[1] = 0.0
        plain[1] = False
    if B >= 9:
        a[2] *= 1e-6
        b[2] *= 1e-6                              # |a|^2 |b|^2 ~ D^2 1e-24 < 1e-16: the clamp is active
        a[3] *= 1e-6                              # small, but off the clamp for D > 1 ...
        plain[2] = False
        plain[3] = bool(float((a[3].double() ** 2).sum() * (b[3].double() ** 2).sum()) > 4e-16)
    ref = LC.cosine_ref(a, b)
    scale = (a.double() * b.double()).abs().sum(1) / torch.sqrt(torch.clamp((a.double() ** 2).sum(1) * (b.double() ** 2).sum(1), min=1e-16))
    f = Fenced()
    out, mean = f.new("out_per_row", (B,)), f.new("out_mean", (1,))
    ad, bd = a.to(dev()), b.to(dev())
    L.check(lib().rvlm_cosine_rows(ad.data_ptr(), bd.data_ptr(), B, D, out.data_ptr(), mean.data_ptr(), st()))
    torch.cuda.synchronize()
    tag = f"cosine D{D} B{B}"
    f.check(tag)
    got = out.cpu().double()
    if B >= 2:
        assert float(got[1]) == 0.0, f"{tag}: the all-zero row gives {float(got[1])!r}"
    worst = {}
    frac = float(((got - ref).abs() / scale.clamp_min(1e-300)).max()) / row_cap(D)
    assert frac <= BARS["cosine"], f"{tag}: off by {frac:.2f} of the row-sum cap {row_cap(D):.2e}"
    worst["cosine"] = frac
    tref = torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1, eps=1e-8)
    frac_t = float(((got - tref).abs() / scale.clamp_min(1e-300))[plain].max()) / row_cap(D)
    assert frac_t <= BARS["cosine"], f"{tag}: off torch's cosine_similarity by {frac_t:.2f} of the row-sum cap"
    check_scalar(tag, mean, out, L.RED_MEAN, worst)
    only = Fenced()
    out2 = only.new("out_per_row", (B,))
    L.check(lib().rvlm_cosine_rows(ad.data_ptr(), bd.data_ptr(), B, D, out2.data_ptr(), None, st()))
    torch.cuda.synchronize()
    only.check(tag + " no mean")
    assert torch.equal(bits(out2), bits(out))
    record("loss_kernels_cosine", D=D, B=B, **worst)


# ---------------------------------------------------------------------------------------------------------------------------
# h. the zero-shot head: logits = (emb @ T) * scale and d_emb = (d_logits * scale) @ T^T
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("B,D,C", list(HEAD_BARS))
def test_head_logits_and_backward(B, D, C, scale):
    emb, T, _ = LC.head_case(B, D, C, seed=1)
    dl = torch.randn(B, C, generator=torch.Generator().manual_seed(11000 + C + B))
    e64, T64, dl64 = emb.double(), T.double(), dl.double()
    f = Fenced()
    logits, d_emb = f.new("logits", (B, C)), f.new("d_emb", (B, D))
    ed, Td, dld = emb.to(dev()), T.to(dev()), dl.to(dev())
    L.check(lib().rvlm_head_logits(ed.data_ptr(), Td.data_ptr(), B, D, C, scale, logits.data_ptr(), st()))
    L.check(lib().rvlm_head_logits_bwd(dld.data_ptr(), Td.data_ptr(), B, D, C, scale, d_emb.data_ptr(), st()))
    torch.cuda.synchronize()
    tag = f"B{B} D{D} C{C} scale {scale:g}"
    f.check(tag)
    w_f = assert_elems(f"head logits {tag}", logits.cpu(), (e64 @ T64) * scale, scale * torch.sqrt((e64 ** 2) @ (T64 ** 2)),
                       HEAD_BARS[B, D, C][0])
    w_b = assert_elems(f"head backward {tag}", d_emb.cpu(), (dl64 * scale) @ T64.t(), scale * torch.sqrt((dl64 ** 2) @ (T64 ** 2).t()),
                       HEAD_BARS[B, D, C][1])
    record("loss_kernels_head", B=B, D=D, C=C, scale=scale, head_logits=w_f, head_logits_bwd=w_b)


# ---------------------------------------------------------------------------------------------------------------------------
# the label check of compute_loss("ce", ...): an out-of-range label never reaches the kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["C", "-1"])
def test_compute_loss_ce_refuses_labels_outside_the_classes(bad):
    emb, T, y = LC.head_case(4, 64, 7)
    emb, T, y = emb.to(dev()), T.to(dev()), y.to(dev())
    y[2] = 7 if bad == "C" else -1
    for red in ("mean", "none"):
        with pytest.raises(IndexError):
            R.compute_loss("ce", emb, y, emb, 100., T, red)
        with pytest.raises(IndexError):
            R.ComputeLossWrapper(emb, T, red, "ce", 100.)(emb, y)
    y[2] = 6                                                   # the largest label that is in range still runs
    assert bool(torch.isfinite(R.compute_loss("ce", emb, y, emb, 100., T, "none")).all())
