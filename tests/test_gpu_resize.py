"""The in-model bicubic resizer on the GPU: the standalone kernels against float64 F.interpolate on the CPU, the adjoint as an
adjoint, the two forms fused into the patch embedding against resize-then-im2col, the engine at a reduced input size against the
CPU oracle composed with F.interpolate, and the attack routes (APGD / APGD-T / FAB-T / AutoAttack / pgd) at the images' own
resolution against the generic route and against what the reference produced (tests/golden/attacks_resize_tiny.npz)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from oracle import vit_ref as V
from tests.gpu_helpers import dev, cos_sim, rel_max, st, lib
from tests.helpers import load_golden, weights_digest

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

SIZE_PAIRS = [((32, 32), (224, 224)), ((96, 96), (224, 224)), ((12, 12), (32, 32)), ((224, 224), (224, 224)), ((5, 5), (13, 13)),
              ((7, 19), (30, 11))]          # the last: both directions at once, non-square


def interp64(x, size):
    return F.interpolate(x.double().cpu(), size=size, mode="bicubic", align_corners=False)


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


def make_engine(cfg, w, precision, max_batch=8, **kw):
    return R.VitEngine(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch, **kw)


def f3(v):
    return (C.c_float * 3)(*v)


# ---------------------------------------------------------------------------------------------- standalone kernels
@pytest.mark.parametrize("in_hw,out_hw", SIZE_PAIRS)
@pytest.mark.parametrize("B,Cn", [(1, 1), (3, 3), (1, 3), (3, 1)])
def test_resize_forward_vs_float64_interpolate(in_hw, out_hw, B, Cn):
    g = torch.Generator().manual_seed(B * 10 + Cn)
    x = torch.rand(B, Cn, *in_hw, generator=g)
    y = R.BicubicResize(out_hw)(x.to(dev()))
    ref = interp64(x, out_hw)
    assert y.shape == ref.shape and y.dtype == torch.float32
    assert float((y.double().cpu() - ref).abs().max()) <= 2e-6
    if in_hw == out_hw:
        assert torch.equal(y.cpu(), x)


def test_resize_does_not_clamp_the_overshoot():
    x = torch.zeros(1, 1, 8, 8)
    x[..., :, 4:] = 1.0                                     # a step edge: the cubic rings on both sides of it
    y = R.BicubicResize(56)(x.to(dev())).cpu()
    ref = interp64(x, (56, 56))
    assert float(ref.min()) < -0.05 and float(ref.max()) > 1.05
    assert float((y.double() - ref).abs().max()) <= 2e-6
    assert float(y.min()) < -0.05 and float(y.max()) > 1.05


@pytest.mark.parametrize("in_hw,out_hw", SIZE_PAIRS)
def test_resize_adjoint_is_the_adjoint(in_hw, out_hw):
    g = torch.Generator().manual_seed(3)
    B, Cn = 3, 3
    x = torch.rand(B, Cn, *in_hw, generator=g)
    gy = torch.randn(B, Cn, *out_hw, generator=g)
    xd = x.to(dev()).requires_grad_(True)
    y = R.BicubicResize(out_hw)(xd)
    (gx,) = torch.autograd.grad(y, xd, gy.to(dev()))
    (gx2,) = torch.autograd.grad(R.BicubicResize(out_hw)(xd), xd, gy.to(dev()))
    assert torch.equal(gx, gx2), "the gather sums in a fixed order: the same bits every run"
    # <R x, gy> = <x, R^T gy>
    lhs = float((y.detach().double().cpu() * gy.double()).sum())
    rhs = float((x.double() * gx.double().cpu()).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), float(y.detach().abs().double().cpu().flatten() @ gy.abs().double().flatten()) * 1e-1)
    # ... and CPU autograd of F.interpolate
    xr = x.double().requires_grad_(True)
    (gref,) = torch.autograd.grad(F.interpolate(xr, size=out_hw, mode="bicubic", align_corners=False), xr, gy.double())
    assert float((gx.double().cpu() - gref).abs().max()) <= 2e-6 * max(1.0, float(gref.abs().max()))


def test_bicubic_resize_finite_differences_and_refusals():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 6, 7, generator=g).to(dev())
    cot = torch.randn(2, 3, 15, 10, generator=g).to(dev())
    r = R.BicubicResize((15, 10))
    xg = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad((r(xg) * cot).sum(), xg)
    # the operator is linear: a central difference is exact up to fp32 rounding of the two sums
    h = 0.25
    for (b, c, i, j) in [(0, 0, 0, 0), (1, 2, 5, 6), (0, 1, 3, 2), (1, 0, 0, 6), (0, 2, 5, 0)]:
        e = torch.zeros_like(x)
        e[b, c, i, j] = h
        fd = float(((r(x + e).double() - r(x - e).double()) * cot.double()).sum()) / (2 * h)
        assert abs(fd - float(gx[b, c, i, j])) <= 2e-5 * max(1.0, abs(fd)), (b, c, i, j, fd, float(gx[b, c, i, j]))
    with pytest.raises(TypeError):
        r(x.half())
    with pytest.raises(ValueError):
        r(x[0])
    with pytest.raises(L.RvlmError):
        r(x.cpu())
    # a strided view is made contiguous, not misread
    xt = torch.rand(2, 3, 7, 6, generator=g).to(dev()).transpose(2, 3)
    assert torch.equal(r(xt), r(xt.contiguous()))


# ---------------------------------------------------------------------------------------------- fused hooks
@pytest.mark.parametrize("in_hw,img,P", [((32, 32), 224, 14), ((96, 96), 224, 32), ((12, 12), 32, 8), ((20, 9), 32, 16)])
@pytest.mark.parametrize("with_delta", [False, True])
def test_fused_front_end_equals_resize_then_im2col(in_hw, img, P, with_delta):
    g = torch.Generator().manual_seed(7)
    B = 3
    x = torch.rand(B, 3, *in_hw, generator=g).to(dev())
    d = ((torch.rand(B, 3, *in_hw, generator=g) - 0.5) * 0.06).to(dev()) if with_delta else None
    K = 3 * P * P
    Kpad = (K + 63) // 64 * 64
    rows = B * (img // P) ** 2
    mean, std = f3(R.CLIP_MEAN), f3(R.CLIP_STD)
    big = R.BicubicResize((img, img))(x + d if with_delta else x)
    for bf16 in (0, 1):
        dt = torch.bfloat16 if bf16 else torch.float32
        a_ref = torch.full((rows, Kpad), 7.0, dtype=dt, device=dev())
        a_got = torch.full((rows, Kpad), 9.0, dtype=dt, device=dev())
        L.check(lib().rvlm_k_im2col_normalize(big.data_ptr(), None, B, img, P, mean, std, a_ref.data_ptr(), Kpad, Kpad, bf16, st()))
        L.check(lib().rvlm_k_resize_im2col_normalize(x.data_ptr(), L.ptr(d), B, in_hw[0], in_hw[1], img, P, mean, std,
                                                     a_got.data_ptr(), Kpad, Kpad, bf16, st()))
        torch.cuda.synchronize()
        # the same operations in the same order (x + delta, four row cubics, the column cubic, Normalize): the same bits
        assert torch.equal(a_got, a_ref), float((a_got.float() - a_ref.float()).abs().max())
        assert float(a_got[:, K:].abs().max()) == 0.0 if Kpad > K else True


@pytest.mark.parametrize("in_hw,img,P", [((32, 32), 224, 14), ((96, 96), 224, 32), ((12, 12), 32, 8), ((20, 9), 32, 16)])
def test_fused_tail_equals_col2im_then_adjoint(in_hw, img, P):
    g = torch.Generator().manual_seed(8)
    B = 3
    K = 3 * P * P
    lda = (K + 63) // 64 * 64
    rows = B * (img // P) ** 2
    std = f3(R.CLIP_STD)
    dA = torch.randn(rows, lda, generator=g).to(dev())
    for bf16 in (0, 1):
        src = dA.to(torch.bfloat16).contiguous() if bf16 else dA
        full = torch.empty(B, 3, img, img, device=dev())
        L.check(lib().rvlm_k_col2im_grad(src.data_ptr(), lda, bf16, B, img, P, std, full.data_ptr(), st()))
        ref = torch.empty(B, 3, *in_hw, device=dev())
        L.check(lib().rvlm_resize_bicubic_adjoint(full.data_ptr(), B * 3, in_hw[0], in_hw[1], img, img, ref.data_ptr(), st()))
        got = torch.full((B, 3, *in_hw), 5.0, device=dev())
        got2 = torch.empty_like(got)
        for out in (got, got2):
            L.check(lib().rvlm_k_col2im_resize_grad(src.data_ptr(), lda, bf16, B, in_hw[0], in_hw[1], img, P, std, out.data_ptr(), st()))
        torch.cuda.synchronize()
        assert torch.equal(got, got2)
        # 1 / std once per low-resolution pixel instead of once per patch element: equal to fp32 rounding of the sums
        assert rel_max(got.cpu(), ref.cpu()) < 2e-6
        # ... and against float64: R^T (dA0 / std) R
        g64 = torch.empty(B, 3, img, img, dtype=torch.float64)
        s64 = src.double().cpu()[:, :K].reshape(B, img // P, img // P, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, img, img)
        g64 = s64 / torch.tensor(R.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
        xr = torch.zeros(B, 3, *in_hw, dtype=torch.float64, requires_grad=True)
        (want,) = torch.autograd.grad(F.interpolate(xr, size=(img, img), mode="bicubic", align_corners=False), xr, g64)
        assert rel_max(got.cpu(), want) < 2e-6


def test_hooks_refuse_bad_arguments():
    x = torch.zeros(1, 3, 8, 8, device=dev())
    a = torch.zeros(16, 192, device=dev())
    mean, std = f3(R.CLIP_MEAN), f3(R.CLIP_STD)
    assert lib().rvlm_k_resize_im2col_normalize(x.data_ptr(), None, 1, 8, 8, 32, 7, mean, std, a.data_ptr(), 192, 192, 0, st()) == L.RVLM_ERR_ARG
    assert lib().rvlm_k_resize_im2col_normalize(x.data_ptr(), None, 1, 0, 8, 32, 8, mean, std, a.data_ptr(), 192, 192, 0, st()) == L.RVLM_ERR_ARG
    assert lib().rvlm_k_col2im_resize_grad(a.data_ptr(), 100, 0, 1, 8, 8, 32, 8, std, x.data_ptr(), st()) == L.RVLM_ERR_ARG
    assert lib().rvlm_resize_bicubic(x.data_ptr(), 0, 8, 8, 16, 16, a.data_ptr(), st()) == L.RVLM_ERR_ARG
    assert lib().rvlm_resize_bicubic_adjoint(None, 3, 8, 8, 16, 16, a.data_ptr(), st()) == L.RVLM_ERR_ARG


# ---------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_native_input_size_is_bit_identical_to_a_fresh_handle(precision):
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    g = torch.Generator().manual_seed(1)
    B = 4
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g).to(dev())
    d0 = ((torch.rand(x.shape, generator=g) - 0.5) * (8 / 255)).to(dev())
    T = torch.randn(cfg.out_dim, 10, generator=g)
    T = (T / T.norm(dim=0, keepdim=True)).to(dev())
    y = torch.randint(0, 10, (B,), generator=g).to(dev())

    def run(eng):
        emb = eng.forward(x, d0, True, save=True)
        gx = eng.backward_input(torch.ones_like(emb))
        e2, per, sc, g2 = eng.fwd_inputgrad(x, d0, "ce", "mean", T, y, True)
        xa, flags, tr = eng.pgd_run(x, d0, "ce", "mean", T, y, True, 4 / 255, 5, 1 / 255, 0.9, "max", want_trace=True)
        return emb, gx, e2, per, sc, g2, xa, flags, tr
    fresh = make_engine(cfg, w, precision)
    want = run(fresh)
    fresh.close()
    eng = make_engine(cfg, w, precision)
    eng.set_input_size(40, 56)                      # through a resized geometry and back
    assert eng.input_size == (40, 56)
    eng.forward(x[:, :, :40, :56].contiguous(), None, True)
    eng.set_input_size(cfg.image_size, cfg.image_size)
    got = run(eng)
    eng.set_input_size(0, 0)
    assert eng.input_size == (cfg.image_size, cfg.image_size)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    eng.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg,in_hw,B", [(V.VIT_TINY, (16, 16), 4), (V.VIT_TINY, (12, 12), 4), (V.VIT_TINY2, (32, 32), 3),
                                         (V.VIT_TINY2, (50, 77), 3)])
def test_engine_at_reduced_input_vs_oracle(cfg, in_hw, B, precision):
    w = V.init_weights(cfg, seed=9)
    ref = V.ClipVisionModelRef(cfg, w).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, *in_hw, generator=g)
    cot = torch.randn(B, cfg.out_dim, generator=g)
    size = (cfg.image_size, cfg.image_size)
    xr = x.clone().requires_grad_(True)
    e_ref = ref(F.interpolate(xr, size=size, mode="bicubic", align_corners=False), True)
    (g_ref,) = torch.autograd.grad((e_ref * cot).sum(), xr)
    eng = make_engine(cfg, w, precision)
    with pytest.raises(ValueError):
        eng.forward(x.to(dev()), None, True)                   # still at the model's own size
    eng.set_input_size(*in_hw)
    emb = eng.forward(x.to(dev()), None, True, save=True)
    gx = eng.backward_input(cot.to(dev()))
    assert gx.shape == x.shape
    if precision == "fp32":
        assert rel_max(emb.cpu(), e_ref.detach()) < 1e-4
        assert rel_max(gx.cpu(), g_ref) < 1e-3
    else:
        assert cos_sim(emb.cpu(), e_ref.detach()) > 0.999
        assert cos_sim(gx.cpu(), g_ref) > 0.98
        assert np.mean(np.sign(gx.cpu().numpy()) == np.sign(g_ref.numpy())) > 0.9
    # delta lives in the small space and is added before the resize
    d = (torch.rand_like(x) - 0.5) * 0.03
    assert torch.equal(eng.forward(x.to(dev()), d.to(dev()), True), eng.forward((x + d).to(dev()), None, True))
    # the fused front end == BicubicResize, then the engine at its own size (the same bits: same operations, same order)
    e_fused = eng.forward(x.to(dev()), None, True)
    eng.set_input_size(0, 0)
    e_two = eng.forward(R.BicubicResize(size)(x.to(dev())), None, True)
    assert torch.equal(e_fused, e_two)
    eng.close()


def test_input_size_state_and_error_codes():
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=9)
    x = torch.rand(3, 3, 16, 16).to(dev())
    eng = make_engine(cfg, w, "fp32")
    h = eng._h
    assert lib().rvlm_vit_set_input_size(h, 33, 16) == L.RVLM_ERR_UNSUPPORTED         # in > image_size
    assert lib().rvlm_vit_set_input_size(h, 16, 64) == L.RVLM_ERR_UNSUPPORTED
    assert lib().rvlm_vit_set_input_size(h, -1, 16) == L.RVLM_ERR_ARG
    assert lib().rvlm_vit_set_input_size(h, 0, 16) == L.RVLM_ERR_ARG
    with pytest.raises(NotImplementedError):
        eng.set_input_size(48, 48)
    assert eng.input_size == (32, 32)
    # set_input_size between forward and backward: no mixing of two geometries
    eng.set_input_size(16, 16)
    emb = eng.forward(x, None, True, save=True)
    eng.set_input_size(12, 12)
    g = torch.empty(3, 3, 12, 12, device=dev())
    assert lib().rvlm_vit_backward_input(h, emb.data_ptr(), 3, g.data_ptr(), st()) == L.RVLM_ERR_STATE
    eng.set_input_size(16, 16)
    assert lib().rvlm_vit_backward_input(h, emb.data_ptr(), 3, g.data_ptr(), st()) == L.RVLM_ERR_STATE
    xg = x.clone().requires_grad_(True)
    out = R.ClipVisionModel(eng)(xg, True)
    eng.set_input_size(12, 12)
    with pytest.raises(RuntimeError):
        out.sum().backward()
    # the context manager restores on exceptions
    eng.set_input_size(0, 0)
    with pytest.raises(KeyError):
        with eng.input_size_of(16, 16):
            assert eng.input_size == (16, 16)
            raise KeyError("x")
    assert eng.input_size == (32, 32)
    eng.close()
    # a trainable handle runs at the model's own resolution only
    tr = make_engine(cfg, w, "fp32", trainable=True)
    assert lib().rvlm_vit_set_input_size(tr._h, 16, 16) == L.RVLM_ERR_UNSUPPORTED
    assert lib().rvlm_vit_set_input_size(tr._h, 32, 32) == L.RVLM_OK and lib().rvlm_vit_set_input_size(tr._h, 0, 0) == L.RVLM_OK
    tr.close()


def test_two_handle_entries_need_one_input_size():
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=9)
    g = torch.Generator().manual_seed(2)
    B = 4
    x = torch.rand(B, 3, 16, 16, generator=g).to(dev())
    eng = make_engine(cfg, w, "bf16+x3fwd-first")
    ref = V.ClipVisionModelRef(cfg, w).eval()
    emb = torch.empty(B, cfg.out_dim, device=dev())
    gx = torch.empty_like(x)
    L.check(lib().rvlm_vit_set_input_size(eng._h32, 16, 16))                  # one handle of the pair only
    assert lib().rvlm_vit_forward_for(eng._h32, eng._h, x.data_ptr(), None, B, 1, emb.data_ptr(), st()) == L.RVLM_ERR_STATE
    assert lib().rvlm_vit_backward_input_from(eng._h, eng._h32, emb.data_ptr(), B, gx.data_ptr(), st()) == L.RVLM_ERR_STATE
    ls = eng._loss_spec("l2", "mean", False, emb, None, 100.0, B=B)
    out = torch.empty_like(x)
    assert lib().rvlm_pgd_run_mixed_fwd(eng._h, eng._h32, 1, x.data_ptr(), None, B, C.byref(ls), 0, 0.01, 2, 0.005, 0.9, 1,
                                        out.data_ptr(), None, None, st()) == L.RVLM_ERR_STATE
    assert lib().rvlm_pgd_run_mixed(eng._h, eng._h32, 1, x.data_ptr(), None, B, C.byref(ls), 0, 0.01, 2, 0.005, 0.9, 1,
                                    out.data_ptr(), None, None, st()) == L.RVLM_ERR_STATE
    L.check(lib().rvlm_vit_set_input_size(eng._h32, 0, 0))
    # both handles through the Python engine: the handoff works at the reduced size
    eng.set_input_size(16, 16)
    cot = torch.randn(B, cfg.out_dim, generator=g)
    e, gq = eng.handoff_inputgrad(x, None, output_normalize=True, cot=cot.to(dev()))
    xr = x.cpu().clone().requires_grad_(True)
    e_ref = ref(F.interpolate(xr, size=(32, 32), mode="bicubic", align_corners=False), True)
    (g_ref,) = torch.autograd.grad((e_ref * cot).sum(), xr)
    assert gq.shape == x.shape and rel_max(e.cpu(), e_ref.detach()) < 1e-3 and cos_sim(gq.cpu(), g_ref) > 0.98
    e0 = eng.forward(x, None, False)
    d0 = ((torch.rand(x.shape, generator=g) * 2 - 1) * (4 / 255)).to(dev())
    xa, flags, _ = eng.pgd_run(x, d0, "l2", "mean", e0, None, False, 4 / 255, 3, 1 / 255, 0.9, "max")
    assert xa.shape == x.shape and int(flags.item()) == 0 and float((xa - x).abs().max()) <= float(np.float32(4 / 255))
    eng.close()


# ---------------------------------------------------------------------------------------------- attack routes
def _golden(size, precision="fp32", max_batch=8):
    z = load_golden("attacks_resize_tiny.npz")
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=int(z["weights_seed"]))
    assert weights_digest(w) == str(z["weights_sha256"])
    eng = make_engine(cfg, w, precision, max_batch=max_batch)
    t = f"s{size}_"
    T = torch.from_numpy(z[t + "T"]).to(dev())
    x, y = torch.from_numpy(z[t + "x"]).to(dev()), torch.from_numpy(z[t + "y"]).to(dev())
    return z, t, eng, T, x, y


class _CountingResize(R.BicubicResize):
    """Counts the calls of the STANDALONE resizer: zero on the fused route."""
    calls = 0

    def forward(self, v):
        type(self).calls += 1
        return super().forward(v)


@pytest.mark.parametrize("size", [16, 12])
def test_classification_model_logits_fused_vs_two_step_vs_reference(size):
    z, t, eng, T, x, y = _golden(size)
    rs = _CountingResize(32)
    clf = R.ClassificationModel(eng, T, resizer=rs).eval()
    plain = R.ClassificationModel(eng, T, resizer=lambda v: rs(v)).eval()      # the same operator behind a plain callable
    _CountingResize.calls = 0
    with torch.no_grad():
        fused = clf(x)
    assert _CountingResize.calls == 0 and eng.input_size == (32, 32)
    with torch.no_grad():
        two = plain(x)
    assert _CountingResize.calls == 1
    assert rel_max(fused.cpu(), two.cpu()) < 1e-6
    assert rel_max(fused.cpu(), torch.from_numpy(z[t + "logits"])) < 1e-4
    assert torch.equal(fused.max(1)[1], y)
    # chunks beyond max_batch go through the fused front end one by one
    big = torch.cat([x, x], 0)
    with torch.no_grad():
        assert rel_max(clf(big).cpu(), torch.cat([fused, fused], 0).cpu()) < 1e-5
    assert _CountingResize.calls == 1
    # a differentiable call: resizer, then engine, through autograd
    xg = x.clone().requires_grad_(True)
    lg = clf(xg)
    (gx,) = torch.autograd.grad(lg[:, 0].sum(), xg)
    assert gx.shape == x.shape and _CountingResize.calls == 2 and float(gx.abs().max()) > 0
    eng.close()


@pytest.mark.parametrize("size", [16, 12])
def test_apgd_fused_route_vs_generic_route_vs_reference_golden(size):
    z, t, eng, T, x, y = _golden(size)
    eps, n_iter = float(z[t + "eps"]), int(z["n_iter"])
    rs = _CountingResize(32)
    clf = R.ClassificationModel(eng, T, resizer=rs).eval()
    generic = R.ClassificationModel(eng, T, resizer=lambda v: rs(v)).eval()
    xn = z[t + "x"]
    res = {}
    for name, model in (("fused", clf), ("generic", generic)):
        _CountingResize.calls = 0
        atk = R.APGDAttack(model, n_iter=n_iter, norm="Linf", n_restarts=2, eps=eps, seed=0, loss="ce", alpha=2.0, use_rs=True)
        adv = atk.perturb(x.clone(), y.clone())
        assert (_CountingResize.calls == 0) == (name == "fused"), "the fused route never calls the standalone resizer"
        assert eng.input_size == (32, 32)
        with torch.no_grad():
            robust = (clf(adv).max(1)[1] == y).cpu().numpy()
        assert np.array_equal(robust, z[t + "apgd_robust"]), name
        a = adv.cpu().numpy()
        assert a.shape == xn.shape and np.abs(a - xn).max() <= np.float32(eps) + 1e-7 and a.min() >= 0 and a.max() <= 1
        moved = (z[t + "apgd_adv"] != xn).reshape(7, -1).any(1)
        assert np.array_equal((a != xn).reshape(7, -1).any(1), moved), name
        assert np.mean(a[moved] == z[t + "apgd_adv"][moved]) > 0.85, name
        res[name] = a
    assert np.abs(res["fused"] - res["generic"]).max() < 2e-5 or np.mean(res["fused"] == res["generic"]) > 0.98
    # one run: the loss of the best point and the robust flags (autopgd_base.py:205-451's return values)
    atk = R.APGDAttack(clf, n_iter=n_iter, norm="Linf", n_restarts=1, eps=eps, seed=0, loss="ce", alpha=2.0, use_rs=True)
    atk.init_hyperparam(x)
    torch.random.manual_seed(0)
    _, acc1, loss_best, xba = atk.attack_single_run(x.clone(), y.clone())
    assert np.array_equal(acc1.cpu().numpy(), z[t + "run_acc"])
    np.testing.assert_allclose(loss_best.cpu().numpy(), z[t + "run_loss_best"], rtol=0.05, atol=1e-3)
    assert np.mean(xba.cpu().numpy() == z[t + "run_x_best_adv"]) > 0.85
    eng.close()


@pytest.mark.parametrize("size", [16, 12])
def test_autoattack_and_targeted_at_input_resolution_vs_reference_golden(size):
    z, t, eng, T, x, y = _golden(size)
    eps, n_iter, ntc = float(z[t + "eps"]), int(z["n_iter"]), int(z["n_target_classes"])
    rs = _CountingResize(32)
    clf = R.ClassificationModel(eng, T, resizer=rs).eval()
    _CountingResize.calls = 0
    aa = R.AutoAttack(clf, norm="Linf", eps=eps, seed=0, verbose=False, version="custom", attacks_to_run=["apgd-ce", "apgd-t"],
                      device=dev(), alpha=2.0, iterations_apgd=n_iter, use_rs=True)
    aa.apgd.n_restarts = 1
    aa.apgd_targeted.n_target_classes = ntc
    x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=int(z["bs"]), return_labels=True)
    # clean pass, apgd-ce and apgd-t all on the engine at the images' own size - unless the survivors of apgd-ce leave a batch of
    # ONE image for apgd-t (the device loops need B > 1, with or without a resizer)
    if int(z[t + "aa_robust_after_ce"].sum()) % int(z["bs"]) != 1:
        assert _CountingResize.calls == 0
    with torch.no_grad():
        robust = (clf(x_adv).max(1)[1] == y).cpu().numpy()
    assert np.array_equal(robust, z[t + "aa_robust"])
    assert np.array_equal(y_adv.cpu().numpy(), z[t + "aa_y_adv"])
    xa, xn = x_adv.cpu().numpy(), z[t + "x"]
    moved = (z[t + "aa_x_adv"] != xn).reshape(7, -1).any(1)
    assert np.array_equal((xa != xn).reshape(7, -1).any(1), moved)
    assert np.mean(xa[moved] == z[t + "aa_x_adv"][moved]) > 0.85
    # the targeted attack alone: fused == generic
    outs = []
    for model in (clf, R.ClassificationModel(eng, T, resizer=lambda v: rs(v)).eval()):
        atk = R.APGDAttack_targeted(model, n_iter=n_iter, norm="Linf", n_restarts=1, eps=eps, seed=0, n_target_classes=ntc,
                                    alpha=2.0, use_rs=True)
        outs.append(atk.perturb(x.clone(), y.clone()).cpu().numpy())
        assert np.abs(outs[-1] - xn).max() <= np.float32(eps) + 1e-7
    assert np.array_equal((outs[0] != xn).reshape(7, -1).any(1), (outs[1] != xn).reshape(7, -1).any(1))
    assert np.abs(outs[0] - outs[1]).max() < 2e-5 or np.mean(outs[0] == outs[1]) > 0.98
    eng.close()


@pytest.mark.parametrize("size", [16, 12])
def test_pgd_run_at_input_resolution_vs_reference_golden(size):
    z, t, eng, T, x, y = _golden(size)
    eps = float(z[t + "eps"])
    d0 = torch.from_numpy(z[t + "pgd_delta0"]).to(dev())
    eng.set_input_size(size, size)
    xa, flags, trace = eng.pgd_run(x, d0, "ce", "mean", T, y, True, eps, 10, eps / 4, 0.9, "max", want_trace=True)
    assert int(flags.item()) == 0 and xa.shape == x.shape
    got, ref = xa.cpu().numpy(), z[t + "pgd_xadv"]
    assert np.abs(got - z[t + "x"]).max() <= np.float32(eps) and got.min() >= 0.0 and got.max() <= 1.0
    assert np.mean(got == ref) > 0.95, np.mean(got == ref)
    assert abs(float(trace[0]) - float(z[t + "pgd_loss_start"])) <= 0.05 * abs(float(z[t + "pgd_loss_start"])) + 1e-4
    e = eng.forward(xa, None, True)
    lf = float(R.compute_loss("ce", e, y, None, 100., T, "mean"))
    assert abs(lf - float(z[t + "pgd_loss_final"])) <= 0.05 * abs(float(z[t + "pgd_loss_final"]))
    eng.close()


@pytest.mark.parametrize("size", [16, 12])
def test_fab_t_fused_route_vs_generic_route(size):
    z, t, eng, T, x, y = _golden(size)
    eps = float(z[t + "eps"])
    rs = _CountingResize(32)
    clf = R.ClassificationModel(eng, T, resizer=rs).eval()
    generic = R.ClassificationModel(eng, T, resizer=lambda v: rs(v)).eval()
    outs = {}
    for name, model in (("fused", clf), ("generic", generic)):
        _CountingResize.calls = 0
        atk = R.FABAttack(model, norm="Linf", n_restarts=1, n_iter=10, eps=eps, seed=0, targeted=True, n_target_classes=3)
        assert atk._engine_route(7, True, x) == (name == "fused")
        adv = atk.perturb(x.clone(), y.clone())
        assert (_CountingResize.calls == 0) == (name == "fused")
        assert eng.input_size == (32, 32) and adv.shape == x.shape
        with torch.no_grad():
            outs[name] = (adv.cpu().numpy(), (clf(adv).max(1)[1] == y).cpu().numpy())
    assert np.array_equal(outs["fused"][1], outs["generic"][1])
    # FAB is continuous but not smooth (the projection picks faces): per-sample distances, as tests/test_gpu_fab.py compares
    xn = z[t + "x"]
    dist = [np.abs(o[0] - xn).reshape(7, -1).max(1) for o in (outs["fused"], outs["generic"])]
    assert dist[0].max() <= eps + 1e-7 and np.array_equal(dist[0] > 0, dist[1] > 0)
    assert (np.abs(dist[0] - dist[1]) <= 0.02 * np.maximum(dist[1], 1e-12)).all(), (dist[0] / eps, dist[1] / eps)
    eng.close()


def test_square_attack_runs_at_input_resolution():
    z, t, eng, T, x, y = _golden(16)
    eps = float(z[t + "eps"])
    rs = _CountingResize(32)
    clf = R.ClassificationModel(eng, T, resizer=rs).eval()
    _CountingResize.calls = 0
    atk = R.SquareAttack(clf, norm="Linf", n_queries=40, eps=eps, p_init=.8, n_restarts=1, seed=5)
    adv = atk.perturb(x.clone(), y.clone())
    assert _CountingResize.calls == 0 and adv.shape == x.shape and eng.input_size == (32, 32)
    assert float((adv - x).abs().max()) <= float(np.float32(eps)) + 1e-7 and float(adv.min()) >= 0 and float(adv.max()) <= 1
    eng.close()


@pytest.mark.parametrize("size", [32, 96])
def test_full_size_geometry_vit_b32_bf16(size):
    """CIFAR (32) and STL-10 (96) into ViT-B/32 at 224: shapes, the eps ball and [0, 1] in the small space, an ascending loss."""
    cfg = R.CONFIGS["ViT-B-32"]
    sd = R.random_state_dict(cfg, seed=0, device=dev())
    B = 4
    eng = R.VitEngine(cfg, sd, precision="bf16", max_batch=B)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, size, size, generator=g).to(dev())
    T = torch.randn(cfg.out_dim, 10, generator=g)
    T = (T / T.norm(dim=0, keepdim=True)).to(dev())
    eng.set_input_size(size, size)
    with torch.no_grad():
        y = (eng.forward(x, None, True) @ T).max(1)[1]
    eps = 4 / 255
    d0 = ((torch.rand(x.shape, generator=g) * 2 - 1) * eps).to(dev())
    xa, flags, trace = eng.pgd_run(x, d0, "ce", "mean", T, y, True, eps, 10, 1 / 255, 0.9, "max", want_trace=True)
    assert tuple(xa.shape) == (B, 3, size, size) and int(flags.item()) == 0
    assert float((xa - x).abs().max()) <= float(np.float32(eps)) and float(xa.min()) >= 0 and float(xa.max()) <= 1
    tr = trace.cpu().numpy()
    assert np.isfinite(tr).all() and tr[-1] > tr[0]
    xa2, _, _ = eng.pgd_run(x, d0, "ce", "mean", T, y, True, eps, 10, 1 / 255, 0.9, "max")
    assert torch.equal(xa, xa2)
    # the same through the model-level API: APGD on the device loop at the images' own size
    clf = R.ClassificationModel(eng, T, resizer=R.BicubicResize(224)).eval()
    eng.set_input_size(0, 0)
    adv = R.APGDAttack(clf, n_iter=5, norm="Linf", n_restarts=1, eps=eps, seed=0, loss="ce").perturb(x.clone(), y.clone())
    assert adv.shape == x.shape and float((adv - x).abs().max()) <= float(np.float32(eps)) + 1e-7
    assert eng.input_size == (224, 224)
    eng.close()
