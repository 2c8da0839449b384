"""VLM-side attacks (RVLM_HAS_VLM_ATTACKS) on the GPU: each kernel of csrc/vlm_attack_kernels.hip against a torch restatement of
vlm_eval/attacks/pgd.py:39-65 / apgd.py:240-266, 321-351 written here (fp64 for the tolerance checks, the same lines in fp32 for the
bit-exact L-inf checks), PGD.perturb / APGD.perturb / apgd on the generic route replaying the reference's own loss and gradient
traces (tests/golden/vlm_attacks.npz), a run with host synchronisation forbidden, and the engine route against the generic route
driving the same tower through autograd."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.vlm_attacks import APGD, PGD, TokenLossModel, apgd
from oracle import vit_ref as V
from tests.gpu_helpers import dev, st, lib, record
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
MASKS = ["context", "query", 1, None]
SIZES = [192, 147, 70001, 150528]          # P % 4 == 0 and != 0; the last two take several trips of the grid-stride loops


def full_mask(mask_out, B, n_img, P, dtype):
    m = torch.ones(B, n_img, P, dtype=dtype)
    if mask_out == "context":
        m[:, :-1] = 0
    elif mask_out == "query":
        m[:, -1] = 0
    elif mask_out is not None:
        m[:, mask_out] = 0
    return m


def byte_mask(mask_out, n_img):
    if mask_out == 1 and n_img == 1:
        mask_out = 0
    m = full_mask(mask_out, 1, n_img, 1, torch.uint8).reshape(n_img)
    return mask_out, m


# ---- the reference's lines, restated ----------------------------------------------------------------------------------------------
def normalize_grad_ref(g, linf):
    return g.sign() if linf else F.normalize(g.flatten(1), p=2, dim=1).view_as(g)


def pgd_update_ref(x, g, d, v, m, linf, eps, step, mode, image_space):
    """pgd.py:40-65 on [B, n_img, P]; returns (delta, velocity, saw a NaN gradient)."""
    g = m * g
    nan = bool(g.isnan().any())
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    g = normalize_grad_ref(g, linf)
    v = normalize_grad_ref(0.9 * v + g, linf)
    d = d - step * v if mode == "min" else d + step * v
    d = torch.clamp(d, -eps, eps) if linf else torch.renorm(d, p=2, dim=0, maxnorm=eps)
    if image_space:
        d = torch.clamp(x + d, 0, 1) - x
    return d, v, nan


def l2n(t):
    return (t ** 2).flatten(1).sum(-1).sqrt().view(-1, 1, 1)


def apgd_step_ref(x, xa, xo, g, m, step, a, linf, eps):
    """apgd.py:242-266 on [B, n_img, P], step [B, 1, 1]; returns the new x_adv (x_adv_old becomes the old x_adv)."""
    g = g * m
    grad2 = xa - xo
    if linf:
        z = xa + step * torch.sign(g)
        z = torch.clamp(torch.min(torch.max(z, x - eps), x + eps), 0.0, 1.0)
        z = torch.clamp(torch.min(torch.max(xa + (z - xa) * a + grad2 * (1 - a), x - eps), x + eps), 0.0, 1.0)
    else:
        z = xa + step * g / (l2n(g) + 1e-12)
        z = torch.clamp(x + (z - x) / (l2n(z - x) + 1e-12) * torch.min(eps * torch.ones_like(x), l2n(z - x)), 0.0, 1.0)
        z = xa + (z - xa) * a + grad2 * (1 - a)
        z = torch.clamp(x + (z - x) / (l2n(z - x) + 1e-12) * torch.min(eps * torch.ones_like(x), l2n(z - x)), 0.0, 1.0)
    return z


def _inputs(B, n_img, P, seed, linf):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, n_img, P, generator=gen)
    g = torch.randn(B, n_img, P, generator=gen)
    g[:, :, ::7] = 0.0                                        # sign(0) = 0 must survive
    r = 4 / 255 if linf else 0.8 / (n_img * P) ** 0.5
    d = (torch.rand(B, n_img, P, generator=gen) * 2 - 1) * r
    v = torch.randn(B, n_img, P, generator=gen).sign() if linf else F.normalize(torch.randn(B, n_img * P, generator=gen)).view(B, n_img, P)
    return x, g, d, v


def _close(got, want64, rtol):
    got, want64 = got.double(), want64.double()
    return float((got - want64).norm() / want64.norm().clamp_min(1e-30)) <= rtol


# ---- kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("n_img", [1, 2, 5])
def test_mask_grad(P, n_img):
    l = lib()
    B = 2
    for mo in MASKS:
        mo, mb = byte_mask(mo, n_img)
        _, g, _, _ = _inputs(B, n_img, P, 3, True)
        gd, md = g.to(dev()), mb.to(dev())
        out = torch.full_like(gd, 7.0)
        flags = torch.zeros(1, dtype=torch.int32, device=dev())
        L.check(l.rvlm_mask_grad(gd.data_ptr(), md.data_ptr(), B, n_img, P, out.data_ptr(), flags.data_ptr(), st()))
        assert torch.equal(out.cpu(), g * full_mask(mo, B, n_img, P, torch.float32)) and int(flags.item()) == 0
        # NaN / Inf under a 0 of the mask is NaN in the reference's product too; in place
        g2 = g.clone(); g2[1, 0, 3] = float("inf"); g2[0, n_img - 1, P - 1] = float("nan")
        gd = g2.to(dev())
        L.check(l.rvlm_mask_grad(gd.data_ptr(), md.data_ptr(), B, n_img, P, gd.data_ptr(), flags.data_ptr(), st()))
        want = g2 * full_mask(mo, B, n_img, P, torch.float32)
        assert torch.equal(gd.cpu().isnan(), want.isnan()) and torch.equal(gd.cpu().nan_to_num(5.0), want.nan_to_num(5.0))
        assert int(flags.item()) == L.FLAG_NAN_GRAD
    # no mask at all
    L.check(l.rvlm_mask_grad(gd.data_ptr(), None, B, n_img, P, out.data_ptr(), None, st()))
    assert torch.equal(out.cpu().nan_to_num(5.0), gd.cpu().nan_to_num(5.0))


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("n_img", [1, 2, 5])
def test_pgd_masked_update(norm, P, n_img):
    l = lib()
    linf, B = norm == "linf", 2
    eps, step = (4 / 255, 1 / 255) if linf else (0.5, 0.1)
    for mo in MASKS:
        mo, mb = byte_mask(mo, n_img)
        for mode, image_space in (("max", True), ("min", True), ("max", False)):
            x, g, d, v = _inputs(B, n_img, P, 5, linf)
            if not image_space:
                x = x * 3 - 1
            m1 = full_mask(mo, 1, n_img, 1, torch.bool).reshape(n_img)
            d[:, ~m1] = 0                                     # masked images as the attack keeps them: never moved, no momentum
            v[:, ~m1] = 0
            xd, gd, dd, vd, md = (t.to(dev()) for t in (x, g, d, v, mb))
            xa = torch.empty_like(xd)
            flags = torch.zeros(1, dtype=torch.int32, device=dev())
            L.check(l.rvlm_pgd_masked_update(xd.data_ptr(), gd.data_ptr(), dd.data_ptr(), vd.data_ptr(), md.data_ptr(), B, n_img, P,
                                             0 if linf else 2, eps, step, 0.9, int(mode == "max"), int(image_space), xa.data_ptr(),
                                             flags.data_ptr(), st()))
            assert int(flags.item()) == 0, (mo, mode, image_space, int(flags.item()))
            d64, v64, _ = pgd_update_ref(x.double(), g.double(), d.double(), v.double(), full_mask(mo, B, n_img, P, torch.float64), linf,
                                         eps, step, mode, image_space)
            got_d, got_v = dd.cpu(), vd.cpu()
            if linf:
                d32, v32, _ = pgd_update_ref(x, g, d, v, full_mask(mo, B, n_img, P, torch.float32), True, eps, step, mode, image_space)
                assert torch.equal(got_d, d32) and torch.equal(got_v, v32), (mo, mode, image_space)
                assert float((got_d.double() - d64).abs().max()) <= 2e-7 and torch.equal(got_v.double(), v64)
                assert torch.equal(xa.cpu(), x + d32)
            else:
                # delta = clamp(x + d, 0, 1) - x carries the rounding of x + d (half an ulp of a value in [0,1]) in fp32
                assert float((got_d.double() - d64).abs().max()) <= 2e-7 + 2e-6 * float(d64.abs().max()), (mo, mode, image_space)
                assert _close(got_v, v64, 2e-6) and _close(xa.cpu(), x.double() + d64, 2e-6), (mo, mode, image_space)
                assert float(got_d.double().flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-6)
            # masked images: a zero gradient and zero momentum - bit-identical, whatever the attacked images of the sample do
            assert torch.equal(got_d[:, ~m1], d[:, ~m1]) and torch.equal(got_v[:, ~m1], v[:, ~m1]), (mo, mode, image_space)
            assert torch.equal(xa.cpu()[:, ~m1], x[:, ~m1])


def test_pgd_masked_update_flags():
    """NaN / range flags exactly where pgd.py prints (:41-43) or asserts (:62-65)."""
    l = lib()
    B, n_img, P = 1, 3, 192
    for kind in (0, 2):
        for case, want in (("clean", 0), ("nan_grad_attacked", L.FLAG_NAN_GRAD), ("nan_grad_masked", L.FLAG_NAN_GRAD),
                           ("inf_grad_masked", L.FLAG_NAN_GRAD), ("nan_delta", L.FLAG_NAN_DELTA | L.FLAG_ADV_RANGE),
                           ("nan_delta_nospace", L.FLAG_NAN_DELTA), ("x_outside", 0)):
            x, g, d, v = _inputs(B, n_img, P, 9, kind == 0)
            v.zero_()
            if case == "nan_grad_attacked":
                g[0, 2, 5] = float("nan")
            if case == "nan_grad_masked":
                g[0, 0, 5] = float("nan")
            if case == "inf_grad_masked":
                g[0, 1, 7] = float("inf")                     # mask * inf = NaN in the reference
            if case.startswith("nan_delta"):
                d[0, 2, 11] = float("nan")
            if case == "x_outside":
                x[0, 2, 3] = 1.5                              # clamp(x + d, 0, 1) - x brings x + d back: the reference passes :62 too
            mb = byte_mask("context", n_img)[1]
            xd, gd, dd, vd, md = (t.to(dev()) for t in (x, g, d, v, mb))
            flags = torch.zeros(1, dtype=torch.int32, device=dev())
            L.check(l.rvlm_pgd_masked_update(xd.data_ptr(), gd.data_ptr(), dd.data_ptr(), vd.data_ptr(), md.data_ptr(), B, n_img, P, kind,
                                             0.05 if kind == 0 else 0.5, 0.01, 0.9, 1, int(case != "nan_delta_nospace"), None,
                                             flags.data_ptr(), st()))
            got = int(flags.item())
            assert got == want, (kind, case, got, want)
            if "grad" in case:                                # NaN -> 0: the update is the one of a zero gradient there
                assert not dd.cpu().isnan().any()
    with pytest.raises(NotImplementedError):
        L.check(l.rvlm_pgd_masked_update(xd.data_ptr(), gd.data_ptr(), dd.data_ptr(), vd.data_ptr(), None, 1, 3, 192, 1, 0.1, 0.1, 0.9,
                                         1, 1, None, None, st()))
    with pytest.raises(ValueError):
        L.check(l.rvlm_pgd_masked_update(xd.data_ptr(), gd.data_ptr(), dd.data_ptr(), vd.data_ptr(), None, 1, 0, 192, 0, 0.1, 0.1, 0.9,
                                         1, 1, None, None, st()))


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("n_img", [1, 2, 5])
def test_apgd_masked_step(norm, P, n_img):
    l = lib()
    linf, B = norm == "linf", 2
    eps = 4 / 255 if linf else 0.5
    for mo in MASKS:
        mo, mb = byte_mask(mo, n_img)
        m1 = full_mask(mo, 1, n_img, 1, torch.bool).reshape(n_img)
        for a in (1.0, 0.75):
            x, g, d, _ = _inputs(B, n_img, P, 21, linf)
            gen = torch.Generator().manual_seed(22)
            xa = (x + d).clamp(0, 1)
            xo = (xa + (torch.rand(x.shape, generator=gen) * 2 - 1) * (1 / 255 if linf else 1e-3)).clamp(0, 1)
            xa[:, ~m1] = x[:, ~m1]                            # masked images as the attack keeps them: never moved
            xo[:, ~m1] = xa[:, ~m1]
            step = torch.tensor([2 * eps, 0.5 * eps])
            xd, xad, xod, gd, md, sd = (t.to(dev()) for t in (x, xa, xo, g, mb, step))
            flags = torch.zeros(1, dtype=torch.int32, device=dev())
            L.check(l.rvlm_apgd_masked_step(xd.data_ptr(), xad.data_ptr(), xod.data_ptr(), gd.data_ptr(), md.data_ptr(), sd.data_ptr(),
                                            a, eps, B, n_img, P, 0 if linf else 2, flags.data_ptr(), st()))
            assert int(flags.item()) == 0
            assert torch.equal(xod.cpu(), xa), "x_adv_old must hold the previous x_adv"
            got = xad.cpu()
            assert torch.equal(got[:, ~m1], xa[:, ~m1]), "masked images must come out bit-identical"
            mf = full_mask(mo, B, n_img, P, torch.float64)
            want64 = apgd_step_ref(x.double(), xa.double(), xo.double(), g.double(), mf, step.double().view(B, 1, 1), a, linf, eps)
            if linf:
                want32 = apgd_step_ref(x, xa, xo, g, mf.float(), step.view(B, 1, 1), a, True, eps)
                assert torch.equal(got, want32), (mo, a)
                assert float((got.double() - want64).abs().max()) <= 2e-7
            else:
                assert _close(got, want64, 2e-6), (mo, a)
    # NaN in the masked gradient is flagged and not zeroed (apgd.py has no such line)
    g[0, n_img - 1, 1] = float("nan")
    mb = torch.ones(n_img, dtype=torch.uint8)
    xd, xad, xod, gd, md, sd = (t.to(dev()) for t in (x, xa, xo, g, mb, step))
    L.check(l.rvlm_apgd_masked_step(xd.data_ptr(), xad.data_ptr(), xod.data_ptr(), gd.data_ptr(), md.data_ptr(), sd.data_ptr(), 0.75,
                                    eps, B, n_img, P, 0 if linf else 2, flags.data_ptr(), st()))
    assert int(flags.item()) == L.FLAG_NAN_GRAD


def test_apgd_masked_bookkeeping_vs_restatement():
    """apgd.py:321-351 in fp64 torch with its nonzero() indexing, driven by a scripted loss sequence that rises, stalls and
    oscillates, so that the best-loss select, both step-halving conditions and the restart from x_best all occur."""
    l = lib()
    B, n_img, P, n_iter = 1, 3, 147, 50
    n = n_img * P
    gen = torch.Generator().manual_seed(31)
    losses = torch.cumsum(torch.randn(n_iter + 1, B, generator=gen), 0)
    losses[20:30] = losses[19] - 0.5                          # a stall: no improvement between two checkpoints
    xs = torch.rand(n_iter + 1, B, n, generator=gen)          # stand-ins for the iterates and gradients of each iteration
    gs = torch.randn(n_iter + 1, B, n, generator=gen)
    # reference
    x_adv, grad = xs[0].clone(), gs[0].clone()
    x_best, x_best_adv, grad_best = x_adv.clone(), x_adv.clone(), grad.clone()
    loss_steps = torch.zeros(n_iter, B)
    loss_best = losses[0].clone(); lbl = loss_best.clone(); red = torch.ones_like(loss_best)
    step = torch.full((B, 1), 0.25)
    k, n_iter_min, size_decr, counter3 = max(int(0.22 * n_iter), 1), max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1), 0
    # device
    dv = lambda t: t.clone().to(dev())   # noqa: E731
    d_xadv, d_grad, d_xbest, d_xbestadv, d_gradbest = dv(x_adv), dv(grad), dv(x_best), dv(x_best_adv), dv(grad_best)
    d_steps, d_best, d_lbl, d_red, d_step = dv(loss_steps), dv(loss_best), dv(lbl), dv(red), dv(step.view(B))
    scratch = torch.zeros(5 * B, dtype=torch.uint8, device=dev())
    d_losses, d_xs, d_gs = losses.to(dev()), xs.to(dev()), gs.to(dev())
    halvings = improvements = 0
    for i in range(n_iter):
        x_adv, d_xadv = xs[i + 1].clone(), d_xs[i + 1].clone()            # "the gradient step" and "the new gradient"
        if i < n_iter - 1:
            grad, d_grad = gs[i + 1].clone(), d_gs[i + 1].clone()
        y1 = losses[i + 1].clone()
        x_best_adv = x_adv + 0.
        loss_steps[i] = y1 + 0
        ind = (y1 > loss_best).nonzero().squeeze()
        improvements += int(ind.numel())
        x_best[ind] = x_adv[ind].clone(); grad_best[ind] = grad[ind].clone(); loss_best[ind] = y1[ind] + 0
        counter3 += 1
        do_check = counter3 == k
        L.check(l.rvlm_apgd_masked_bookkeeping(i, B, n_iter, k, int(do_check), d_losses[i + 1].data_ptr(), d_steps.data_ptr(),
                                               d_best.data_ptr(), d_lbl.data_ptr(), d_red.data_ptr(), d_step.data_ptr(),
                                               d_xadv.data_ptr(), d_grad.data_ptr(), d_xbest.data_ptr(), d_gradbest.data_ptr(),
                                               d_xbestadv.data_ptr(), scratch.data_ptr(), n, st()))
        if do_check:
            t = torch.zeros(B)
            for c in range(k):
                t += (loss_steps[i - c] > loss_steps[i - c - 1]).float()
            osc = (t <= k * 0.75 * torch.ones_like(t)).float()
            osc = torch.max(osc, (1. - red) * (lbl >= loss_best).float())
            red, lbl = osc.clone(), loss_best.clone()
            if osc.sum() > 0:
                io = (osc > 0).nonzero().squeeze()
                step[io] /= 2.0
                x_adv[io] = x_best[io].clone(); grad[io] = grad_best[io].clone()
                halvings += 1
            counter3 = 0
            k = max(k - size_decr, n_iter_min)
        for name, got, want in (("x_adv", d_xadv, x_adv), ("grad", d_grad, grad), ("x_best", d_xbest, x_best),
                                ("x_best_adv", d_xbestadv, x_best_adv), ("grad_best", d_gradbest, grad_best),
                                ("loss_best", d_best, loss_best), ("step", d_step, step.view(B)), ("loss_steps", d_steps, loss_steps)):
            assert torch.equal(got.cpu(), want), (i, name)
    assert halvings >= 1 and improvements >= 1, (halvings, improvements)
    assert scratch[:B].cpu().eq(0).all()


# ---- the drivers against the reference's outputs ---------------------------------------------------------------------------------
class _Inject(torch.autograd.Function):
    """A loss of prescribed value whose gradient with respect to its input is a prescribed tensor."""

    @staticmethod
    def forward(ctx, v, value, G):
        ctx.G = G
        return value.clone()

    @staticmethod
    def backward(ctx, go):
        return ctx.G.clone(), None, None


class Replay:
    """The golden's model: call c returns losses[c] and hands back grads[c].  Everything lives on the device beforehand."""

    def __init__(self, z, name, scalar):
        self.losses = torch.from_numpy(z[name + "/losses"]).to(dev())
        self.grads = torch.from_numpy(z[name + "/grads"].astype(np.float32)).to(dev())
        self.scalar, self.calls = scalar, 0

    def __call__(self, x):
        c = self.calls
        self.calls += 1
        value = self.losses[c].reshape(()) if self.scalar else self.losses[c]
        return _Inject.apply(x, value, self.grads[c])


def _cases(kind):
    return [c for c in json.loads(str(load_golden("vlm_attacks.npz")["cases"])) if c["kind"] == kind]


@pytest.mark.parametrize("case", _cases("pgd"), ids=lambda c: c["name"])
def test_pgd_perturb_vs_reference_golden(case, capsys):
    z = load_golden("vlm_attacks.npz")
    name = case["name"]
    x = torch.from_numpy(z["x_shift" if case["shifted"] else "x"]).to(dev())
    pert = torch.from_numpy(z[name + "/pert"]).to(dev()) if case["pert"] else None
    model = Replay(z, name, scalar=True)
    atk = PGD(model, case["norm"], case["eps"], mode=case["mode"], mask_out=case["mask_out"], image_space=case["image_space"])
    adv, loss = atk.perturb(x, case["iterations"], case["stepsize"], perturbation=pert, return_loss=True)
    assert model.calls == case["iterations"]
    got, want = adv.cpu().numpy(), z[name + "/adv"]
    assert got.shape == want.shape and got.dtype == np.float32
    assert float(loss) == float(z[name + "/loss"])
    if case["norm"] == "linf":
        assert np.array_equal(got, want), f"{np.mean(got != want):.4f} of the pixels differ"
    else:
        rel = np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64))
        assert rel <= 2e-6, rel
    assert ("attention: nan in gradient" in capsys.readouterr().out) == case["nan"]
    # masked images never move (without a perturbation handed in on them)
    if not case["pert"] and case["mask_out"] is not None:
        m = full_mask(case["mask_out"], 1, 3, 1, torch.bool).reshape(3).numpy()
        assert np.array_equal(got[:, ~m], x.cpu().numpy()[:, ~m])


@pytest.mark.parametrize("case", _cases("apgd"), ids=lambda c: c["name"])
def test_apgd_vs_reference_golden(case):
    z = load_golden("vlm_attacks.npz")
    name = case["name"]
    x = torch.from_numpy(z["x"]).to(dev())
    pert = torch.from_numpy(z[name + "/pert"]).to(dev()) if case["pert"] else None
    atk = APGD(Replay(z, name, scalar=False), case["norm"], case["eps"], mask_out=case["mask_out"], initial_stepsize=case["alpha"])
    adv = atk.perturb(x, case["n_iter"], pert_init=pert)
    assert atk.model.calls == case["n_iter"] + 1
    # all three outputs, through apgd() called the way APGD.perturb calls it
    x_best, loss_best, x_best_adv = apgd(Replay(z, name, scalar=False), x, norm=case["norm"], eps=case["eps"], n_iter=case["n_iter"],
                                         mask=atk._set_mask(x), alpha=case["alpha"], pert_init=pert)
    assert torch.equal(adv, x_best)
    assert np.array_equal(loss_best.cpu().numpy(), z[name + "/loss_best"])
    for got, want in ((x_best.cpu().numpy(), z[name + "/x_best"]), (x_best_adv.cpu().numpy(), z[name + "/x_best_adv"])):
        if case["norm"] == "linf":
            assert np.array_equal(got, want), f"{np.mean(got != want):.4f} of the pixels differ"
        else:
            rel = np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64))
            assert rel <= 2e-6, rel
    # the reference's full-size mask tensor is accepted and gives the same bits
    mo = atk.mask_out
    full = full_mask(mo, 1, 3, 1, torch.float32).reshape(1, 3, 1, 1, 1, 1).expand(x.shape).contiguous().to(dev())
    again = apgd(Replay(z, name, scalar=False), x, norm=case["norm"], eps=case["eps"], n_iter=case["n_iter"], mask=full,
                 alpha=case["alpha"], pert_init=pert)[0]
    assert torch.equal(again, x_best)


# ---- no host synchronisation inside the loops -------------------------------------------------------------------------------------
class _NoSyncModel:
    """A differentiable stand-in for a VLM that forbids host synchronisation from its first call to its last: every kernel launch,
    allocation and torch op of the attack between two model calls then runs under torch.cuda.set_sync_debug_mode('error')."""

    def __init__(self, w, n_calls, scalar):
        self.w, self.n_calls, self.scalar, self.calls = w, n_calls, scalar, 0

    def __call__(self, x):
        if self.calls == 0:
            torch.cuda.set_sync_debug_mode("error")
        self.calls += 1
        loss = torch.tanh((x * self.w).flatten(1).sum(1))
        if self.calls == self.n_calls:
            torch.cuda.set_sync_debug_mode("default")
        return loss.sum() if self.scalar else loss


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_no_host_sync_inside_the_loops(norm):
    gen = torch.Generator().manual_seed(41)
    x = torch.rand(1, 5, 1, 3, 16, 16, generator=gen).to(dev())
    w = torch.randn(x.shape, generator=gen).to(dev()) * 0.05
    eps = 4 / 255 if norm == "linf" else 0.5
    try:
        m = _NoSyncModel(w, 20, scalar=True)
        adv = PGD(m, norm, eps, mode="max").perturb(x, 20, eps / 4)
        assert m.calls == 20
        m = _NoSyncModel(w, 21, scalar=False)
        adv2 = APGD(m, norm, eps, initial_stepsize=1.0).perturb(x, 20)
        assert m.calls == 21
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a in (adv, adv2):
        assert torch.equal(a[:, :-1], x[:, :-1]) and not torch.equal(a[:, -1], x[:, -1])
    # the guard does catch a synchronising loop: the same model under a loop that reads a value back
    m = _NoSyncModel(w, 3, scalar=True)
    try:
        with pytest.raises(RuntimeError):
            m(x)
            float(m(x))
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- engine route -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("attack", ["pgd_linf", "pgd_l2", "apgd_linf"])
def test_engine_route_equals_generic_route_through_the_tower(precision, attack):
    """TokenLossModel (one rvlm_vit_tokens_fwd_inputgrad per iteration, no autograd graph) against the generic route driving the
    same ClipVisionTower through torch autograd: 3 images, mask_out='context', a toy ViT read LLaVA's way (2 of its 3 blocks)."""
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=9)
    eng = R.VitEngine(R.VitConfig(cfg.image_size, cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.out_dim, cfg.act),
                      {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=4)
    tower = R.ClipVisionTower(eng, select_layer=-2, select_feature="patch").eval()
    gen = torch.Generator().manual_seed(51)
    s = cfg.image_size
    x = torch.rand(1, 3, 1, 3, s, s, generator=gen).to(dev())
    d0 = ((torch.rand(x.shape, generator=gen) * 2 - 1) * (4 / 255)).to(dev())
    with torch.no_grad():
        ref = tower(x.reshape(-1, 3, s, s)).clone()
    fused = TokenLossModel(tower, ref)

    def generic(v):
        return ((tower(v.reshape(-1, 3, s, s)) - ref) ** 2).sum().reshape(1)

    if attack == "apgd_linf":
        run = lambda m: APGD(m, "linf", 4 / 255, mask_out="context").perturb(x, 10, pert_init=d0)   # noqa: E731
    else:
        norm, eps, step = ("linf", 4 / 255, 1 / 255) if attack == "pgd_linf" else ("l2", 1.5, 0.4)
        run = lambda m: PGD(m, norm, eps, mode="max", mask_out="context").perturb(x, 10, step, perturbation=d0)   # noqa: E731
    a, b = run(fused), run(lambda v: generic(v).sum() if attack != "apgd_linf" else generic(v))
    assert a.shape == x.shape and float(a.min()) >= 0 and float(a.max()) <= 1
    same = float((a - b).abs().le(1e-6).float().mean())
    moved = float((a[:, -1] != x[:, -1]).float().mean())
    with torch.no_grad():
        la, lb, l0 = float(generic(a)), float(generic(b)), float(generic((x + d0).clamp(0, 1)))
    record(f"vlm_engine_route[{precision},{attack}]", same=same, moved=moved, loss_engine=la, loss_generic=lb, loss_start=l0)
    assert moved > 0.5 and la > l0, (moved, la, l0)
    if attack == "apgd_linf":
        assert torch.equal(a[:, :-1], (x + d0).clamp(0, 1)[:, :-1])     # masked images: pert_init clamped into [0,1], then untouched
    assert same > (0.999 if precision == "fp32" else 0.95), same
    assert abs(la - lb) <= (1e-3 if precision == "fp32" else 0.05) * abs(lb), (la, lb)
    # masked images went through the forward: the loss counts their tokens
    with torch.no_grad():
        per = ((tower(a.reshape(-1, 3, s, s)) - ref) ** 2).sum(dim=(1, 2))
    if attack != "apgd_linf":
        assert float(per[:-1].sum()) > 0 and float(fused(a)) == pytest.approx(float(per.sum()), rel=1e-5)
    eng.close()
