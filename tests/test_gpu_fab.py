"""FAB / FAB-T on the GPU: the projection kernel against the reference's golden rows and an fp64 property check, the fused
step, the bookkeeping kernels, the logit-difference loss, and FABAttack / AutoAttack(version='standard') against what the
reference produced on the tiny ViT + 10-class head (tests/golden/fab_tiny.npz).  FAB is continuous (no sign()): attacks are
compared by the set of fooled images and the per-sample distance, not by identical pixels."""
import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from oracle import vit_ref as V
from tests.fab_cases import hashed_row
from tests.gpu_helpers import dev, lib, st
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu


def project(t, w, b, want_lambda=True):
    t, w, b = (torch.as_tensor(a, dtype=torch.float32).to(dev()).contiguous() for a in (t, w, b))
    R_, D = t.shape
    d = torch.full_like(t, 7.0)
    lam = torch.full([R_], -1.0, device=dev())
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    L.check(lib().rvlm_fab_projection_linf(t.data_ptr(), w.data_ptr(), b.data_ptr(), R_, D, d.data_ptr(),
                                           lam.data_ptr() if want_lambda else None, flags.data_ptr(), st()), "projection")
    torch.cuda.synchronize()
    return d.cpu().numpy(), lam.cpu().numpy(), int(flags.item())


def test_projection_matches_the_reference_rows():
    z = load_golden("fab_tiny.npz")
    for tag in ("p1003", "p3000"):
        d, lam, flags = project(z[f"{tag}_t"], z[f"{tag}_w"], z[f"{tag}_b"])
        assert flags == 0
        assert np.abs(d - z[f"{tag}_d"]).max() <= 1e-6
        assert np.abs(lam - z[f"{tag}_lambda"]).max() <= 1e-5 * z[f"{tag}_lambda"].max()
        assert (np.abs(lam - z[f"{tag}_lambda"]) <= 1e-5 * z[f"{tag}_lambda"] + 1e-12).all()
    D = int(z["big_D"])
    rows = [hashed_row(D, int(s), float(o)) for s, o in z["big_salt_offset"]]
    d, lam, flags = project(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows]))
    assert flags == 0
    assert (np.abs(lam - z["big_lambda"]) <= 1e-5 * z["big_lambda"]).all()
    assert np.abs(d[:, ::997] - z["big_d_stride997"]).max() <= 1e-6


def test_projection_properties_full_size_and_reproducible():
    g = torch.Generator().manual_seed(5)
    R_, D = 256, 150528
    t = torch.rand(R_, D, generator=g)
    w = torch.randn(R_, D, generator=g) * (torch.rand(R_, D, generator=g) > 0.1)
    wt = (w.double() * t.double()).sum(1)
    aw = w.abs().double().sum(1)
    scale = torch.tensor([1e-4, 1e-2, 0.1, 0.3, -1e-3, -0.05, -0.2, 0.6]).repeat(R_ // 8).double()   # 0.6: misses the box
    b = (wt + scale * aw).float()
    d1, lam1, flags = project(t, w, b)
    d2, lam2, _ = project(t, w, b)
    assert flags == 0
    assert np.array_equal(d1, d2) and np.array_equal(lam1, lam2)          # bit-identical run to run
    d = torch.from_numpy(d1)
    z = t + d
    assert float(z.min()) >= 0.0 and float(z.max()) <= 1.0                 # the box, exactly
    assert bool((d[w == 0] == 0).all())
    assert np.allclose(d.abs().max(1)[0].numpy(), lam1, rtol=0, atol=0)
    resid = ((w.double() * z.double()).sum(1) - b.double()).abs()
    feasible = (w.abs().double() * torch.where((scale[:, None] > 0) == (w > 0), 1 - t, t).double()).sum(1) > (scale * aw).abs()
    assert int(feasible.sum()) == R_ * 7 // 8
    # (the second term: c = b - w.t is formed from an fp32 sum of 150 528 products - 1e-7 of sum|w_i| is its rounding, and it is
    # all that is left of the tolerance on a row whose b happens to be near 0)
    assert bool((resid[feasible] <= 1e-4 * (1 + b.double().abs()[feasible]) + 1e-7 * aw[feasible]).all())
    # the rows that miss the box go to the faces
    miss = ~feasible
    zz = z[miss][w[miss] != 0]
    assert bool(((zz == 0) | (zz >= 1 - 1e-6)).all())                  # t + fl(1 - t) may round one ulp below 1


def test_projection_nan_row_terminates_and_is_flagged():
    g = torch.Generator().manual_seed(6)
    t = torch.rand(4, 3000, generator=g)
    w = torch.randn(4, 3000, generator=g)
    b = (w * t).sum(1) + torch.tensor([3.0, -2.0, 5.0, 1.0])
    d_ok, lam_ok, f0 = project(t, w, b)
    w_bad = w.clone()
    w_bad[1, 17] = float("nan")
    d, lam, flags = project(t, w_bad, b)
    assert f0 == 0 and flags == L.FLAG_FAB_NONFINITE
    keep = [0, 2, 3]
    assert np.array_equal(d[keep], d_ok[keep]) and np.array_equal(lam[keep], lam_ok[keep])
    assert lam[1] == 0 and not np.isnan(d[1]).any() and np.abs(d[1]).max() == 0


def test_linf_step_equals_projection_plus_update():
    g = torch.Generator().manual_seed(7)
    B, D = 6, 3 * 32 * 32
    x0 = torch.rand(B, D, generator=g)
    x1 = (x0 + 0.02 * torch.randn(B, D, generator=g)).clamp(0, 1)
    dg = torch.randn(B, D, generator=g)
    df = torch.tensor([-3.0, -0.5, 2.0, -8.0, -0.2, -40.0])
    alpha_max, eta = 0.1, 1.05
    x1d, x0d, dgd, dfd = (a.to(dev()).contiguous() for a in (x1, x0, dg, df))
    out = x1d.clone()
    lam = torch.empty(B, 2, device=dev())
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    L.check(lib().rvlm_fab_linf_step(out.data_ptr(), x0d.data_ptr(), dgd.data_ptr(), dfd.data_ptr(), B, D, alpha_max, eta,
                                     lam.data_ptr(), flags.data_ptr(), st()), "step")
    torch.cuda.synchronize()
    b = -df + (dg * x1).sum(1)                                          # fab_base.py:186-187
    d3, lam3, _ = project(torch.cat([x1, x0]), torch.cat([dg, dg]), torch.cat([b, b]))
    d1, d0 = torch.from_numpy(d3[:B]), torch.from_numpy(d3[B:])
    a = torch.from_numpy(lam3).clamp_min(1e-8)
    alpha = (a[:B] / (a[:B] + a[B:])).clamp(0, alpha_max)[:, None]
    want = ((x1 + eta * d1) * (1 - alpha) + (x0 + d0 * eta) * alpha).clamp(0, 1)
    assert int(flags.item()) == 0
    assert np.allclose(lam.cpu().numpy(), np.stack([lam3[:B], lam3[B:]], 1), rtol=1e-3, atol=1e-7)   # b is re-summed in fp32
    assert float((out.cpu() - want).abs().max()) <= 2e-6


def test_track_best_and_jacobian_argmin():
    g = torch.Generator().manual_seed(8)
    B, D, beta = 5, 1003, 0.9
    x0 = torch.rand(B, D, generator=g)
    x1 = (x0 + 0.05 * torch.randn(B, D, generator=g)).clamp(0, 1)
    adv = torch.rand(B, D, generator=g)
    res2 = torch.tensor([1e10, 1e-4, 1e10, 0.5, 1e10])
    eq = torch.tensor([0, 0, 1, 0, 1], dtype=torch.uint8)
    x1d, x0d, advd, resd, eqd = (a.to(dev()).contiguous() for a in (x1, x0, adv, res2, eq))
    L.check(lib().rvlm_fab_track_best(x1d.data_ptr(), x0d.data_ptr(), advd.data_ptr(), resd.data_ptr(), eqd.data_ptr(), beta,
                                      B, D, st()), "track_best")
    torch.cuda.synchronize()
    t = (x1 - x0).abs().max(1)[0]
    is_adv = eq == 0
    better = is_adv & (t < res2)
    assert torch.equal(advd.cpu(), torch.where(better[:, None], x1, adv))
    assert torch.equal(resd.cpu(), torch.where(better, t, res2))
    assert torch.equal(x1d.cpu(), torch.where(is_adv[:, None], x0 + (x1 - x0) * beta, x1))
    assert better.tolist() == [True, False, False, True, False]
    # streaming arg-min over classes == the reference's [K, B, D] form (fab_base.py:166-184)
    K = 6
    G = torch.randn(K, B, D, generator=g)
    zl = torch.randn(B, K, generator=g)
    y = torch.tensor([0, 3, 5, 2, 2])
    G[4], zl[:, 4] = G[1], zl[:, 1]                                       # a tie between classes 1 and 4: the first wins
    u = torch.arange(B)
    dfr = zl - zl[u, y][:, None]
    dgr = G.transpose(0, 1) - G[y, u][:, None]
    dfr[u, y] = 1e10
    ind = (dfr.abs() / (1e-12 + dgr.abs().sum(-1))).min(1)[1]
    best_dist = torch.full([B], float("inf"), device=dev())
    best_df, best_w = torch.zeros(B, device=dev()), torch.zeros(B, D, device=dev())
    yd, gy = y.to(dev()), G[y, u].to(dev()).contiguous()
    for k in range(K):
        gk, dfk = G[k].to(dev()).contiguous(), (zl[:, k] - zl[u, y]).to(dev()).contiguous()
        L.check(lib().rvlm_fab_jacobian_argmin(gk.data_ptr(), gy.data_ptr(), dfk.data_ptr(), yd.data_ptr(), k, B, D,
                                               best_dist.data_ptr(), best_df.data_ptr(), best_w.data_ptr(), st()), "argmin")
    torch.cuda.synchronize()
    assert torch.equal(best_df.cpu(), dfr[u, ind])
    assert torch.equal(best_w.cpu(), dgr[u, ind])


def _tiny(z, precision="fp32", max_batch=8):
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=int(z["weights_seed"]))
    eng = R.VitEngine(R.VitConfig(cfg.image_size, cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.out_dim, cfg.act),
                      {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch)
    clf = R.ClassificationModel(eng, torch.from_numpy(z["T"]).to(dev())).eval()
    return eng, clf, torch.from_numpy(z["x"]).to(dev()), torch.from_numpy(z["y"]).to(dev())


def test_logit_diff_loss_and_fwd_inputgrad():
    assert L.LOSS_LOGIT_DIFF == 4
    g = torch.Generator().manual_seed(9)
    B, D, C_ = 5, 32, 10
    emb = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    T = torch.nn.functional.normalize(torch.randn(D, C_, generator=g), dim=0)
    y, yt = torch.tensor([1, 4, 4, 0, 9]), torch.tensor([2, 4, 0, 7, 3])         # row 1: y == target
    embd, Td, yd, ytd = emb.to(dev()), T.to(dev()).contiguous(), y.to(dev()), yt.to(dev())
    per, d_emb = torch.empty(B, device=dev()), torch.empty(B, D, device=dev())
    peq = torch.empty(B, dtype=torch.uint8, device=dev())
    scratch = torch.empty(B * C_ + D * C_, device=dev())
    L.check(lib().rvlm_loss_grad(L.LOSS_LOGIT_DIFF, L.RED_NONE, embd.data_ptr(), Td.data_ptr(), yd.data_ptr(), ytd.data_ptr(),
                                 B, D, C_, 100.0, per.data_ptr(), None, d_emb.data_ptr(), peq.data_ptr(), scratch.data_ptr(),
                                 st()), "loss_grad")
    torch.cuda.synchronize()
    zl = (emb.double() @ T.double()) * 100.0
    u = torch.arange(B)
    assert float((per.cpu().double() - (-(zl[u, y] - zl[u, yt]))).abs().max()) <= 1e-4
    assert float((d_emb.cpu().double() - 100.0 * (T.double()[:, yt] - T.double()[:, y]).T).abs().max()) <= 1e-4
    assert torch.equal(peq.cpu().bool(), zl.max(1)[1] == y)
    # through the engine: df / dg of one call against autograd through ClassificationModel
    z = load_golden("fab_tiny.npz")
    eng, clf, x, yy = _tiny(z)
    with torch.no_grad():
        tgt = clf(x).topk(2, dim=1)[1][:, 1]
    _, df, _, dg = eng.fwd_inputgrad(x, None, "logit-diff", "none", clf.text_embedding, yy, True, 100.0, y_target=tgt)
    xr = x.clone().requires_grad_(True)
    zl = clf(xr)
    u = torch.arange(x.shape[0], device=dev())
    diff = -(zl[u, yy] - zl[u, tgt])
    (gr,) = torch.autograd.grad(diff.sum(), xr)
    assert float((df - diff.detach()).abs().max()) <= 1e-3
    assert float((dg - gr).abs().max()) <= 1e-4 * float(gr.abs().max())
    eng.close()


class _Counting(torch.nn.Module):
    """A plain differentiable torch callable around the classifier (so FABAttack takes the generic route) that counts calls."""

    def __init__(self, clf):
        super().__init__()
        self.clf, self.calls = clf, 0

    def forward(self, v):
        self.calls += 1
        return self.clf(v)


def _compare(z, tag, adv, x, y, clf, eps):
    dist = (adv - x).abs().reshape(x.shape[0], -1).max(1)[0].cpu().numpy()
    with torch.no_grad():
        fooled = (clf(adv).max(1)[1] != y).cpu().numpy()
    assert np.array_equal(fooled, z[f"{tag}_fooled"]), (fooled, dist / eps)
    assert dist.max() <= eps + 1e-7
    assert np.array_equal(dist > 0, z[f"{tag}_fooled"])
    ref = z[f"{tag}_dist"]
    assert (np.abs(dist - ref)[fooled] <= 0.02 * ref[fooled]).all(), (dist / eps, ref / eps)
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1


def test_fabattack_vs_reference_golden():
    z = load_golden("fab_tiny.npz")
    eng, clf, x, y = _tiny(z)
    eps, n_iter, ntc = float(z["eps"]), int(z["n_iter"]), int(z["n_target_classes"])
    # targeted, engine route (rvlm_vit_fwd_inputgrad with RVLM_LOSS_LOGIT_DIFF)
    atk = R.FABAttack(clf, norm="Linf", n_restarts=1, n_iter=n_iter, eps=eps, seed=0, targeted=True, n_target_classes=ntc)
    assert atk._engine_route(7, True) and not atk._engine_route(7, False) and not atk._engine_route(1, True)
    _compare(z, "fabt", atk.perturb(x.clone(), y.clone()), x, y, clf, eps)
    assert int(atk.flags.item()) == 0
    # targeted and untargeted, generic route (autograd through the classifier)
    wrapped = _Counting(clf)
    atk = R.FABAttack(wrapped, norm="Linf", n_restarts=1, n_iter=n_iter, eps=eps, seed=0, targeted=True, n_target_classes=ntc)
    _compare(z, "fabt", atk.perturb(x.clone(), y.clone()), x, y, clf, eps)
    assert wrapped.calls == int(z["fabt_n_model_calls"])
    wrapped.calls = 0
    atk = R.FABAttack(wrapped, norm="Linf", n_restarts=2, n_iter=n_iter, eps=eps, seed=0, targeted=False)
    _compare(z, "fab", atk.perturb(x.clone(), y.clone()), x, y, clf, eps)
    assert wrapped.calls == int(z["fab_n_model_calls"])
    eng.close()


@pytest.mark.parametrize("tag", ["aa_std", "aa_fabt"])
def test_autoattack_standard_vs_reference_golden(tag):
    z = load_golden("fab_tiny.npz")
    eng, clf, x, y = _tiny(z)
    eps = float(z["eps"])
    kw = dict(version="standard") if tag == "aa_std" else dict(version="custom", attacks_to_run=["fab-t"])
    aa = R.AutoAttack(clf, norm="Linf", eps=eps, seed=0, verbose=False, device=dev(), alpha=2.0,
                      iterations_apgd=int(z["iterations_apgd"]), use_rs=True, **kw)
    aa.apgd.n_restarts, aa.apgd_targeted.n_target_classes = 1, int(z["n_target_classes"])
    aa.fab.n_iter, aa.fab.n_target_classes, aa.fab.n_restarts = int(z["n_iter"]), int(z["n_target_classes"]), 1
    aa.square.n_queries = int(z["square_queries"])
    x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=int(z["bs"]), return_labels=True)
    with torch.no_grad():
        robust = (clf(x_adv).max(1)[1] == y).cpu().numpy()
    assert np.array_equal(robust, ~z[f"{tag}_fooled"])
    assert np.array_equal(y_adv.cpu().numpy(), z[f"{tag}_y_adv_returned"])
    dist = (x_adv - x).abs().reshape(7, -1).max(1)[0].cpu().numpy()
    assert np.array_equal(dist > 0, z[f"{tag}_fooled"]) and dist.max() <= eps + 1e-7
    if tag == "aa_fabt":
        ref = z[f"{tag}_dist"]
        assert (np.abs(dist - ref) <= 0.02 * ref + 1e-12).all(), (dist / eps, ref / eps)
    eng.close()


def test_fabt_full_size_bf16():
    cfg = R.CONFIGS["ViT-L-14"]
    sd = R.random_state_dict(cfg, seed=0, device=dev())
    eng = R.VitEngine(cfg, sd, precision="bf16", max_batch=8)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(8, 3, 224, 224, generator=g).to(dev())
    T = torch.nn.functional.normalize(torch.randn(cfg.out_dim, 1000, generator=g), dim=0).to(dev())
    clf = R.ClassificationModel(eng, T).eval()
    with torch.no_grad():
        y = clf(x).max(1)[1]
    ws = eng.workspace_bytes()
    eps = 4 / 255
    atk = R.FABAttack(clf, norm="Linf", n_iter=5, eps=eps, seed=0, targeted=True, n_target_classes=1)
    adv = atk.perturb(x.clone(), y.clone())
    torch.cuda.synchronize()
    assert eng.workspace_bytes() == ws
    assert int(atk.flags.item()) == 0
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1 and not bool(torch.isnan(adv).any())
    dist = (adv - x).abs().reshape(8, -1).max(1)[0]
    assert float(dist.max()) <= eps + 1e-7
    with torch.no_grad():
        fooled = clf(adv).max(1)[1] != y
    assert bool((dist[fooled] > 0).all()) and bool((dist[~fooled] == 0).all())
    eng.close()
