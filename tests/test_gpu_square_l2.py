"""Square Attack, L2 (RVLM_HAS_SQUARE_L2) on the GPU.

(1) rvlm_square_l2_propose against a float64 torch evaluation, written here, of one query of autoattack/square.py:339-379 on the
    same float32 inputs.  Tolerance |x_new - fp64| <= 2e-6 * eps + 2.4e-7: four chained norms, each a tree sum with relative error
    under 5e-7, times an element of magnitude at most eps, plus one rounding at 1.
(2) robustvlm_amd.SquareAttack(norm='L2') driven with the reference's own classifier as ``predict`` (evaluated on the host, the
    method of test_gpu_engine.test_square_attack_vs_reference_golden) against tests/golden/square_l2_tiny.npz: the counters and the
    decisions are exact; the images agree within the per-query bound accumulated linearly over the queries.
(3) the same through AutoAttack(norm='L2', version='custom', attacks_to_run=['square']).
(4) the native route (fp32 engine + ClassificationModel), (5) ViT-L/14 bf16 at eps = 3.0: properties only.
"""
import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from oracle import vit_ref as V
from tests.gpu_helpers import dev
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

IDX = (0, 1, 3, 4, 8)          # n_active = 5 of 9 images
N_IMG, SENTINEL = 9, -7.0


def tol(eps):
    return 2e-6 * eps + 2.4e-7


def query_fp64(x, x_best, idx, c, vh, vw, vh2, vw2, s, eps, eta, sign):
    """Steps 3 to 6 of one L2 query (square.py:339-379) in float64 on float32 inputs; eps is the float32 value the kernel gets."""
    eps = float(np.float32(eps))
    xc = x[idx].double()
    d = x_best[idx].double() - xc
    m = d.shape[0]
    win1 = d[:, :, vh:vh + s, vw:vw + s]
    nw1 = (win1 ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    union = torch.zeros_like(d)
    union[:, :, vh:vh + s, vw:vw + s] = 1.
    union[:, :, vh2:vh2 + s, vw2:vw2 + s] = 1.
    nimg = (d ** 2).flatten(1).sum(1).sqrt().view(-1, 1, 1, 1)
    nws = ((d * union) ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()
    new = eta.double().view(1, 1, s, s) * sign.double().view(m, c, 1, 1) + win1 / (1e-12 + nw1)
    new = new / (1e-12 + (new ** 2).sum(dim=(-2, -1), keepdim=True).sqrt()) * \
        (torch.clamp(eps ** 2 - nimg ** 2, min=0.) / c + nws ** 2).sqrt()
    d = d.clone()
    d[:, :, vh2:vh2 + s, vw2:vw2 + s] = 0.
    d[:, :, vh:vh + s, vw:vw + s] = new
    nd = (d ** 2).flatten(1).sum(1).sqrt().view(-1, 1, 1, 1)
    return torch.clamp(xc + eps * d / (nd + 1e-12), 0., 1.)


def window_pairs(h, w, s):
    """((vh, vw), (vh2, vw2)): opposite corners (disjoint when they fit, at the borders), overlapping, identical."""
    a = (min(1, h - s), min(2, w - s))
    b = (min(a[0] + s // 2, h - s), min(a[1] + s // 3, w - s))
    pairs = [((0, 0), (h - s, w - s)), ((h - s, 0), (0, w - s)), (a, b), (b, b)]
    return list(dict.fromkeys(pairs))


def make_case(c, h, w, s, eps, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N_IMG, c, h, w, generator=g)
    x[0, :, :3] = 0.0                                                    # pixels on the faces 0 and 1
    x[1, :, -3:] = 1.0
    x[3, 0, :, :2] = 1.0
    t = torch.randn(N_IMG, c, h, w, generator=g)
    scale = torch.full((N_IMG,), 0.8)
    scale[4] = 1.5                                                       # |delta| > eps: no room left
    scale[8] = 1.0
    x_best = torch.clamp(x + eps * scale.view(-1, 1, 1, 1) * t / t.flatten(1).norm(dim=1).view(-1, 1, 1, 1), 0., 1.)
    eta = R.square.eta_window(s)
    if seed % 2:
        eta = eta.permute([1, 0])
    sign = torch.sign(2 * torch.rand(len(IDX), c, generator=g) - 1)
    return x.contiguous(), x_best.contiguous(), eta.contiguous(), sign


def propose(lib, x, x_best, idx, c, h, w, vh, vw, vh2, vw2, s, eps, eta, sign, flags, x_new=None):
    if x_new is None:
        x_new = torch.full((idx.numel() + 2, c, h, w), SENTINEL, device=x.device)
    rc = lib.rvlm_square_l2_propose(x.data_ptr(), x_best.data_ptr(), idx.data_ptr(), idx.numel(), c, h, w, vh, vw, vh2, vw2, s, eps,
                                    eta.data_ptr(), sign.data_ptr(), x_new.data_ptr(), L.ptr(flags), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, x_new


@pytest.mark.parametrize("c,h,w,s,eps", [(3, 21, 27, 3, 1.0), (3, 21, 27, 21, 0.5), (3, 32, 32, 7, 1.0), (3, 32, 32, 32, 0.75),
                                         (3, 224, 224, 3, 3.0), (3, 224, 224, 45, 3.0)])
def test_kernel_against_fp64(c, h, w, s, eps):
    lib = L.load()
    x, x_best, eta, sign = make_case(c, h, w, s, eps, seed=100 * h + s)
    idx = torch.tensor(IDX)
    worst = 0.0
    for (vh, vw), (vh2, vw2) in window_pairs(h, w, s):
        xb = x_best.clone()
        xb[3, :, vh:vh + s, vw:vw + s] = x[3, :, vh:vh + s, vw:vw + s]   # delta = 0 inside window 1
        want = query_fp64(x, xb, idx, c, vh, vw, vh2, vw2, s, eps, eta, sign)
        xd, xbd, etad, signd, idxd = (t.to(dev()) for t in (x, xb, eta, sign, idx))
        flags = torch.zeros(1, dtype=torch.int32, device=dev())
        rc, got = propose(lib, xd, xbd, idxd, c, h, w, vh, vw, vh2, vw2, s, eps, etad, signd, flags)
        L.check(rc, "rvlm_square_l2_propose")
        assert int(flags.item()) == 0
        assert torch.all(got[len(IDX):] == SENTINEL)                    # rows beyond n_active are untouched
        err = (got[:len(IDX)].cpu().double() - want).abs().max().item()
        worst = max(worst, err)
        print(f"({c},{h},{w}) s={s} windows ({vh},{vw}) ({vh2},{vw2}): max |x_new - fp64| = {err:.3e} (bound {tol(eps):.3e})")
        assert err <= tol(eps)
        nrm = (want - x[idx].double()).flatten(1).norm(dim=1)
        assert float(nrm.max()) <= eps * (1 + 1e-9)
        _, again = propose(lib, xd, xbd, idxd, c, h, w, vh, vw, vh2, vw2, s, eps, etad, signd, flags)
        assert torch.equal(got, again)                                   # bit-identical run to run
    print(f"({c},{h},{w}) s={s}: worst {worst:.3e}")


def test_kernel_nan_sets_the_flag_and_keeps_the_row():
    lib = L.load()
    c, h, w, s, eps = 3, 32, 32, 7, 1.0
    x, x_best, eta, sign = make_case(c, h, w, s, eps, seed=7)
    xd, xbd, etad, signd, idxd = (t.to(dev()) for t in (x, x_best, eta, sign, torch.tensor(IDX)))
    flags = torch.zeros(1, dtype=torch.int32, device=dev())
    rc, clean = propose(lib, xd, xbd, idxd, c, h, w, 3, 4, 20, 9, s, eps, etad, signd, flags)
    L.check(rc)
    assert int(flags.item()) == 0
    for bad in (float("nan"), float("inf")):
        xbn = xbd.clone()
        xbn[4, 1, 30, 31] = bad                                          # image 4 is row a = 3; the pixel is in neither window
        flags.zero_()
        rc, got = propose(lib, xd, xbn, idxd, c, h, w, 3, 4, 20, 9, s, eps, etad, signd, flags)
        L.check(rc)
        assert int(flags.item()) == L.FLAG_SQUARE_NONFINITE
        assert torch.equal(got[3].view(torch.int32), xbn[4].view(torch.int32))
        keep = [0, 1, 2, 4, 5, 6]
        assert torch.equal(got[keep], clean[keep])


def test_kernel_refuses_bad_arguments_without_a_launch():
    lib = L.load()
    c, h, w, s, eps = 3, 21, 27, 5, 1.0
    x, x_best, eta, sign = make_case(c, h, w, s, eps, seed=3)
    xd, xbd, etad, signd, idxd = (t.to(dev()) for t in (x, x_best, eta, sign, torch.tensor(IDX)))
    x_new = torch.full((len(IDX), c, h, w), SENTINEL, device=dev())
    bad = [dict(vh=17), dict(vw=23), dict(vh2=-1), dict(vw2=23), dict(vh2=17), dict(vh=-1), dict(s=0), dict(s=22), dict(eps=0.0),
           dict(eps=float("nan")), dict(eps=float("inf"))]
    for kw in bad:
        a = dict(vh=1, vw=2, vh2=10, vw2=20, s=s, eps=eps)
        a.update(kw)
        rc, _ = propose(lib, xd, xbd, idxd, c, h, w, a["vh"], a["vw"], a["vh2"], a["vw2"], a["s"], a["eps"], etad, signd, None, x_new)
        assert rc == L.RVLM_ERR_ARG, kw
        with pytest.raises(ValueError):
            L.check(rc)
    many = torch.zeros(1, 17, 8, 8, device=dev())
    rc = lib.rvlm_square_l2_propose(many.data_ptr(), many.data_ptr(), idxd.data_ptr(), 1, 17, 8, 8, 0, 0, 0, 0, 3, 1.0, etad.data_ptr(),
                                    signd.data_ptr(), many.data_ptr(), None, L.stream_ptr())
    assert rc == L.RVLM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(x_new == SENTINEL)
    rc, _ = propose(lib, xd, xbd, idxd, c, h, w, 16, 22, 0, 0, s, eps, etad, signd, None, x_new)    # the last admissible corner
    L.check(rc)
    assert not torch.any(x_new == SENTINEL)


# --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    z = load_golden("square_l2_tiny.npz")
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=int(z["weights_seed"]))
    clf_ref = V.ClassificationModelRef(cfg, w, torch.from_numpy(z["T"]), 100.0).eval()
    return z, cfg, w, clf_ref


def host_predict(clf_ref, calls):
    def predict(v):
        calls.append(tuple(v.shape))
        with torch.no_grad():
            return clf_ref(v.cpu()).to(v.device)
    return predict


def check_properties(adv, x, eps, robust):
    assert not bool(torch.isnan(adv).any())
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    assert float((adv.double() - x.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    keep = torch.as_tensor(robust, device=adv.device)
    assert torch.equal(adv[keep], x[keep])                               # unfooled images are returned unchanged


@pytest.mark.parametrize("tag", ["a", "b"])
def test_attack_vs_reference_golden(golden, tag):
    z, cfg, w, clf_ref = golden
    assert tag in z["settings"].tolist()
    calls = []
    x, y = torch.from_numpy(z["x"]).to(dev()), torch.from_numpy(z["y"]).to(dev())
    eps, nq = float(z[tag + "_eps"]), int(z[tag + "_n_queries"])
    bound = nq * tol(eps)
    atk = R.SquareAttack(host_predict(clf_ref, calls), norm="L2", n_queries=nq, eps=eps, p_init=.8,
                         n_restarts=int(z[tag + "_n_restarts"]), seed=int(z[tag + "_seed"]), loss=str(z[tag + "_loss"]),
                         resc_schedule=False)
    adv = atk.perturb(x.clone(), y.clone())
    assert len(calls) == int(z[tag + "_n_model_calls"])
    with torch.no_grad():
        robust = (clf_ref(adv.cpu()).max(1)[1] == y.cpu()).numpy()
    assert np.array_equal(robust, z[tag + "_robust"])
    err = np.abs(adv.cpu().numpy().astype(np.float64) - z[tag + "_adv"]).max()
    print(f"{tag}: max |adv - golden| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    check_properties(adv, x, eps, robust)
    torch.random.manual_seed(11)
    used, xb = atk.attack_single_run(x.clone(), y.clone())
    assert np.array_equal(used.cpu().numpy(), z[tag + "_run_queries"])
    err = np.abs(xb.cpu().numpy().astype(np.float64) - z[tag + "_run_x_best"]).max()
    print(f"{tag}: max |x_best - golden| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert int(atk.flags.item()) == 0


def test_through_autoattack_vs_reference_golden(golden):
    z, cfg, w, clf_ref = golden
    calls = []
    x, y = torch.from_numpy(z["x"]).to(dev()), torch.from_numpy(z["y"]).to(dev())
    eps, nq = float(z["aa_eps"]), int(z["aa_n_queries"])
    aa = R.AutoAttack(host_predict(clf_ref, calls), norm="L2", eps=eps, seed=0, verbose=False, version="custom",
                      attacks_to_run=["square"], device=dev())
    aa.square.n_queries = nq
    x_adv, y_adv = aa.run_standard_evaluation(x.clone(), y.clone(), bs=4, return_labels=True)
    assert len(calls) == int(z["aa_n_model_calls"])
    assert np.array_equal(y_adv.cpu().numpy(), z["aa_y_adv"])
    robust = (y_adv == y).cpu().numpy()
    assert np.array_equal(robust, z["aa_robust"])
    err = np.abs(x_adv.cpu().numpy().astype(np.float64) - z["aa_x_adv"]).max()
    print(f"aa: max |x_adv - golden| = {err:.3e} (bound {nq * tol(eps):.3e})")
    assert err <= nq * tol(eps)
    check_properties(x_adv, x, eps, robust)


def test_native_route(golden):
    z, cfg, w, _ = golden
    x, y = torch.from_numpy(z["x"]).to(dev()), torch.from_numpy(z["y"]).to(dev())
    eng = R.VitEngine(R.VitConfig(cfg.image_size, cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.out_dim, cfg.act),
                      {k: v.to(dev()) for k, v in w.items()}, precision="fp32", max_batch=8)
    clf = R.ClassificationModel(eng, torch.from_numpy(z["T"]).to(dev())).eval()
    eps, nq = float(z["a_eps"]), int(z["a_n_queries"])
    atk = R.SquareAttack(clf, norm="L2", n_queries=nq, eps=eps, p_init=.8, n_restarts=2, seed=5, loss="margin", resc_schedule=False)
    with torch.no_grad():
        y0 = clf(x).max(1)[1]
    adv = atk.perturb(x.clone(), y0.clone())
    with torch.no_grad():
        robust = (clf(adv).max(1)[1] == y0).cpu().numpy()
    check_properties(adv, x, eps, robust)
    assert int(atk.flags.item()) == 0
    assert bool((adv != x).flatten(1).any(1).cpu().numpy()[~robust].all())
    eng.close()


def test_full_size_bf16():
    cfg = V.VIT_L_14
    w = V.init_weights(cfg, seed=3)
    eng = R.VitEngine(R.VitConfig(cfg.image_size, cfg.patch, cfg.width, cfg.layers, cfg.heads, cfg.out_dim, cfg.act),
                      {k: v.to(dev()) for k, v in w.items()}, precision="bf16", max_batch=8)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(8, 3, 224, 224, generator=g).to(dev())
    T = torch.randn(cfg.out_dim, 10, generator=g)
    clf = R.ClassificationModel(eng, (T / T.norm(dim=0, keepdim=True)).to(dev())).eval()
    with torch.no_grad():
        y = clf(x).max(1)[1]
    before = eng.workspace_bytes()
    atk = R.SquareAttack(clf, norm="L2", n_queries=20, eps=3.0, p_init=.8, n_restarts=1, seed=0, resc_schedule=False)
    adv = atk.perturb(x.clone(), y.clone())
    with torch.no_grad():
        robust = (clf(adv).max(1)[1] == y).cpu().numpy()
    check_properties(adv, x, 3.0, robust)
    assert int(atk.flags.item()) == 0
    assert eng.workspace_bytes() == before
    eng.close()
