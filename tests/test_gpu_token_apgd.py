"""Batched token APGD (RVLM_HAS_TOKEN_APGD) on the GPU: rvlm_apgd_run_tokens against the same loop driven from the host over the
public entries (bit for bit), against the reference's own apgd() runs (tests/golden/token_apgd_tiny.npz), its exact properties, the
zero-gradient start, chunking, refusals and flags, and the trainer's eval_step_tokens."""
import functools

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.trainer import AdversarialTrainer
from robustvlm_amd.vlm_attacks import TokenLossModel, apgd as vlm_apgd
from oracle import vit_ref as V
from tests import token_apgd_cases as TC
from tests.gpu_helpers import dev, lib, st, record

pytestmark = pytest.mark.gpu

LARGE = {0: 32 / 255, 2: 6.0}          # norm_kind -> the large radius of the fixture
CFGS = {"tiny": V.VIT_TINY, "tiny2": V.VIT_TINY2,
        "s257": V.VitConfig(224, 14, 256, 2, 4, 64),        # B = 2: 514 rows - the persistent bf16 GEMM, the S = 257 flash backward
        "s577": V.VitConfig(336, 14, 128, 2, 2, 64)}        # S = 577: the loss scratch


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


def make_engine(cfg, w, precision, max_batch, **kw):
    return R.VitEngine(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, precision=precision, max_batch=max_batch, **kw)


def schedule(n_iter):
    """The host's checkpoint schedule (apgd.py:192-213, 329-351): [(k, do_check)] per iteration."""
    k = max(int(0.22 * n_iter), 1)
    n_iter_min, size_decr = max(int(0.06 * n_iter), 1), max(int(0.03 * n_iter), 1)
    counter3, out = 0, []
    for _ in range(n_iter):
        counter3 += 1
        do_check = int(counter3 == k)
        out.append((k, do_check))
        if do_check:
            counter3, k = 0, max(k - size_decr, n_iter_min)
    return out


def fwd_inputgrad(eng, x_adv, ref, sel, depth, ln_post, per, grad):
    L.check(lib().rvlm_vit_tokens_fwd_inputgrad(eng._h, x_adv.data_ptr(), None, x_adv.shape[0], depth, int(ln_post), sel, ref.data_ptr(),
                                                L.RED_NONE, None, per.data_ptr(), None, L.ptr(grad), st()),
            "rvlm_vit_tokens_fwd_inputgrad")


def host_loop(eng, x, x_init, ref, sel, depth, ln_post, kind, eps, n_iter, step0, rho=0.75):
    """apgd() over the public entries in the reference's order.  Returns (x_best, loss_best, x_last, trace [n_iter + 1, B], step)."""
    l, B, npix = lib(), x.shape[0], x[0].numel()
    x_adv = (x if x_init is None else x_init).clamp(0., 1.).contiguous()
    x_best, x_best_adv, x_old = x_adv.clone(), x_adv.clone(), x_adv.clone()
    f32 = dict(dtype=torch.float32, device=x.device)
    u8 = dict(dtype=torch.uint8, device=x.device)
    loss_steps, per, grad = torch.zeros(n_iter, B, **f32), torch.empty(B, **f32), torch.empty_like(x)
    fwd_inputgrad(eng, x_adv, ref, sel, depth, ln_post, per, grad)
    grad_best, loss_best, lbc = grad.clone(), per.clone(), per.clone()
    reduced, step = torch.ones(B, **f32), torch.full((B,), step0, **f32)
    pred, acc, f0, f1, f2 = (torch.zeros(B, **u8) for _ in range(5))
    trace = [per.clone()]
    step_fn = l.rvlm_apgd_l2_step if kind == 2 else l.rvlm_apgd_linf_step
    for i, (k, do_check) in enumerate(schedule(n_iter)):
        L.check(step_fn(x.data_ptr(), x_adv.data_ptr(), x_old.data_ptr(), grad.data_ptr(), step.data_ptr(), 0.75 if i > 0 else 1.0,
                        eps, npix, B, st()), "apgd step")
        fwd_inputgrad(eng, x_adv, ref, sel, depth, ln_post, per, grad if i < n_iter - 1 else None)
        L.check(l.rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, rho, per.data_ptr(), pred.data_ptr(), loss_steps.data_ptr(),
                                           loss_best.data_ptr(), lbc.data_ptr(), reduced.data_ptr(), step.data_ptr(), acc.data_ptr(),
                                           f0.data_ptr(), f1.data_ptr(), f2.data_ptr(), st()), "rvlm_apgd_controller_rho")
        L.check(l.rvlm_apgd_select(x_adv.data_ptr(), grad.data_ptr(), x_best.data_ptr(), grad_best.data_ptr(), x_best_adv.data_ptr(),
                                   f0.data_ptr(), f1.data_ptr(), f2.data_ptr(), npix, B, st()), "rvlm_apgd_select")
        trace.append(per.clone())
    return x_best, loss_best, x_best_adv, torch.stack(trace), step


def reproducible(eng, x, ref, sel, depth, ln_post):
    """rvlm_vit_tokens_fwd_inputgrad twice: the same bits?"""
    outs = []
    for _ in range(2):
        per, grad = torch.empty(x.shape[0], device=x.device), torch.empty_like(x)
        fwd_inputgrad(eng, x, ref, sel, depth, ln_post, per, grad)
        outs.append((per, grad))
    return torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def shapes_of(cfg):
    Lr = cfg.layers
    return ((Lr - 1, "patch", False), (Lr, "all", False), (Lr, "all", True))


@functools.lru_cache(maxsize=None)
def runs(cfg_name, precision, B, n_iters, max_batch):
    """Every (norm, shape, n_iter) case of one engine, fused and host-driven, computed once and shared by the tests that read it (CPU
    tensors; the engine is closed)."""
    cfg = CFGS[cfg_name]
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, precision, max_batch)
    g = torch.Generator().manual_seed(31)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g).to(dev())
    u = (torch.rand(x.shape, generator=g) * 2 - 1).to(dev())
    out = []
    for depth, select, ln_post in shapes_of(cfg):
        tok = eng.forward_tokens(x, depth=depth, ln_post=ln_post)
        ref = (tok[:, 1:] if select == "patch" else tok).contiguous()
        sel = L.TOKENS_PATCH if select == "patch" else L.TOKENS_ALL
        for kind in (0, 2):
            eps = LARGE[kind]
            p0 = eps * u if kind == 0 else 0.5 * eps * u / u.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
            x_init = (x + p0).contiguous()
            exact = reproducible(eng, x_init, ref, sel, depth, ln_post)
            for n_iter in n_iters:
                fused = eng.apgd_run_tokens(x, x_init, ref, eps, n_iter, 2 * eps, depth=depth, ln_post=ln_post, select=select,
                                            norm_kind=kind, want_trace=True, want_step=True)
                xb, lb, xl, flags, trace, step = fused
                host = host_loop(eng, x, x_init, ref, sel, depth, ln_post, kind, eps, n_iter, 2 * eps)
                per = torch.empty(B, device=x.device)
                fwd_inputgrad(eng, xb, ref, sel, depth, ln_post, per, None)            # the loss recomputed at x_best
                out.append(dict(case=(depth, select, ln_post, kind, n_iter), eps=eps, exact=exact, flags=int(flags.item()), x=x.cpu(),
                                fused=[t.cpu() for t in (xb, lb, xl, trace, step)], host=[t.cpu() for t in host], at_best=per.cpu()))
    eng.close()
    return out


SMALL = [pytest.param(c, p, 3, (1, 2, 10, 25), 4, id=f"{c}-{p}") for c in ("tiny", "tiny2") for p in ("fp32", "bf16")]
WIDE = [pytest.param("s257", "bf16", 2, (3,), 2, id="s257-bf16"), pytest.param("s577", "fp32", 2, (2,), 2, id="s577-fp32"),
        pytest.param("s577", "bf16", 2, (2,), 2, id="s577-bf16")]
NAMES = ("x_best", "loss_best", "x_last", "trace", "step")


def check_equal_to_host_loop(rs):
    for r in rs:
        if r["exact"]:
            for name, a, b in zip(NAMES, r["fused"], r["host"]):
                assert torch.equal(a, b), (r["case"], name, float((a - b).abs().max()))
        else:     # a forward / backward that is not bit-reproducible run to run: the traces agree to 1e-5 relative instead
            for i in (1, 3):
                torch.testing.assert_close(r["fused"][i], r["host"][i], rtol=1e-5, atol=0, msg=lambda m: f"{r['case']} {NAMES[i]}: {m}")
        assert r["flags"] == 0, (r["case"], r["flags"])


# ---- 1. the loop is the public entries in the reference's order ------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,precision,B,n_iters,max_batch", SMALL)
def test_fused_loop_equals_the_host_loop_over_the_public_entries(cfg_name, precision, B, n_iters, max_batch):
    """torch.equal on x_best, loss_best, x_last, the loss trace and the final step sizes.  Should rvlm_vit_tokens_fwd_inputgrad not be
    bit-reproducible run to run at some shape (it is called twice first), that shape's traces and best losses are compared to 1e-5
    relative instead; on the MI355X every shape here took the exact branch."""
    rs = runs(cfg_name, precision, B, n_iters, max_batch)
    assert len(rs) == 3 * 2 * len(n_iters)
    print(cfg_name, precision, "exact:", sum(r["exact"] for r in rs), "of", len(rs))
    check_equal_to_host_loop(rs)
    for r in rs:
        if r["case"][-1] == 25:           # the controller really ran: a step was halved
            assert float(r["fused"][4].min()) < np.float32(2 * r["eps"]), (r["case"], r["fused"][4])


# ---- 2. ... at the shapes where other kernels take over --------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,precision,B,n_iters,max_batch", WIDE)
def test_fused_loop_equals_the_host_loop_at_the_wide_shapes(cfg_name, precision, B, n_iters, max_batch):
    check_equal_to_host_loop(runs(cfg_name, precision, B, n_iters, max_batch))


# ---- 4. exact properties, every case of the first test ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,precision,B,n_iters,max_batch", SMALL)
def test_exact_properties(cfg_name, precision, B, n_iters, max_batch):
    for r in runs(cfg_name, precision, B, n_iters, max_batch):
        kind, eps, x = r["case"][3], r["eps"], r["x"]
        xb, lb, xl, trace, _ = r["fused"]
        for it in (xb, xl):
            assert float(it.min()) >= 0 and float(it.max()) <= 1, r["case"]
            if kind == 0:      # the ball in the arithmetic that made it: fl(x - eps) <= x_adv <= fl(x + eps), eps as float32, exactly
                e32 = torch.tensor(eps, dtype=torch.float32)
                assert bool((it <= x + e32).all()) and bool((it >= x - e32).all()), r["case"]
            else:
                assert float((it.double() - x.double()).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5), r["case"]
        assert torch.equal(lb, trace.max(dim=0).values), r["case"]
        torch.testing.assert_close(r["at_best"], lb, rtol=1e-5, atol=0, msg=lambda m: f"{r['case']}: {m}")


# ---- 3. against the reference's runs --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_runs():
    """Every case of the fixture on one fp32 engine: the fused loop on the batch and, at the large radii, the existing route -
    vlm_attacks.apgd(TokenLossModel(...)) one image at a time."""
    cases, get = TC.load()
    w = V.init_weights(V.VIT_TINY, seed=int(np.load(TC.PATH)["weights_seed"]))
    eng = make_engine(V.VIT_TINY, w, "fp32", 4)
    out = {}
    for c in cases:
        g = get(c["name"])
        x, p0 = torch.from_numpy(g["x"]).to(dev()), torch.from_numpy(g["pert_init"]).to(dev())
        tower = R.ClipVisionTower(eng, select_layer=c["depth"] - 3, select_feature="patch" if c["select"] == "patch" else "cls_patch")
        assert tower.depth == c["depth"]
        ref = tower(x).detach().contiguous()
        xb, lb, xl, trace = R.apgd_tokens(tower, x, ref, c["norm"], c["eps"], n_iter=c["n_iter"], pert_init=p0, return_trace=True)
        o = dict(x_best=xb.cpu().numpy(), loss_best=lb.cpu().numpy(), x_last=xl.cpu().numpy(), trace=trace.cpu().numpy())
        if c["radius"] == "large":
            one = []
            for b in range(x.shape[0]):
                shape6 = (1, 1, 1) + tuple(x.shape[1:])
                _, lb1, _ = vlm_apgd(TokenLossModel(tower, ref[b:b + 1]), x[b:b + 1].reshape(shape6), c["norm"], c["eps"],
                                     n_iter=c["n_iter"], pert_init=p0[b:b + 1].reshape(shape6))
                one.append(float(lb1))
            o["loss_best_single"] = np.array(one, np.float32)
        out[c["name"]] = o
    eng.close()
    return out


FIX_CASES = TC.load()[0]


def in_ball(case, it, x):
    assert it.min() >= 0 and it.max() <= 1
    if case["norm"] == "linf":       # fl(x - eps) <= x_adv <= fl(x + eps) in float32, exactly
        assert (it <= x + np.float32(case["eps"])).all() and (it >= x - np.float32(case["eps"])).all()
    else:
        B = x.shape[0]
        assert np.sqrt(((it.astype(np.float64) - x) ** 2).reshape(B, -1).sum(1)).max() <= case["eps"] * (1 + 1e-5)


@pytest.mark.parametrize("case", [c for c in FIX_CASES if c["radius"] == "small"], ids=lambda c: c["name"])
def test_small_radii_against_the_reference(case):
    """The bars of the pooled fused loop against its reference golden (test_fused_apgd_vs_reference_golden): identical pixels > 0.90
    (L-inf), loss_best within rtol 0.1."""
    got, g = fixture_runs()[case["name"]], TC.load()[1](case["name"])
    in_ball(case, got["x_best"], g["x"])
    in_ball(case, got["x_last"], g["x"])
    frac = float(np.mean(got["x_best"] == g["x_best"]))
    print(case["name"], "identical pixels", frac, "loss_best", got["loss_best"], "reference", g["loss_best"])
    if case["norm"] == "linf":
        assert frac > 0.90, frac
    np.testing.assert_allclose(got["loss_best"], g["loss_best"], rtol=0.1)


@pytest.mark.parametrize("case", [c for c in FIX_CASES if c["radius"] == "large"], ids=lambda c: c["name"])
def test_large_radii_deviate_no_more_than_the_single_image_route(case):
    """No pixel bar at the large radii (the controller amplifies single sign flips): the fused loop's worst relative deviation of
    loss_best from the reference is at most that of vlm_attacks.apgd(TokenLossModel(...)) - the same arithmetic one image at a time -
    plus 0.02."""
    got, g = fixture_runs()[case["name"]], TC.load()[1](case["name"])
    in_ball(case, got["x_best"], g["x"])
    dev_fused = float(np.max(np.abs(got["loss_best"] - g["loss_best"]) / g["loss_best"]))
    dev_single = float(np.max(np.abs(got["loss_best_single"] - g["loss_best"]) / g["loss_best"]))
    print(case["name"], "fused", dev_fused, "single", dev_single)
    record("token_apgd_large_radius/" + case["name"], fused_rel_dev=dev_fused, single_image_rel_dev=dev_single)
    assert dev_fused <= dev_single + 0.02, (dev_fused, dev_single)


# ---- 5. zero gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,eps", [("linf", 32 / 255), ("l2", 6.0)])
def test_zero_gradient_start_stays_put(norm, eps):
    cfg = V.VIT_TINY
    eng = make_engine(cfg, V.init_weights(cfg, seed=9), "fp32", 4)
    tower = R.ClipVisionTower(eng, select_layer=-2)
    x = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(dev())
    ref = tower(x).detach().contiguous()
    n_iter = 25
    xb, lb, xl, flags, trace, step = eng.apgd_run_tokens(x, None, ref, eps, n_iter, 2 * eps, depth=tower.depth, select="patch",
                                                         norm_kind=0 if norm == "linf" else 2, want_trace=True, want_step=True)
    assert torch.equal(xb, x.clamp(0, 1)) and torch.equal(xl, xb)
    assert not trace.any() and not lb.any()
    n_checks = sum(c for _, c in schedule(n_iter))        # a loss that never moves halves the step at every checkpoint, no more
    assert torch.equal(step, torch.full_like(step, float(np.float32(2 * eps)) * 0.5 ** n_checks))
    assert int(flags.item()) == 0
    out = R.apgd_tokens(tower, x, ref, norm, eps, n_iter=3)
    assert torch.equal(out[0], x) and not out[1].any()
    eng.close()


# ---- 6. chunking -------------------------------------------------------------------------------------------------------------------
def test_chunks_beyond_max_batch():
    cfg = V.VIT_TINY
    eng = make_engine(cfg, V.init_weights(cfg, seed=9), "fp32", 2)
    tower = R.ClipVisionTower(eng, select_layer=-1, select_feature="cls_patch")
    g = torch.Generator().manual_seed(2)
    x = torch.rand(5, 3, 32, 32, generator=g).to(dev())
    p0 = ((torch.rand(x.shape, generator=g) * 2 - 1) * (32 / 255)).to(dev())
    ref = torch.cat([tower(x[i:i + 2]).detach() for i in (0, 2, 4)])
    whole = R.apgd_tokens(tower, x, ref, "linf", 32 / 255, n_iter=10, pert_init=p0, return_trace=True)
    parts = [R.apgd_tokens(tower, x[a:b], ref[a:b], "linf", 32 / 255, n_iter=10, pert_init=p0[a:b], return_trace=True)
             for a, b in ((0, 2), (2, 4), (4, 5))]
    for j in range(3):
        assert torch.equal(whole[j], torch.cat([p[j] for p in parts]))
    assert torch.equal(whole[3], torch.cat([p[3] for p in parts], dim=1)) and whole[3].shape == (11, 5)
    eng.close()


# ---- 7. refusals and flags ----------------------------------------------------------------------------------------------------------
def test_refusals_and_flags():
    cfg = V.VIT_TINY
    w = V.init_weights(cfg, seed=9)
    eng = make_engine(cfg, w, "fp32", 2)
    tower = R.ClipVisionTower(eng, select_layer=-2)
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev())
    ref = tower(x).detach().contiguous()
    xb, lb, fl = torch.empty_like(x), torch.empty(2, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())

    def call(h=None, x_=x, B=2, ref_=ref, kind=0, n_iter=2, out=xb, depth=1, select=L.TOKENS_PATCH):
        return lib().rvlm_apgd_run_tokens(h or eng._h, L.ptr(x_), None, B, depth, 0, select, L.ptr(ref_), kind, 0.1, n_iter, 0.2, 0.75,
                                          L.ptr(out), lb.data_ptr(), None, None, None, fl.data_ptr(), st())
    assert call() == L.RVLM_OK
    assert call(ref_=None) == L.RVLM_ERR_ARG and call(x_=None) == L.RVLM_ERR_ARG and call(out=None) == L.RVLM_ERR_ARG
    assert call(kind=1) == L.RVLM_ERR_UNSUPPORTED
    assert call(n_iter=0) == L.RVLM_ERR_ARG and call(n_iter=1025) == L.RVLM_ERR_ARG
    assert call(B=3) == L.RVLM_ERR_ARG and call(B=0) == L.RVLM_ERR_ARG
    assert call(depth=0) == L.RVLM_ERR_ARG and call(depth=3) == L.RVLM_ERR_ARG and call(select=2) == L.RVLM_ERR_ARG
    torch.cuda.synchronize()
    assert int(fl.item()) == 0
    # through Python
    with pytest.raises(NotImplementedError):
        eng.apgd_run_tokens(x, None, ref, 0.1, 2, 0.2, depth=1, select="patch", norm_kind=1)
    for n_iter in (0, 1025):
        with pytest.raises(ValueError):
            eng.apgd_run_tokens(x, None, ref, 0.1, n_iter, 0.2, depth=1, select="patch")
    with pytest.raises(ValueError, match="max_batch"):
        eng.apgd_run_tokens(torch.cat([x, x]), None, torch.cat([ref, ref]), 0.1, 2, 0.2, depth=1, select="patch")
    with pytest.raises(L.RvlmError):
        R.apgd_tokens(tower, x.cpu(), ref, "linf", 0.1)
    # a handoff-precision engine: refused in Python, and its forward-provider handle by the C entry as by the other token passes
    mixed = make_engine(cfg, w, "bf16+x3fwd-first", 2)
    with pytest.raises(ValueError, match="plain precisions"):
        mixed.apgd_run_tokens(x, None, ref, 0.1, 2, 0.2, depth=1, select="patch")
    assert call(h=mixed._h32) == L.RVLM_ERR_STATE
    mixed.close()
    # a NaN reference: the flag, and the assertion pgd() raises on the token route
    bad = ref.clone()
    bad[1, 3, 5] = float("nan")
    flags = eng.apgd_run_tokens(x, None, bad, 0.1, 2, 0.2, depth=1, select="patch")[3]
    assert int(flags.item()) & L.FLAG_TOKENS_NONFINITE
    with pytest.raises(AssertionError, match="non-finite token loss"):
        R.apgd_tokens(tower, x, bad, "linf", 0.1, n_iter=2)
    eng.close()


# ---- 8. trainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_eval_step_tokens_leaves_training_alone():
    cfg = R.VitConfig(96, 16, 128, 3, 2, 48)
    w = {k: v.to(dev()) for k, v in V.init_weights(V.VIT_TINY2, seed=21).items()}
    kw = dict(batch_size=4, precision="fp32", lr=1e-3, wd=1e-2, warmup=2, steps=10, loss="l2-tokens", inner_loss="l2-tokens",
              attack="pgd", iterations_adv=2, token_depth=-2, token_select="patch")
    tr, twin = AdversarialTrainer(cfg, w, **kw), AdversarialTrainer(cfg, w, **kw)
    g = torch.Generator().manual_seed(8)
    x = torch.rand(4, 3, 96, 96, generator=g).to(dev())
    d0 = ((torch.rand(x.shape, generator=g) * 2 - 1) * tr.eps).to(dev())
    tr.model.train()
    before = (tr.params.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.grads.flat.clone(), tr.step_total, tr.cur_lr)
    logs = tr.eval_step_tokens(x, n_iter=5, pert_init=d0)
    assert set(logs) == {"eval/l2-tokens", "eval/l2-tokens-clean", "eval/cos-sim-tokens"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in logs.values()), logs
    assert logs["eval/l2-tokens-clean"] == 0.0                 # step 0: the trained and the frozen towers are the same tower
    assert logs["eval/l2-tokens"] >= logs["eval/l2-tokens-clean"] and logs["eval/l2-tokens"] > 0
    assert -1 <= logs["eval/cos-sim-tokens"] <= 1
    assert tr.model.training
    after = (tr.params.flat, tr.exp_avg, tr.exp_avg_sq, tr.grads.flat, tr.step_total, tr.cur_lr)
    for a, b in zip(before[:4], after[:4]):
        assert torch.equal(a, b)
    assert before[4:] == after[4:]
    tr.model.eval()
    tr.eval_step_tokens(x, n_iter=1, pert_init=d0)
    assert not tr.model.training
    tr.model.train()
    outs = []
    for t in (tr, twin):                                        # the twin never evaluated
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        outs.append(t.train_step(x, None))
    assert torch.equal(tr.params.flat, twin.params.flat) and torch.equal(tr.exp_avg, twin.exp_avg)
    assert torch.equal(tr.exp_avg_sq, twin.exp_avg_sq)
    assert float(outs[0]["loss"]) == float(outs[1]["loss"])
    pooled = AdversarialTrainer(cfg, w, batch_size=4, precision="fp32", attack="none")
    with pytest.raises(ValueError, match="l2-tokens"):
        pooled.eval_step_tokens(x)
    pooled.close()
    tr.close()
    twin.close()
