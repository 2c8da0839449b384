"""SGD with momentum on the device (``--opt sgd``, train/adversarial_training_clip.py:198-206): rvlm_sgd_step against
torch.optim.SGD, its two access paths against each other, its argument checks, and AdversarialTrainer(opt="sgd") - one step in
closed form, five steps against the reference's own train_one_epoch (tests/golden/train_step_sgd_tiny.npz), the optimizer file."""
import functools

import numpy as np
import pytest
import torch

import robustvlm_amd as R
from robustvlm_amd import _lib as L
from robustvlm_amd.config import parameter_order
from robustvlm_amd.trainer import AdversarialTrainer
from oracle import vit_ref as V
from tests.gpu_helpers import dev
from tests.helpers import load_golden, cfg_from_array, weights_from_golden

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

LR, MOMENTUM, WD = 1e-3, 0.9, 1e-2
# rvlm_sgd_step sweeps at most 4096 blocks x 256 threads x 4 floats per pass (AdamW's cap, 4-wide): one n just past a full sweep
N_PAST_ONE_SWEEP = 4096 * 256 * 4 + 1027


def to_cfg(c):
    return R.VitConfig(c.image_size, c.patch, c.width, c.layers, c.heads, c.out_dim, c.act)


@functools.lru_cache(maxsize=None)
def kernel_data(n):
    g = torch.Generator().manual_seed(3)
    return torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1


def on_device(t, offset=0):
    """A device copy of ``t`` whose first element sits ``offset`` floats behind a 16-byte boundary."""
    store = torch.zeros(t.numel() + 4, device=dev())
    assert store.data_ptr() % 16 == 0
    view = store[offset:offset + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * offset
    return view


def sgd_steps_on_device(n, momentum, wd, offset=0, steps=3):
    """``steps`` consecutive rvlm_sgd_step calls (gradient x step, uploaded x 2 with grad_scale 0.5); returns (params, buffer)."""
    l = L.load()
    p, grad = kernel_data(n)
    dp = on_device(p, offset)
    dbuf = on_device(torch.full((n,), 7.0), offset) if momentum != 0 else None      # first step: written, never read
    for step in range(1, steps + 1):
        dg = on_device(grad * step * 2, offset)          # grad_scale 0.5 undoes the x 2
        L.check(l.rvlm_sgd_step(dp.data_ptr(), dg.data_ptr(), L.ptr(dbuf), n, LR, momentum, wd, int(step == 1), 0.5,
                                L.stream_ptr()), "rvlm_sgd_step")
        torch.cuda.synchronize()
    return dp.cpu(), None if dbuf is None else dbuf.cpu()


# n: tail only / vector only / both / one element range past a full sweep of the grid (the grid-stride loop)
@pytest.mark.parametrize("n", [5, 8192, 10007, N_PAST_ONE_SWEEP])
@pytest.mark.parametrize("momentum,wd", [(MOMENTUM, WD), (MOMENTUM, 0.0), (0.0, WD)], ids=["momentum_wd", "momentum", "plain_nullbuf"])
def test_sgd_kernel_vs_torch(n, momentum, wd):
    p, grad = kernel_data(n)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=LR, momentum=momentum, weight_decay=wd)
    for step in range(1, 4):
        pt.grad = grad.clone() * step
        opt.step()
    got_p, got_buf = sgd_steps_on_device(n, momentum, wd)
    np.testing.assert_allclose(got_p.numpy(), pt.detach().numpy(), rtol=2e-5, atol=2e-7)
    if momentum != 0:
        np.testing.assert_allclose(got_buf.numpy(), opt.state[pt]["momentum_buffer"].numpy(), rtol=2e-5, atol=2e-7)
    else:
        assert got_buf is None and "momentum_buffer" not in opt.state[pt]


@pytest.mark.parametrize("n", [5, 10007, N_PAST_ONE_SWEEP])
@pytest.mark.parametrize("momentum", [MOMENTUM, 0.0])
def test_sgd_kernel_is_bit_identical_on_both_access_paths(n, momentum):
    """The same data behind 16-byte-aligned pointers (16-byte accesses + scalar tail) and behind views offset by one float (scalar
    accesses): the update is elementwise, so parameters and buffers are the same bits."""
    p_a, buf_a = sgd_steps_on_device(n, momentum, WD, offset=0)
    p_m, buf_m = sgd_steps_on_device(n, momentum, WD, offset=1)
    assert torch.equal(p_a, p_m)
    if momentum != 0:
        assert torch.equal(buf_a, buf_m)


def test_sgd_kernel_bad_arguments():
    l = L.load()
    n = 1000
    p, grad = kernel_data(n)
    dp, dg, dbuf = on_device(p), on_device(grad), on_device(torch.full((n,), 0.25))
    call = lambda params, grads, buf, momentum, count=n: L.check(       # noqa: E731
        l.rvlm_sgd_step(params, grads, buf, count, LR, momentum, WD, 0, 1.0, L.stream_ptr()), "rvlm_sgd_step")
    with pytest.raises(ValueError, match="rvlm_sgd_step"):
        call(None, dg.data_ptr(), dbuf.data_ptr(), MOMENTUM)
    with pytest.raises(ValueError, match="rvlm_sgd_step"):
        call(dp.data_ptr(), None, dbuf.data_ptr(), MOMENTUM)
    with pytest.raises(ValueError, match="rvlm_sgd_step"):
        call(dp.data_ptr(), dg.data_ptr(), None, MOMENTUM)
    with pytest.raises(ValueError, match="rvlm_sgd_step"):
        call(dp.data_ptr(), dg.data_ptr(), dbuf.data_ptr(), -0.1)
    assert l.rvlm_sgd_step(dp.data_ptr(), dg.data_ptr(), dbuf.data_ptr(), 0, LR, MOMENTUM, WD, 0, 1.0, L.stream_ptr()) == L.RVLM_OK
    torch.cuda.synchronize()
    # nothing was launched: the tensors are what was uploaded
    assert torch.equal(dp.cpu(), p) and torch.equal(dg.cpu(), grad) and bool((dbuf == 0.25).all())
    # momentum == 0: a buffer that is passed anyway is neither read nor written
    call(dp.data_ptr(), dg.data_ptr(), dbuf.data_ptr(), 0.0)
    torch.cuda.synchronize()
    assert bool((dbuf == 0.25).all()) and not torch.equal(dp.cpu(), p)


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def tiny_problem(B=4, seed=4):
    cfg = V.VIT_TINY2
    w = V.init_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, cfg.image_size, cfg.image_size, generator=g)
    xa = (x + 0.03 * (torch.rand(x.shape, generator=g) * 2 - 1)).clamp(0, 1)
    return cfg, w, x, xa


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_first_train_step_is_the_plain_sgd_update(precision):
    """params = p0 - lr * (grads / world + wd * p0) and momentum_buffer = the bracket, from the trainer's own gradient buffer:
    pins the wiring (pointers, lr, wd, grad_scale, first) whatever the engine's gradient precision."""
    cfg, w, x, xa = tiny_problem()
    lr, wd = 1e-3, 1e-2
    tr = AdversarialTrainer(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, batch_size=4, precision=precision, lr=lr, wd=wd,
                            warmup=2, steps=10, attack="none", opt="sgd", momentum_sgd=0.9)
    p0 = tr.params.flat.double().cpu()
    out = tr.train_step(x.to(dev()), None, data_adv=xa.to(dev()))
    torch.cuda.synchronize()
    assert out["lr"] == lr and tr.step_total == 1 and tr.world == 1
    g = tr.grads.flat.double().cpu()
    assert float(g.abs().max()) > 0
    bracket = g / tr.world + wd * p0
    np.testing.assert_allclose(tr.momentum_buffer.cpu().numpy(), bracket.numpy(), rtol=2e-5, atol=2e-7)
    np.testing.assert_allclose(tr.params.flat.cpu().numpy(), (p0 - lr * bracket).numpy(), rtol=2e-5, atol=2e-7)
    assert not torch.equal(tr.params.flat.double().cpu(), p0)
    tr.close()


TRAIN_CASES = {
    "fare_pgd": dict(attack="pgd", loss="l2", inner_loss="l2", clean_weight=0.0, trades=False, output_normalize=False),
    "tecoa_pgd": dict(attack="pgd", loss="ce", inner_loss="ce", clean_weight=0.0, trades=False, output_normalize=True),
    "none_cw": dict(attack="none", loss="ce", inner_loss="ce", clean_weight=0.5, trades=False, output_normalize=True),
}


def assert_tensor_within(tag, got, ref, bar=1e-2):
    """EVERY element of ``got`` within ``bar`` x the reference's largest magnitude in that tensor (fp64); returns the worst ratio."""
    got, ref = got.double().cpu().reshape(-1), ref.double().reshape(-1)
    vmax = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= bar * vmax, f"{tag}: element error {err:.3e} = {err / vmax:.3e} of the reference's largest {vmax:.3e}"
    return err / vmax


def snapshot(name, s):
    """The reference's parameters (and, for s = 3, 5, momentum buffers) after step s: {key: tensor}, {key: tensor}."""
    z = load_golden(f"train_step_sgd_tiny_{name}_s{s}.npz")
    pick = lambda pre: {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}   # noqa: E731
    return pick("w::"), pick("buf::")


def fixture_trainer(z, zin, name, **extra):
    cfg, w = cfg_from_array(zin["cfg"]), weights_from_golden(zin)
    tr = AdversarialTrainer(to_cfg(cfg), {k: v.to(dev()) for k, v in w.items()}, batch_size=zin["x"].shape[1], precision="fp32",
                            lr=float(z[f"{name}::lr"]), wd=float(z["wd"]), warmup=int(z["warmup"]), steps=int(z["steps"]),
                            embedding_text_labels_norm=torch.from_numpy(zin["T"]).to(dev()), loss_clean="l2",
                            eps=float(zin["eps"]), opt="sgd", momentum_sgd=float(z["momentum"]), **TRAIN_CASES[name], **extra)
    return tr, w


def buffer_piece(tr, k):
    o, c = tr.params.offsets[k]
    return tr.momentum_buffer[o:o + c].view(tr.params.shapes[k])


def fixture_step(tr, z, zin, name, s):
    """Step s + 1 of the reference's run on its batch and adversarial batch; learning rates exact, logged values at the bounds of
    test_train_step_vs_reference_train_one_epoch."""
    x, y = torch.from_numpy(zin["x"][s]).to(dev()), torch.from_numpy(zin["y"][s]).to(dev())
    xa = torch.from_numpy(z[f"{name}::x_adv"][s]).to(dev()) if f"{name}::x_adv" in z.files else x
    out = tr.train_step(x, y, data_adv=xa)
    assert out["lr"] == float(z[f"{name}::lr_used"][s]), (s, out["lr"])
    assert tr.cur_lr == float(z[f"{name}::lr_after"][s])
    for key in ("loss", "loss_total", "cos_sim_clean", "cos_sim"):
        got, want = float(out[key]), float(z[f"{name}::{key}"][s])
        assert abs(got - want) <= 2e-3 * abs(want) + 2e-5, (s, key, got, want)
    assert out["acc"] == float(z[f"{name}::acc"][s]) and out["racc"] == float(z[f"{name}::racc"][s]), s


def assert_state_within(tr, name, s, w0):
    """After step s: every tensor's update w_s - w_0 within 1e-2 of the reference's largest |w_s - w_0| in that tensor and, where the
    fixture holds them (s = 3, 5), every momentum buffer within 1e-2 of the largest |buffer| of that tensor."""
    ref_w, ref_buf = snapshot(name, s)
    sd, worst = tr.state_dict(), 0.0
    assert list(ref_w) == list(w0) and (not ref_buf or list(ref_buf) == list(w0))
    for k in w0:
        worst = max(worst, assert_tensor_within(f"step {s} update of {k}", sd[k].double().cpu() - w0[k].double(),
                                                ref_w[k].double() - w0[k].double()))
    for k in ref_buf:
        worst = max(worst, assert_tensor_within(f"step {s} momentum buffer of {k}", buffer_piece(tr, k), ref_buf[k]))
    return worst


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_sgd_train_step_vs_reference_train_one_epoch(name):
    """AdversarialTrainer(opt="sgd").train_step (fp32 engine) on the batches and adversarial batches of the reference's
    train_one_epoch under torch.optim.SGD(momentum 0.9, wd 1e-2): learning rates exactly, losses / cos-sims within
    2e-3 |want| + 2e-5, acc / racc equal; after steps 1, 3, 5 every tensor's update w_s - w_0 within 1e-2 of the reference's largest
    |w_s - w_0| in that tensor, after steps 3, 5 every momentum buffer within 1e-2 of the largest |buffer| of that tensor (the
    engine's fp32 weight gradients are held to 2e-3 of autograd; five momentum steps add up at most five of those).  The inputs are
    train_step_tiny.npz's (same seeds)."""
    z, zin = load_golden("train_step_sgd_tiny.npz"), load_golden("train_step_tiny.npz")
    tr, w = fixture_trainer(z, zin, name)
    worst = 0.0
    for s in range(zin["x"].shape[0]):
        fixture_step(tr, z, zin, name, s)
        if s + 1 in (1, 3, 5):
            worst = max(worst, assert_state_within(tr, name, s + 1, w))
    print(f"{name}: worst update / buffer error {worst:.3e} of the tensor's largest (bound 1e-2)")
    tr.close()


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_sgd_resume_from_a_state_the_reference_wrote(name):
    """The reference's run interrupted after step 3: its parameters, and its optimizer state in the layout
    torch.optim.SGD(visual.parameters()).state_dict() has (momentum buffers by positional index, the param group with the lr the
    scheduler left behind), loaded with start_step=3 into a fresh trainer; steps 4 - 5 there land within the 1e-2 bound on the
    reference's step-5 parameters and buffers, at the reference's learning rates."""
    z, zin = load_golden("train_step_sgd_tiny.npz"), load_golden("train_step_tiny.npz")
    tr, w = fixture_trainer(z, zin, name)
    w3, buf3 = snapshot(name, 3)
    order = parameter_order(tr.cfg)
    assert sorted(order) == sorted(w3) == sorted(buf3)
    sd = {"state": {i: {"momentum_buffer": buf3[k].clone()} for i, k in enumerate(order)},
          "param_groups": [dict(lr=float(z[f"{name}::lr_after"][2]), momentum=float(z["momentum"]), dampening=0,
                                weight_decay=float(z["wd"]), nesterov=False, maximize=False, foreach=None, differentiable=False,
                                fused=None, params=list(range(len(order))))]}
    params = [torch.nn.Parameter(w3[k].clone()) for k in order]             # it is a file torch's own SGD takes
    torch.optim.SGD(params, lr=1.0, momentum=0.1).load_state_dict(sd)
    tr.load_state_dict({k: v.to(dev()) for k, v in w3.items()})
    with pytest.raises(ValueError, match="start_step"):
        tr.load_optimizer_state_dict(sd)
    tr.load_optimizer_state_dict(sd, start_step=3)
    assert tr.step_total == 3 and tr.cur_lr == float(z[f"{name}::lr_after"][2])
    for k in order:
        assert torch.equal(buffer_piece(tr, k).cpu(), buf3[k]), k
    for s in (3, 4):                                                          # steps 4 - 5
        fixture_step(tr, z, zin, name, s)
    worst = assert_state_within(tr, name, 5, w)
    print(f"{name}: resumed at step 3, worst step-5 update / buffer error {worst:.3e} of the tensor's largest (bound 1e-2)")
    tr.close()


def test_sgd_optimizer_file_and_resume(tmp_path):
    """The optimizer file is torch.optim.SGD's own layout (loads into a real SGD over visual.parameters()-ordered tensors); resuming
    from the files with start_step reproduces the uninterrupted run bit for bit; a file without a step needs start_step; a file of
    the other optimizer is refused either way."""
    cfg, w, x, xa = tiny_problem()
    wd_ = {k: v.to(dev()) for k, v in w.items()}
    kw = dict(batch_size=4, precision="bf16", lr=1e-3, wd=1e-2, warmup=2, steps=10, attack="none")
    xd, xad = x.to(dev()), xa.to(dev())
    order = parameter_order(to_cfg(cfg))
    tr = AdversarialTrainer(to_cfg(cfg), wd_, opt="sgd", momentum_sgd=0.9, **kw)
    fresh = tr.optimizer_state_dict()
    assert fresh["state"] == {} and fresh["param_names"] == order          # torch creates the entries in its first step
    for _ in range(3):
        tr.train_step(xd, None, data_adv=xad)
    out_dir = str(tmp_path / "run_temp")
    final_dir = R.CheckpointWriter(out_dir, steps=10).final(tr.state_dict(), tr.optimizer_state_dict())
    sd = R.load_visual_state_dict(f"{final_dir}/checkpoints/final.pt", to_cfg(cfg))
    opt_sd = torch.load(f"{final_dir}/checkpoints/final_opt.pt")
    assert sorted(opt_sd["state"]) == list(range(len(order))) and list(opt_sd["state"][0]) == ["momentum_buffer"]
    assert opt_sd["param_groups"] == [dict(lr=tr.cur_lr, momentum=0.9, dampening=0, weight_decay=1e-2, nesterov=False,
                                           maximize=False, foreach=None, differentiable=False, fused=None,
                                           params=list(range(len(order))))]
    params = [torch.nn.Parameter(sd[k].clone()) for k in order]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.5, nesterov=False)
    opt.load_state_dict(opt_sd)
    assert opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["nesterov"] is False
    assert opt.param_groups[0]["lr"] == tr.cur_lr and opt.param_groups[0]["weight_decay"] == 1e-2
    o, c = tr.params.offsets[order[5]]
    assert torch.equal(opt.state[params[5]]["momentum_buffer"].reshape(-1), tr.momentum_buffer[o:o + c].cpu())
    # resume (…clip.py:98-102,207-208): SGD's file holds no step, the reference passes --start_step next to --optimizer_state
    tr2 = AdversarialTrainer(to_cfg(cfg), wd_, opt="sgd", momentum_sgd=0.9, **kw)
    tr2.load_state_dict(sd)
    with pytest.raises(ValueError, match="start_step"):
        tr2.load_optimizer_state_dict(opt_sd)
    tr2.load_optimizer_state_dict(opt_sd, start_step=3)
    assert tr2.step_total == 3 and tr2.cur_lr == tr.cur_lr
    for _ in range(2):                                                      # steps 4 - 5
        a = tr.train_step(xd, None, data_adv=xad)
        b = tr2.train_step(xd, None, data_adv=xad)
        assert float(a["loss"]) == float(b["loss"]) and a["lr"] == b["lr"]
    assert torch.equal(tr.params.flat, tr2.params.flat) and torch.equal(tr.momentum_buffer, tr2.momentum_buffer)
    # the other optimizer's file, both ways; the refusal names both
    tra = AdversarialTrainer(to_cfg(cfg), wd_, **kw)
    tra.train_step(xd, None, data_adv=xad)
    adamw_sd, p_before = tra.optimizer_state_dict(), tr2.params.flat.clone()
    for trainer, file in ((tr2, adamw_sd), (tra, opt_sd), (tra, fresh)):
        with pytest.raises(ValueError, match=r"(?s)(adamw.*sgd|sgd.*adamw)"):
            trainer.load_optimizer_state_dict(file, start_step=3)
    assert torch.equal(tr2.params.flat, p_before)
    tr.close(); tr2.close(); tra.close()


def optimizer_buffers(tr):
    """The parameter-sized device tensors a trainer holds besides its parameters and gradients."""
    mine = {tr.params.flat.data_ptr(), tr.grads.flat.data_ptr()}
    return [k for k, v in vars(tr).items()
            if isinstance(v, torch.Tensor) and v.numel() == tr.params.numel and v.data_ptr() not in mine]


def test_sgd_trainer_holds_one_optimizer_buffer_and_none_without_momentum():
    cfg, w, x, xa = tiny_problem()
    wd_ = {k: v.to(dev()) for k, v in w.items()}
    kw = dict(batch_size=4, precision="bf16", lr=1e-3, wd=1e-2, warmup=2, steps=10, attack="none")
    tr = AdversarialTrainer(to_cfg(cfg), wd_, opt="sgd", **kw)                       # momentum_sgd defaults to 0.9
    assert optimizer_buffers(tr) == ["momentum_buffer"] and tr.momentum_sgd == 0.9 and not hasattr(tr, "exp_avg")
    tr.close()
    tr = AdversarialTrainer(to_cfg(cfg), wd_, opt="sgd", momentum_sgd=0, **kw)
    assert optimizer_buffers(tr) == [] and tr.momentum_buffer is None
    p0 = tr.params.flat.double().cpu()
    tr.train_step(x.to(dev()), None, data_adv=xa.to(dev()))                          # the NULL-buffer call through the trainer
    want = p0 - 1e-3 * (tr.grads.flat.double().cpu() + 1e-2 * p0)
    np.testing.assert_allclose(tr.params.flat.cpu().numpy(), want.numpy(), rtol=2e-5, atol=2e-7)
    assert tr.optimizer_state_dict()["state"] == {} and optimizer_buffers(tr) == []
    tr.close()
    tr = AdversarialTrainer(to_cfg(cfg), wd_, **kw)                                  # the default is what it was
    assert tr.opt == "adamw" and sorted(optimizer_buffers(tr)) == ["exp_avg", "exp_avg_sq"]
    tr.close()
