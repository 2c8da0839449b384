"""Per-row fp64 parity of the encoder's non-GEMM kernels at every shape specialisation (through include/rvlm_kernels.h).

Whole-tensor cosines and max-over-tensor bars cannot see ONE wrong row (the odd key of S = 257, one head of the persistent walk, one
32-row tile): every output row here is held to its own relative L2 bar (tests/gpu_helpers.py row_rel_l2) against an fp64 torch
reference on the device, computed from the same rounded inputs the kernel reads.  Output buffers are allocated by the test with their
documented padding, pre-filled with a sentinel and fenced by guard rows: rows a kernel must not write are checked by value."""
import ctypes as C
import math

import pytest
import torch

from robustvlm_amd import _lib as L
from tests.gpu_helpers import dev, st, lib, record, assert_rows, act_ref, dact_ref

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
GUARD = 64              # guard rows in front of and behind every output
SENT_BF, SENT_F = 768.0, -12345.0      # sentinels (exact in bf16 / fp32)
NAN_BITS = 0x7FC1       # a bf16 NaN bit pattern no kernel produces


def guarded(rows, cols, dtype, fill):
    """(whole buffer, the [rows, cols] view a kernel is handed): GUARD rows of `fill` on either side."""
    buf = torch.full((rows + 2 * GUARD, cols), fill, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf, rows, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + rows:] == fill).all())


def guarded_nan(rows, cols):
    buf = torch.full((rows + 2 * GUARD, cols), NAN_BITS, dtype=torch.int16, device=dev())
    return buf, buf[GUARD:GUARD + rows]


def nan_guards_intact(buf, rows):
    return bool((buf[:GUARD] == NAN_BITS).all()) and bool((buf[GUARD + rows:] == NAN_BITS).all())


def bits(t):
    return t.contiguous().view(torch.int16)


def bhsd(t, B, H, S):
    """[B*S, H*64] -> [B, H, S, 64]"""
    return t.reshape(B, S, H, 64).permute(0, 2, 1, 3)


def round_up(a, b):
    return (a + b - 1) // b * b


# --------------------------------------------------------------------------------------------------------------------------
# 1. bf16 flash attention, forward and backward
# --------------------------------------------------------------------------------------------------------------------------
def attn_form(S, use_tr):
    """The kernels attn_fwd_bf16 / attn_bwd_bf16 run at this sequence length (the host rules of csrc/attention_bf16.hip, restated
    for the record): S = 257 with transposing reads takes the 8-wave odd-token forward and the fused backward; everything else the
    generic kernels, `waves` waves walking ceil(tiles / waves) rounds, K / V of the dK / dV kernel LDS-resident up to 288 rows."""
    tiles = round_up(S, 32) // 32
    if S == 257 and use_tr:
        return dict(odd=1, waves=8, rounds=1, resident=1)
    rounds = (tiles + 9) // 10
    return dict(odd=0, waves=(tiles + rounds - 1) // rounds, rounds=rounds, resident=int(round_up(S, 32) * 520 <= 160 * 1024))


def attn_inputs(B, H, S, family, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, S, 3, H, 64, generator=g, device=dev())
    if family == "peaked":
        x[:, :, 0:2] *= math.sqrt(6.0)                   # scores q.k / 8 with a standard deviation of about 6
        if S == 257:                                       # a dominant ODD key, and a dominant key for the ODD query
            for qi in (5, 131):
                x[:, qi, 0] = 1.5 * x[:, 256, 1]
            x[:, 256, 0] = 1.5 * x[:, 40, 1]
    d_o = torch.randn(B * S, H * 64, generator=g, device=dev())
    return x.reshape(B * S, 3 * H * 64).bfloat16(), d_o.bfloat16()


def attn_reference(qkv, d_o, B, H, S):
    """fp64: o, lse2 (log2 domain), d(qkv) for the cotangent d_o - all as [B, H, S, 64] / [B, H, S]."""
    W = H * 64
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    o = torch.softmax(s, -1) @ v
    lse2 = torch.logsumexp(s, -1) * LOG2E
    (gx,) = torch.autograd.grad((o * bhsd(d_o.double(), B, H, S)).sum(), x)
    return o.detach(), lse2.detach(), [bhsd(gx[:, i * W:(i + 1) * W], B, H, S) for i in range(3)]


def attn_backward_reference(qkv, o, lse2, d_o, B, H, S):
    """The flash backward in fp64 on what the KERNEL reads: q, k, v, dO, the bf16 o and the lse2 rows its forward stored.
    D = rowsum(dO o) and P = exp2(s log2(e) - lse2) are functions of those rounded tensors; under a peaked softmax dP - D cancels
    (P -> 1: dP of the dominant key equals D up to 1 - P), so the bf16 rounding of o is part of the backward's input, not an error of
    its arithmetic - against the autograd gradient of the exact forward it shows as tens of percent in rows whose true dQ is nearly zero."""
    q, k, v = qkv.double().reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    do = bhsd(d_o.double(), B, H, S)
    p = torch.exp2((q @ k.transpose(-1, -2)) * (0.125 * LOG2E) - lse2.double()[..., None])
    ds = p * (do @ v.transpose(-1, -2) - (do * bhsd(o.double(), B, H, S)).sum(-1, keepdim=True))
    return (ds @ k) * 0.125, (ds.transpose(-1, -2) @ q) * 0.125, p.transpose(-1, -2) @ do


# Per-(image, head, row) bars.  What the formats allow (bf16 storage of q, k, v, P, dS and of the results) caps them at o 8e-3, lse2 2e-2,
# dq / dk / dv 2e-2; each is set at no more than 3x the worst value seen over every case below on an MI355X (o 4.7e-3, lse2 1.9e-5, dq
# 5.6e-3, dk 5.1e-3, dv 4.9e-3) and never above its cap.
ATTN_BARS = {"o": 8e-3, "lse2": 5e-5, "dq": 1.5e-2, "dk": 1.5e-2, "dv": 1.4e-2}
# class-token kernels (fp32 softmax, one query): seen o 2.2e-3, lse 1.3e-6, dq 2.1e-3, dk 2.5e-3, dv 2.7e-3
CLS_BARS = {"o": 6e-3, "lse": 3.9e-6, "dq": 6e-3, "dk": 7e-3, "dv": 8e-3}

ATTN_SHAPES = [(2, 2, 32), (2, 3, 33), (2, 2, 64), (2, 12, 197), (2, 4, 257), (20, 16, 257), (2, 2, 288), (2, 2, 289), (2, 2, 320),
               (2, 2, 321), (1, 3, 352), (1, 2, 577), (1, 2, 608)]
ATTN_CASES = [(b, h, s, 1) for b, h, s in ATTN_SHAPES] + [(2, 3, 33, 0), (2, 4, 257, 0), (1, 2, 577, 0)]


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("B,H,S,use_tr", ATTN_CASES)
def test_attention_bf16_rows(B, H, S, use_tr, family):
    l = lib()
    W, Sp = H * 64, round_up(S, 32)
    qkv, d_o = attn_inputs(B, H, S, family, 1000 * S + B * H + use_tr)
    o_ref, lse_ref, (dq_ref, dk_ref, dv_ref) = attn_reference(qkv, d_o, B, H, S)
    o_buf, o = guarded(B * S, W, torch.bfloat16, SENT_BF)
    lse_buf, lse = guarded(B * H, Sp, torch.float32, SENT_F)
    ds_buf, dsum = guarded(B * H, Sp, torch.float32, SENT_F)
    dq_buf, dqkv = guarded(B * S, 3 * W, torch.bfloat16, SENT_BF)
    l.rvlm_k_attn_set_use_tr(use_tr)
    try:
        L.check(l.rvlm_k_attn_fwd_bf16(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, S, st()))
        L.check(l.rvlm_k_attn_bwd_bf16(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dsum.data_ptr(),
                                       dqkv.data_ptr(), B, H, S, st()))
        torch.cuda.synchronize()
    finally:
        l.rvlm_k_attn_set_use_tr(1)
    tag = f"B{B} H{H} S{S} tr{use_tr} {family}"
    worst = {"o": assert_rows(f"o {tag}", bhsd(o, B, H, S), o_ref, ATTN_BARS["o"])}
    lse3 = lse.reshape(B, H, Sp)
    worst["lse2"] = float((lse3[:, :, :S].double() - lse_ref).abs().max())
    assert worst["lse2"] <= ATTN_BARS["lse2"], (tag, worst["lse2"])
    flash_ref = attn_backward_reference(qkv, o, lse3[:, :, :S], d_o, B, H, S)
    for i, (name, ref, fref) in enumerate(zip(("dq", "dk", "dv"), (dq_ref, dk_ref, dv_ref), flash_ref)):
        got = bhsd(dqkv[:, i * W:(i + 1) * W], B, H, S)
        worst[name] = assert_rows(f"{name} {tag}", got, fref, ATTN_BARS[name])
        if family == "randn":           # ... and the formula is the gradient: a flat softmax has no cancellation in dP - D
            assert_rows(f"{name} vs autograd {tag}", got, ref, ATTN_BARS[name])
    # rows >= S of the log-sum-exp and D buffers are padding nobody writes; nothing lands outside the buffers
    assert bool((lse3[:, :, S:] == SENT_F).all()), f"{tag}: lse2 rows >= S written"
    assert bool((dsum.reshape(B, H, Sp)[:, :, S:] == SENT_F).all()), f"{tag}: dsum rows >= S written"
    assert guards_intact(o_buf, B * S, SENT_BF) and guards_intact(dq_buf, B * S, SENT_BF), f"{tag}: o / dqkv overrun"
    assert guards_intact(lse_buf, B * H, SENT_F) and guards_intact(ds_buf, B * H, SENT_F), f"{tag}: lse2 / dsum overrun"
    record("attention_bf16_rows", B=B, H=H, S=S, use_tr=use_tr, peaked=family == "peaked", **attn_form(S, use_tr), **worst)


def test_attention_bf16_sequence_limits():
    """160 KiB of LDS: the forward takes S <= 640, the backward S <= 608.  Beyond them the launchers return RVLM_ERR_UNSUPPORTED before
    anything is enqueued - the backward's first kernel (which writes dsum) included."""
    l = lib()
    B, H = 1, 1
    for S, fwd_ok in ((640, True), (641, False)):
        Sp = round_up(S, 32)
        qkv, _ = attn_inputs(B, H, S, "randn", S)
        o_buf, o = guarded(B * S, 64, torch.bfloat16, SENT_BF)
        lse_buf, lse = guarded(B * H, Sp, torch.float32, SENT_F)
        rc = l.rvlm_k_attn_fwd_bf16(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, S, st())
        torch.cuda.synchronize()
        if fwd_ok:
            assert rc == L.RVLM_OK
            o_ref, lse_ref, _ = attn_reference(qkv, torch.zeros(B * S, 64, device=dev()), B, H, S)
            w = assert_rows(f"o S{S}", bhsd(o, B, H, S), o_ref, ATTN_BARS["o"])
            assert float((lse[:, :S].double() - lse_ref[0]).abs().max()) <= ATTN_BARS["lse2"]
            record("attention_bf16_rows", B=B, H=H, S=S, use_tr=1, peaked=0, **attn_form(S, 1), o=w)
        else:
            assert rc == L.RVLM_ERR_UNSUPPORTED
            assert bool((o == SENT_BF).all()) and bool((lse == SENT_F).all())
        assert guards_intact(o_buf, B * S, SENT_BF) and guards_intact(lse_buf, B * H, SENT_F)
    S = 609
    Sp = round_up(S, 32)
    qkv, d_o = attn_inputs(B, H, S, "randn", S)
    o = torch.zeros(B * S, 64, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(B * H, Sp, device=dev())
    ds_buf, dsum = guarded(B * H, Sp, torch.float32, SENT_F)
    dq_buf, dqkv = guarded(B * S, 192, torch.bfloat16, SENT_BF)
    rc = l.rvlm_k_attn_bwd_bf16(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dsum.data_ptr(), dqkv.data_ptr(),
                                B, H, S, st())
    torch.cuda.synchronize()
    assert rc == L.RVLM_ERR_UNSUPPORTED
    assert bool((dsum == SENT_F).all()) and bool((dqkv == SENT_BF).all()), "the dQ kernel ran before the size check refused the call"
    assert guards_intact(ds_buf, B * H, SENT_F) and guards_intact(dq_buf, B * S, SENT_BF)


# --------------------------------------------------------------------------------------------------------------------------
# 2. causal bf16 attention (text tower)
# --------------------------------------------------------------------------------------------------------------------------
CAUSAL_BAR = 8e-3          # the cap; worst seen 3.4e-3


@pytest.mark.parametrize("H", [2, 8, 12])
@pytest.mark.parametrize("S,active", [(77, 0), (2, 0), (31, 0), (32, 0), (33, 0), (64, 0), (96, 0), (77, 33), (77, 9)])
def test_causal_attention_bf16_rows(S, active, H):
    l = lib()
    B, W, A = 3, 64 * H, active or S
    g = torch.Generator(device="cuda").manual_seed(100 * S + H + active)
    qkv = torch.randn(B * S, 3 * W, generator=g, device=dev())
    qkv[:, :W] *= 2.0                                   # logits with a spread of a few units
    qkv = qkv.bfloat16()
    o_buf, o = guarded(B * S, W, torch.bfloat16, SENT_BF)
    L.check(l.rvlm_k_attn_causal_fwd_bf16(qkv.data_ptr(), o.data_ptr(), B, H, S, active, st()))
    torch.cuda.synchronize()
    q, k, v = qkv.double().reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=dev()).triu(1), float("-inf"))
    ref = torch.softmax(s, -1) @ v
    got = bhsd(o, B, H, S)
    w = assert_rows(f"causal o S{S} H{H} active{active}", got[:, :, :A], ref[:, :, :A], CAUSAL_BAR, dims=("prompt", "h", "row"))
    assert bool((got[:, :, A:] == SENT_BF).all()), "rows >= active_len written"
    assert guards_intact(o_buf, B * S, SENT_BF)
    record("causal_attention_bf16_rows", S=S, H=H, active=active, o=w)


# --------------------------------------------------------------------------------------------------------------------------
# 3. LayerNorm (bf16 engine forms)
# --------------------------------------------------------------------------------------------------------------------------
LN_ROW8, LN_GENERIC = 1, 0          # include/rvlm_kernels.h RVLM_LN_FORM_*
LN_FAMILIES = ["randn", "mean50", "clip_like", "lowvar"]


def ln_inputs(M, W, family, seed):
    """x [M, W], gamma, beta.  mean50: rows with mean 50 and unit variance (a one-pass variance E[x^2] - E[x]^2 loses every digit);
    lowvar: rows with a standard deviation of 0.01 (variance 1e-4: the eps of 1e-5 is a tenth of it);
    clip_like: the statistics oracle/vit_ref.py make_clip_like documents - four channels 30-100x the ordinary ones, gains log-uniform
    over [1e-2, 3] with the outlier channels' gains at the low end."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, W, generator=g, device=dev())
    gm = 1 + 0.1 * torch.randn(W, generator=g, device=dev())
    bt = 0.1 * torch.randn(W, generator=g, device=dev())
    if family == "mean50":
        x = x + 50.0
    elif family == "lowvar":
        x = 0.01 * x + 0.3
    elif family == "clip_like":
        gm = torch.exp(torch.rand(W, generator=g, device=dev()) * (math.log(3.0) - math.log(1e-2)) + math.log(1e-2))
        ch = torch.randperm(W, generator=g, device=dev())[:4]
        scale = torch.exp(torch.rand(4, generator=g, device=dev()) * (math.log(100.0) - math.log(30.0)) + math.log(30.0))
        sign = torch.where(torch.rand(4, generator=g, device=dev()) < 0.5, -1.0, 1.0)
        x[:, ch] = 0.05 * x[:, ch] + scale * sign
        gm[ch] = torch.exp(torch.rand(4, generator=g, device=dev()) * (math.log(5e-2) - math.log(1e-2)) + math.log(1e-2))
    return x.contiguous(), gm.contiguous(), bt.contiguous()


def ln_reference(x, gm, bt):
    xd = x.double()
    mu = xd.mean(1)
    rs = (xd.var(1, unbiased=False) + 1e-5).rsqrt()
    return (xd - mu[:, None]) * rs[:, None] * gm.double() + bt.double(), mu, rs


def ln_out_tol(ref, mu, rs, gm, rel):
    """Per-element bound of a LayerNorm output against its fp64 value: `rel` of the value (2^-8: one bf16 rounding), 1e-6 absolute,
    and what a few fp32 ulps of the row mean (8 x 2^-24 |mean|: the mean itself is an fp32 number in the kernel) become behind
    (x - mean) * rstd * gamma - the term that matters for rows with |mean| >> std."""
    return rel * ref.abs() + 1e-6 + 2.0 ** -21 * (mu.abs() * rs)[:, None] * gm.double().abs()


def check_ln_stats(tag, mean, rstd, mu, rs):
    # mean: 1e-6 of the row's scale (|mean| + std: a row whose mean happens to vanish is not held to 1e-6 of nothing); rstd 1e-5
    e_mu = float(((mean.double() - mu).abs() / (mu.abs() + 1 / rs)).max())
    e_rs = float(((rstd.double() - rs).abs() / rs).max())
    assert e_mu <= 1e-6 and e_rs <= 1e-5, (tag, e_mu, e_rs)
    return e_mu, e_rs


@pytest.mark.parametrize("family", LN_FAMILIES)
@pytest.mark.parametrize("W,form", [(512, LN_ROW8), (1024, LN_ROW8), (1536, LN_ROW8), (2048, LN_ROW8), (64, LN_GENERIC), (128, LN_GENERIC),
                                    (384, LN_GENERIC), (768, LN_GENERIC), (1280, LN_GENERIC)])
def test_layernorm_fwd_bf16_rows(W, form, family):
    l = lib()
    assert l.rvlm_k_layernorm_form(W) == form, f"W = {W}: the dispatcher takes form {l.rvlm_k_layernorm_form(W)}, this case is written for {form}"
    worst = 0.0
    for M in (1, 5, 257, 1029):           # 4 rows per workgroup: every remainder
        x, gm, bt = ln_inputs(M, W, family, 7 * W + M)
        y_buf, y = guarded(M, W, torch.bfloat16, SENT_BF)
        st_buf, stats = guarded(2, M, torch.float32, SENT_F)
        L.check(l.rvlm_k_layernorm_fwd_bf16(x.data_ptr(), gm.data_ptr(), bt.data_ptr(), y.data_ptr(), stats[0].data_ptr(),
                                            stats[1].data_ptr(), M, W, st()))
        torch.cuda.synchronize()
        ref, mu, rs = ln_reference(x, gm, bt)
        excess = ((y.double() - ref).abs() / ln_out_tol(ref, mu, rs, gm, 2.0 ** -8)).max(dim=1)
        row = int(excess.values.argmax())
        assert float(excess.values[row]) <= 1.0, (f"W {W} M {M} {family}: row {row} col {int(excess.indices[row])}: {float(y[row, excess.indices[row]])} "
                                                  f"vs {float(ref[row, excess.indices[row]])} ({float(excess.values[row]):.2f} x the bound)")
        worst = max(worst, float(excess.values[row]))
        e_mu, e_rs = check_ln_stats((W, M, family), stats[0], stats[1], mu, rs)
        assert guards_intact(y_buf, M, SENT_BF) and guards_intact(st_buf, 2, SENT_F)
        record("layernorm_fwd_bf16_rows", W=W, M=M, form=form, family=LN_FAMILIES.index(family), y_over_bound=float(excess.values[row]),
               mean=e_mu, rstd=e_rs)


@pytest.mark.parametrize("family", LN_FAMILIES)
@pytest.mark.parametrize("W", [512, 1024, 1536, 2048])
def test_layernorm_bwd_bf16_rows(W, family):
    """layernorm_bwd8<NV, LPONLY>: both forms of the residual-gradient stream at every row-register width, accumulate 0 / 1 / -S."""
    l = lib()
    assert l.rvlm_k_layernorm_form(W) == LN_ROW8
    M, S = 4 * 37 + 3, 5
    x, gm, _ = ln_inputs(M, W, family, 11 * W)
    g = torch.Generator(device="cuda").manual_seed(W + 1)
    dy = torch.randn(M, W, generator=g, device=dev()).bfloat16()
    acc0 = torch.randn(M, W, generator=g, device=dev()).bfloat16()
    _, mu64, rs64 = ln_reference(x, gm, torch.zeros_like(gm))
    mean, rstd = mu64.float().contiguous(), rs64.float().contiguous()
    # the reference evaluates the kernel's formula in fp64 on the statistics the kernel is handed (rounded to fp32)
    gd = dy.double() * gm.double()
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gx = rstd.double()[:, None] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    rows = torch.arange(M, device=dev())
    for accumulate in (0, 1, -S):
        keep = (rows >= 0) if accumulate == 1 else (rows % S == 0) if accumulate < 0 else (rows < 0)
        want = gx + acc0.double() * keep[:, None]
        dr_buf, dres = guarded(M, W, torch.float32, SENT_F)
        dres.copy_(acc0.float())
        lp_buf, lp = guarded(M, W, torch.bfloat16, SENT_BF)
        L.check(l.rvlm_k_layernorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), gm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dres.data_ptr(),
                                            lp.data_ptr(), accumulate, M, W, st()))
        lp2_buf, lp2 = guarded(M, W, torch.bfloat16, SENT_BF)
        lp2.copy_(acc0)
        L.check(l.rvlm_k_layernorm_bwd_bf16(dy.data_ptr(), x.data_ptr(), gm.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
                                            lp2.data_ptr(), accumulate, M, W, st()))
        torch.cuda.synchronize()
        tag = f"W {W} {family} accumulate {accumulate}"
        w32 = assert_rows(f"dres {tag}", dres, want, 2e-7, dims=("row",))          # cap 2e-6; worst seen 7e-8
        assert torch.equal(lp, dres.bfloat16()), tag
        wlp = assert_rows(f"dres_lp alone {tag}", lp2, want, 2.0 ** -8, dims=("row",))
        assert torch.equal(lp2, lp), tag          # same fp32 arithmetic on the same bf16-representable accumulator
        assert guards_intact(dr_buf, M, SENT_F) and guards_intact(lp_buf, M, SENT_BF) and guards_intact(lp2_buf, M, SENT_BF)
        record("layernorm_bwd_bf16_rows", W=W, family=LN_FAMILIES.index(family), accumulate=accumulate, form=LN_ROW8, dres=w32, dres_lp=wlp)


# --------------------------------------------------------------------------------------------------------------------------
# 4. split-bf16 ("x3") operand kernels
# --------------------------------------------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, 1e-40, -3e-39, 1.1754944e-38, 1e30, -1e30, 1.0, -1.00390625, 3.3895314e38 / 4]


def split_emulation(a):
    """hi = bf16(a), lo = bf16(a - hi): round-to-nearest-even, evaluated on the host (IEEE arithmetic, denormals kept)."""
    a = a.detach().cpu().float()
    hi = a.bfloat16()
    lo = (a - hi.float()).bfloat16()
    return hi.to(dev()), lo.to(dev())


def with_specials(a):
    sp = torch.tensor(SPECIALS, device=a.device)
    a[0, : sp.numel()] = sp
    a[-1, -sp.numel():] = sp
    return a


def assert_split3(tag, A3, M, rows_out, K, hi, lo, order="hhl"):
    """A3 [rows_out, 3K] (int16 view): the three K-wide column blocks of rows < M bit for bit, rows M .. rows_out - 1 exactly zero."""
    want = {"h": bits(hi), "l": bits(lo)}
    for i, kind in enumerate(order):
        blk = A3[:M, i * K:(i + 1) * K]
        same = blk == want[kind]
        if not bool(same.all()):
            r, c = (int(v[0]) for v in torch.where(~same))
            raise AssertionError(f"{tag}: block {i} ({kind}) row {r} col {c}: bits {int(blk[r, c]) & 0xffff:#06x}, emulation "
                                 f"{int(want[kind][r, c]) & 0xffff:#06x}")
    assert bool((A3[M:rows_out] == 0).all()), f"{tag}: rows {M}..{rows_out - 1} are not zero"


@pytest.mark.parametrize("K", [264, 1024])
@pytest.mark.parametrize("M", [256, 257, 511])
def test_x3_split_rows_bits(M, K):
    l = lib()
    rows_out, lda = round_up(M, 256), K + 4
    g = torch.Generator(device="cuda").manual_seed(M + K)
    Abuf = torch.randn(M, lda, generator=g, device=dev()) * torch.exp(4 * torch.randn(M, 1, generator=g, device=dev()))
    A = with_specials(Abuf[:, :K])
    buf, A3 = guarded_nan(rows_out, 3 * K)
    L.check(l.rvlm_k_x3_split_rows(Abuf.data_ptr(), lda, A3.data_ptr(), M, rows_out, K, st()))
    torch.cuda.synchronize()
    hi, lo = split_emulation(A)
    assert_split3(f"split_rows M {M} K {K}", A3, M, rows_out, K, hi, lo)
    assert nan_guards_intact(buf, rows_out)
    normal = A.abs() > 1e-30                             # (lo of a smaller value underflows bf16's range)
    resid = ((A.double() - hi.double() - lo.double()).abs() / A.double().abs().clamp_min(1e-300))[normal]
    assert float(resid.max()) <= 2.0 ** -17
    record("x3_split_rows", M=M, K=K, resid_rel=float(resid.max()))


@pytest.mark.parametrize("rows,cols", [(256, 256), (100, 72), (33, 1000)])
def test_x3_prepare_weight_bits(rows, cols):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(rows + cols)
    w = with_specials(torch.randn(rows, cols, generator=g, device=dev()) * 0.05)
    nbuf, nk3 = guarded_nan(rows, 3 * cols)
    tbuf, t3 = guarded_nan(cols, 3 * rows)
    L.check(l.rvlm_k_x3_prepare_weight(w.data_ptr(), rows, cols, nk3.data_ptr(), t3.data_ptr(), st()))
    torch.cuda.synchronize()
    hi, lo = split_emulation(w)
    assert_split3(f"nk3 {rows}x{cols}", nk3, rows, rows, cols, hi, lo, order="hlh")
    assert_split3(f"t3 {rows}x{cols}", t3, cols, cols, rows, hi.t(), lo.t(), order="hlh")
    assert nan_guards_intact(nbuf, rows) and nan_guards_intact(tbuf, cols)


def split_value(A3, M, N):
    """(hi + lo in fp64, hi block == second hi block) of a [hi | hi | lo] buffer (int16 view)."""
    f = A3[:M].view(torch.bfloat16).double()
    return f[:, :N] + f[:, 2 * N:], bool((A3[:M, :N] == A3[:M, N:2 * N]).all())


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("mode,split,dact", [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1)])
def test_x3_act_forms(mode, split, dact, act):
    """x3_act_kernel<MODE, SPLIT, DACT>: act(h) or out * act'(h), to fp32 or straight into the split copy, with or without the bf16
    act'(h) of the handoff.  The activation is evaluated in fp32, so the split copy is held to |value - hi - lo| <= 2^-17 |value|
    plus the fp32 evaluation's own error (2e-6 of the value, 5e-7 max(1, |h|) absolute: GELU's 1 + erf cancels for h << 0)."""
    l = lib()
    N = 264
    for M in (256, 257, 511):
        rows_out = round_up(M, 256)
        g = torch.Generator(device="cuda").manual_seed(M + 10 * mode + act)
        h = torch.randn(M, N, generator=g, device=dev()) * 3
        h.view(-1)[:6] = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-30, -8.0], device=dev())
        up = torch.randn(M, N, generator=g, device=dev())
        ref = act_ref(h.double(), act) if mode == 0 else up.double() * dact_ref(h.double(), act)
        tol = (2.0 ** -17 if split else 0.0) * ref.abs() + 2e-6 * ref.abs() + 5e-7 * h.double().abs().clamp_min(1.0) * (1.0 if mode == 0 else up.double().abs().clamp_min(1e-3))
        obuf, out = guarded(M, N, torch.float32, SENT_F)
        if mode == 1:
            out.copy_(up)
        buf, A3 = guarded_nan(rows_out, 3 * N)
        dbuf, dbf = guarded(M, N, torch.bfloat16, SENT_BF)
        L.check(l.rvlm_k_x3_act(h.data_ptr(), N, out.data_ptr(), N, A3.data_ptr() if split else None, M, rows_out, N, act, mode,
                                dbf.data_ptr() if dact else None, N, st()))
        torch.cuda.synchronize()
        tag = f"x3_act mode {mode} split {split} dact {dact} act {act} M {M}"
        if split:
            got, twin = split_value(A3, M, N)
            assert twin, f"{tag}: the two hi blocks differ"
            assert bool((A3[M:rows_out] == 0).all()), f"{tag}: pad rows not zero"
            assert torch.equal(out, up) if mode == 1 else bool((out == SENT_F).all()), f"{tag}: the fp32 buffer was written"
        else:
            got = out.double()
            assert bool((A3 == NAN_BITS).all())
        over = float(((got - ref).abs() / tol).max())
        assert over <= 1.0, f"{tag}: {over:.2f} x the bound"
        if dact:
            dref = dact_ref(h.double(), act)
            dover = float(((dbf.double() - dref).abs() / (2.0 ** -8 * dref.abs() + 1e-6)).max())
            assert dover <= 1.0, f"{tag}: act'(h) {dover:.2f} x the bound"
        else:
            assert bool((dbf == SENT_BF).all())
        assert nan_guards_intact(buf, rows_out) and guards_intact(obuf, M, SENT_F) and guards_intact(dbuf, M, SENT_BF)
        record("x3_act", mode=mode, split=split, dact=dact, act=act, M=M, over_bound=over)


@pytest.mark.parametrize("dact", [0, 1])
def test_x3_export_bf16(dact):
    l = lib()
    N, ldo, act = 264, 272, 0
    for M in (256, 257, 511):
        g = torch.Generator(device="cuda").manual_seed(M + dact)
        A = torch.randn(M, N, generator=g, device=dev()) * 3
        if not dact:
            A = with_specials(A * torch.exp(4 * torch.randn(M, 1, generator=g, device=dev())))
        buf, out = guarded_nan(M, ldo)
        L.check(l.rvlm_k_x3_export_bf16(A.data_ptr(), N, out.data_ptr(), ldo, M, N, act, dact, st()))
        torch.cuda.synchronize()
        if dact:
            ref = dact_ref(A.double(), act)
            over = float(((out[:, :N].view(torch.bfloat16).double() - ref).abs() / (2.0 ** -8 * ref.abs() + 1e-6)).max())
            assert over <= 1.0, over
        else:
            assert torch.equal(out[:, :N], bits(A.cpu().bfloat16().to(dev()))), "export differs from the round-to-nearest-even cast"
        assert bool((out[:, N:] == NAN_BITS).all()) and nan_guards_intact(buf, M)


@pytest.mark.parametrize("family", LN_FAMILIES)
@pytest.mark.parametrize("W", [512, 1024, 1536, 2048])
def test_x3_layernorm_fwd_rows(W, family):
    l = lib()
    for M in (256, 257, 511):
        rows_out = round_up(M, 256)
        x, gm, bt = ln_inputs(M, W, family, 13 * W + M)
        buf, A3 = guarded_nan(rows_out, 3 * W)
        st_buf, stats = guarded(2, M, torch.float32, SENT_F)
        L.check(l.rvlm_k_x3_layernorm_fwd(x.data_ptr(), gm.data_ptr(), bt.data_ptr(), A3.data_ptr(), stats[0].data_ptr(),
                                          stats[1].data_ptr(), M, rows_out, W, st()))
        torch.cuda.synchronize()
        ref, mu, rs = ln_reference(x, gm, bt)
        got, twin = split_value(A3, M, W)
        assert twin and bool((A3[M:rows_out] == 0).all())
        # 2^-17 of the value for the dropped bits of the split, 2e-6 for the fp32 evaluation
        over = float(((got - ref).abs() / ln_out_tol(ref, mu, rs, gm, 2.0 ** -17 + 2e-6)).max())
        assert over <= 1.0, f"x3 layernorm W {W} M {M} {family}: {over:.2f} x the bound"
        e_mu, e_rs = check_ln_stats((W, M, family), stats[0], stats[1], mu, rs)
        assert nan_guards_intact(buf, rows_out) and guards_intact(st_buf, 2, SENT_F)
        record("x3_layernorm_fwd", W=W, M=M, family=LN_FAMILIES.index(family), over_bound=over, mean=e_mu, rstd=e_rs)


def test_x3_layernorm_fwd_uncovered_width_launches_nothing():
    l = lib()
    M, W = 256, 768
    x, gm, bt = ln_inputs(M, W, "randn", 1)
    buf, A3 = guarded_nan(M, 3 * W)
    rc = l.rvlm_k_x3_layernorm_fwd(x.data_ptr(), gm.data_ptr(), bt.data_ptr(), A3.data_ptr(), None, None, M, M, W, st())
    torch.cuda.synchronize()
    assert rc == L.RVLM_ERR_UNSUPPORTED and bool((buf == NAN_BITS).all())


# --------------------------------------------------------------------------------------------------------------------------
# 5. class-token tail, embedding, im2col / col2im, l2norm
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [17, 50, 197, 257])
def test_attn_cls_rows(S, B):
    """Class-token attention of the last block: only token 0's query row is live; dqkv is written in full (dQ of the others zero)."""
    l = lib()
    H = 3
    W = H * 64
    qkv, d_o_all = attn_inputs(B, H, S, "peaked" if S == 257 else "randn", S + B)
    d_o = d_o_all.reshape(B, S, W)[:, 0].contiguous()
    o_buf, o = guarded(B, W, torch.bfloat16, SENT_BF)
    l_buf, lse = guarded(1, B * H, torch.float32, SENT_F)
    dq_buf, dqkv = guarded(B * S, 3 * W, torch.bfloat16, SENT_BF)
    L.check(l.rvlm_k_attn_cls_fwd_bf16(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, S, st()))
    L.check(l.rvlm_k_attn_cls_bwd_bf16(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), B, H, S, st()))
    torch.cuda.synchronize()
    x = qkv.double().requires_grad_(True)
    q, k, v = x.reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q[:, :, :1] @ k.transpose(-1, -2)) * 0.125                   # [B, H, 1, S]
    o_ref = torch.softmax(s, -1) @ v                                   # [B, H, 1, 64]
    (gx,) = torch.autograd.grad((o_ref[:, :, 0] * d_o.double().reshape(B, H, 64)).sum(), x)
    worst = {"o": assert_rows(f"cls o S{S} B{B}", o.reshape(B, H, 1, 64), o_ref.detach(), CLS_BARS["o"])}
    worst["lse"] = float((lse.reshape(B, H).double() - torch.logsumexp(s.detach(), -1)[:, :, 0]).abs().max())
    assert worst["lse"] <= CLS_BARS["lse"], worst["lse"]
    # backward: the flash formula in fp64 on the kernel's own o and lse (see attn_backward_reference), and autograd for the flat case
    qd, kd, vd = (t.detach() for t in (q, k, v))
    dod = d_o.double().reshape(B, H, 64)
    p = torch.exp((kd @ qd[:, :, 0, :, None])[..., 0] * 0.125 - lse.reshape(B, H, 1).double())            # [B, H, S]
    ds = p * ((vd @ dod[..., None])[..., 0] - (dod * o.double().reshape(B, H, 64)).sum(-1, keepdim=True)) * 0.125
    dq_f = torch.zeros_like(qd)
    dq_f[:, :, 0] = (ds[..., None] * kd).sum(2)
    flash_ref = (dq_f, ds[..., None] * qd[:, :, :1], p[..., None] * dod[:, :, None])
    for i, name in enumerate(("dq", "dk", "dv")):
        got = bhsd(dqkv[:, i * W:(i + 1) * W], B, H, S)
        worst[name] = assert_rows(f"cls {name} S{S} B{B}", got, flash_ref[i], CLS_BARS[name])
        # ... and the formula is the gradient.  dV = p dO row by row; with ONE query a dK row is a single dS_j q, so where dP_j happens to
        # meet D the bf16 rounding of o shows in that row alone: dQ / dK are tied to autograd over each (image, head) instead
        auto = bhsd(gx[:, i * W:(i + 1) * W], B, H, S)
        if name == "dv":
            assert_rows(f"cls dv vs autograd S{S} B{B}", got, auto, CLS_BARS["dv"])
        elif S != 257:                  # (the peaked case: dP - D cancels for the query itself, as in test_attention_bf16_rows)
            assert_rows(f"cls {name} vs autograd S{S} B{B}", got.reshape(B, H, 1, S * 64), auto.reshape(B, H, 1, S * 64), ATTN_BARS[name])
    assert bool((dqkv.reshape(B, S, 3 * W)[:, 1:, :W] == 0).all()), "dQ rows of the other tokens are not zero"
    assert guards_intact(o_buf, B, SENT_BF) and guards_intact(l_buf, 1, SENT_F) and guards_intact(dq_buf, B * S, SENT_BF)
    record("attn_cls_rows", S=S, B=B, **worst)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S,W", [(17, 192), (50, 768), (197, 384), (257, 1024)])
def test_embed_lnpre_rows(S, W, B):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(S + W + B)
    patch = torch.randn(B * (S - 1), W, generator=g, device=dev())
    cls = torch.randn(W, generator=g, device=dev())
    pos = 0.5 * torch.randn(S, W, generator=g, device=dev())
    gm = 1 + 0.1 * torch.randn(W, generator=g, device=dev())
    bt = 0.1 * torch.randn(W, generator=g, device=dev())
    dx0 = torch.randn(B * S, W, generator=g, device=dev())
    x_buf, x0 = guarded(B * S, W, torch.float32, SENT_F)
    t_buf, tok = guarded(B * S, W, torch.float32, SENT_F)
    st_buf, stats = guarded(2, B * S, torch.float32, SENT_F)
    L.check(l.rvlm_k_embed_lnpre_fwd(patch.data_ptr(), cls.data_ptr(), pos.data_ptr(), gm.data_ptr(), bt.data_ptr(), x0.data_ptr(),
                                     stats[0].data_ptr(), stats[1].data_ptr(), tok.data_ptr(), B, S, W, st()))
    torch.cuda.synchronize()
    tokens = (torch.cat([cls.expand(B, 1, W), patch.reshape(B, S - 1, W)], 1) + pos).reshape(B * S, W)     # one fp32 addition: exact reference
    assert torch.equal(tok, tokens)
    ref, mu, rs = ln_reference(tokens, gm, bt)
    w_x0 = assert_rows(f"x0 S{S} W{W} B{B}", x0, ref, 3.5e-7, dims=("row",))          # cap 2e-6; worst seen 1.2e-7
    check_ln_stats((S, W, B), stats[0], stats[1], mu, rs)
    assert guards_intact(x_buf, B * S, SENT_F) and guards_intact(t_buf, B * S, SENT_F) and guards_intact(st_buf, 2, SENT_F)
    # backward of the patch rows, on the statistics the forward wrote
    mean, rstd = stats[0].contiguous(), stats[1].contiguous()
    gd = dx0.double() * gm.double()
    xh = (tokens.double() - mean.double()[:, None]) * rstd.double()[:, None]
    gx = rstd.double()[:, None] * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    want = gx.reshape(B, S, W)[:, 1:].reshape(B * (S - 1), W)
    for bf, dtype, fill, bar in ((0, torch.float32, SENT_F, 2e-7), (1, torch.bfloat16, SENT_BF, 2.0 ** -8)):      # seen 6.5e-8 / 2.2e-3
        d_buf, dp = guarded(B * (S - 1), W, dtype, fill)
        L.check(l.rvlm_k_embed_lnpre_bwd(dx0.data_ptr(), patch.data_ptr(), pos.data_ptr(), gm.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                         dp.data_ptr(), bf, B, S, W, st()))
        torch.cuda.synchronize()
        w = assert_rows(f"d_patch bf16={bf} S{S} W{W} B{B}", dp, want, bar, dims=("row",))
        assert guards_intact(d_buf, B * (S - 1), fill)
        record("embed_lnpre_rows", S=S, W=W, B=B, bf16=bf, x0=w_x0, d_patch=w)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("P,grid", [(8, 4), (14, 16), (16, 14), (32, 7)])        # S = 17, 257, 197, 50; Kpad - 3 P^2 = 0, 52, 0, 0
def test_im2col_col2im(P, grid, B):
    l = lib()
    img, Kp = P * grid, 3 * P * P
    Kpad, rows = round_up(Kp, 64), B * grid * grid
    lda = Kpad + 8
    g = torch.Generator(device="cuda").manual_seed(P + B)
    x = torch.rand(B, 3, img, img, generator=g, device=dev())
    delta = (torch.rand(B, 3, img, img, generator=g, device=dev()) * 2 - 1) * (4 / 255)
    mean3 = (C.c_float * 3)(0.48145466, 0.4578275, 0.40821073)
    std3 = (C.c_float * 3)(0.26862954, 0.26130258, 0.27577711)
    m = torch.tensor(list(mean3), dtype=torch.float64, device=dev())[None, :, None, None]
    s = torch.tensor(list(std3), dtype=torch.float64, device=dev())[None, :, None, None]

    def patches(t):      # [B, 3, img, img] -> [rows, 3 P^2] in the column order c*P*P + i*P + j
        return t.reshape(B, 3, grid, P, grid, P).permute(0, 2, 4, 1, 3, 5).reshape(rows, Kp)
    for d in (None, delta):
        pix = x if d is None else x + d                      # the kernel's one fp32 addition
        ref = patches((pix.double() - m) / s)
        for bf, dtype, fill, rel in ((0, torch.float32, SENT_F, 2.0 ** -22), (1, torch.bfloat16, SENT_BF, 2.0 ** -8)):
            buf, A0 = guarded(rows, lda, dtype, fill)
            L.check(l.rvlm_k_im2col_normalize(x.data_ptr(), L.ptr(d), B, img, P, mean3, std3, A0.data_ptr(), lda, Kpad, bf, st()))
            torch.cuda.synchronize()
            over = float(((A0[:, :Kp].double() - ref).abs() / (rel * ref.abs() + 1e-6)).max())
            assert over <= 1.0, (P, B, bf, over)
            assert bool((A0[:, Kp:Kpad] == 0).all()), "pad columns are not zero"
            assert bool((A0[:, Kpad:] == fill).all()) and guards_intact(buf, rows, fill)
    # col2im: grad_x = dA0[row, col] / std_c, one fp32 division
    for bf, dtype in ((0, torch.float32), (1, torch.bfloat16)):
        dA = torch.randn(rows, lda, generator=g, device=dev()).to(dtype)
        gbuf, gx = guarded(B * 3 * img, img, torch.float32, SENT_F)
        L.check(l.rvlm_k_col2im_grad(dA.data_ptr(), lda, bf, B, img, P, std3, gx.data_ptr(), st()))
        torch.cuda.synchronize()
        want = dA[:, :Kp].double().reshape(B, grid, grid, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, img, img) / s
        assert float(((gx.reshape(B, 3, img, img).double() - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 2.0 ** -23
        assert guards_intact(gbuf, B * 3 * img, SENT_F)


@pytest.mark.parametrize("B,D", [(1, 48), (3, 512), (5, 768), (130, 100)])
def test_l2norm_rows(B, D):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(B + D)
    e = torch.randn(B, D, generator=g, device=dev()) * torch.exp(3 * torch.randn(B, 1, generator=g, device=dev()))
    d_out = torch.randn(B, D, generator=g, device=dev())
    o_buf, out = guarded(B, D, torch.float32, SENT_F)
    i_buf, inv = guarded(1, B, torch.float32, SENT_F)
    d_buf, d_raw = guarded(B, D, torch.float32, SENT_F)
    L.check(l.rvlm_l2_normalize_rows(e.data_ptr(), B, D, out.data_ptr(), inv.data_ptr(), st()))
    L.check(l.rvlm_k_l2_normalize_bwd(d_out.data_ptr(), e.data_ptr(), inv.data_ptr(), d_raw.data_ptr(), B, D, st()))
    torch.cuda.synchronize()
    ed = e.double().requires_grad_(True)
    ref = torch.nn.functional.normalize(ed, dim=1)
    (gref,) = torch.autograd.grad((ref * d_out.double()).sum(), ed)
    w_f = assert_rows(f"l2norm fwd B{B} D{D}", out, ref.detach(), 2.7e-7, dims=("row",))          # worst seen 9e-8
    assert float(((inv[0].double() - 1 / e.double().norm(dim=1)).abs() * e.double().norm(dim=1)).max()) <= 1e-6
    w_b = assert_rows(f"l2norm bwd B{B} D{D}", d_raw, gref, 3.2e-7, dims=("row",))          # worst seen 1.1e-7
    assert guards_intact(o_buf, B, SENT_F) and guards_intact(i_buf, 1, SENT_F) and guards_intact(d_buf, B, SENT_F)
    record("l2norm_rows", B=B, D=D, fwd=w_f, bwd=w_b)
