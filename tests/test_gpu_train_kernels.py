"""Per-element fp64 parity of the training step's kernels (csrc/train_kernels.hip, through include/rvlm_kernels.h) at every
reduction regime.

The column reductions behind every bias and LayerNorm-affine gradient pick their launch shape from the row count (1, 16 or 128 row
chunks, rvlm_k_reduce_chunks) and, for bf16 rows, from the operand's width and alignment (rvlm_k_colsum_form).  A chunk that drops its
last row, a 64-column block left unwritten or an ignored `accumulate` moves a whole-tensor cosine in the fifth digit, so every output
ELEMENT here is held to its own bar (tests/gpu_helpers.py elem_rel) against an fp64 torch evaluation on the device of the values the
kernel reads (bf16 inputs: the rounded values).  The scale of a column sum is the L2 norm of its terms (sqrt(R) x their RMS): a sum
that nearly cancels is judged on that absolute scale.  Operands sit inside larger NaN-filled buffers (a read outside the operand
poisons the result), leading dimensions exceed the widths, outputs and the reduce scratch carry guard regions that must stay
untouched, and a test asserts the chunk count and the kernel form it was written for instead of assuming them."""
import pytest
import torch

from robustvlm_amd import _lib as L
from tests.gpu_helpers import dev, st, lib, record, assert_elems

pytestmark = pytest.mark.gpu

GUARD = 64                  # guard elements in front of and behind every output, and behind the reduce scratch
SENT = -12345.0             # sentinel (exact in fp32 and bf16)
FORM_GENERIC, FORM_16B = 0, 1      # include/rvlm_kernels.h RVLM_COLSUM_FORM_*
NAN = float("nan")

# (rows, row chunks the dispatchers must choose).  4 112 = 16 x 257: 33-row chunks, the last one short and three empty; 32 896 =
# 128 x 257: the rows of a training step at B = 128 (bench.py --mode train)
ROWS = [(1, 1), (3, 1), (255, 1), (256, 16), (257, 16), (4095, 16), (4096, 128), (4097, 128), (4112, 128), (32896, 128)]
# 100: a partial 64-column block and a partial 16-column reduce block; the multiples of 256 take the 16-byte bf16 form when aligned
COLS = [64, 100, 768, 1024, 3072, 4096]
DTYPES = [torch.float32, torch.bfloat16]

# Bars: the worst value of the first run of each comparison on an MI355X (in the comment), times a margin of 3 to 4.
BAR_COLSUM = 3e-6           # measured 9.0e-7 (fp32 rows; bf16 rows 4.7e-7, accumulate 5.9e-7, the odd partial-row counts 3.0e-7)
BAR_LN = 3e-6               # measured 8.4e-7 (dgamma, bf16 dy; dbeta 7.6e-7, accumulate 6.9e-7, the tail's shape 5.3e-7)
BAR_POS = 4e-6              # measured 1.1e-6 (accumulate 9.6e-7)
BAR_ADAMW = {"p": 1.2e-6, "m": 2e-7, "v": 7e-7}      # against fp64; measured 3.9e-7, 5.9e-8, 2.1e-7
BAR_ADAMW_TORCH = 1.2e-6    # against torch.optim.AdamW in fp32; measured 3.7e-7


def tname(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def in_nan(t, ld, off=0, tail_rows=8):
    """The 2-D tensor t as a kernel operand inside a NaN-filled buffer: rows `ld` elements apart, the base pointer `off` elements
    behind the allocation's (aligned) start, NaN in every pad column and in `tail_rows` rows behind the last.  Returns (buffer, view)."""
    R, C = t.shape
    buf = torch.full((off + (R + tail_rows) * ld,), NAN, dtype=t.dtype, device=dev())
    view = buf[off:off + R * ld].view(R, ld)[:, :C]
    view.copy_(t)
    assert buf.data_ptr() % 256 == 0
    return buf, view


def out_guarded(n, fill):
    """(buffer, the n-element output view a kernel is handed): GUARD sentinels on either side, the view itself set to `fill`."""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=dev())
    view = buf[GUARD:GUARD + n]
    if torch.is_tensor(fill):
        view.copy_(fill.flatten())
    else:
        view.fill_(fill)
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all())


def red_scratch(need):
    """Reduce scratch of exactly `need` floats (NaN: a partial the second pass reads but the first never wrote poisons the result)
    followed by GUARD sentinels."""
    buf = torch.full((need + GUARD,), SENT, dtype=torch.float32, device=dev())
    buf[:need] = NAN
    return buf


def red_guard_intact(buf, need):
    return bool((buf[need:] == SENT).all())


def last_row_of_a_chunk(R, nch, pick):
    """The last row of one non-empty row chunk (rows_per = ceil(R / nch), the partial kernels' own split)."""
    rows_per = (R + nch - 1) // nch
    nonempty = (R + rows_per - 1) // rows_per
    k = pick % nonempty
    return min(R, (k + 1) * rows_per) - 1


def rows_input(family, R, C, dtype, g, nch):
    """[R, C] values of the kernel's element type.
    randn: every row matters equally.  const: every column constant at a multiple of 1/8 (every partial sum is exact in fp32: the
    result must equal R x the constant bit for bit).  huge: one row of +-1000s - the last row of a chunk - among rows of 1e-3 (a
    dropped or doubled row is an O(1) error of its column, not 1 / R)."""
    if family == "randn":
        t = torch.randn(R, C, generator=g, device=dev())
    elif family == "const":
        t = ((torch.arange(C, device=dev()) % 16 - 8).float() / 8).expand(R, C).contiguous()
    else:
        t = 1e-3 * torch.randn(R, C, generator=g, device=dev())
        hr = last_row_of_a_chunk(R, nch, 5 * R + C)
        t[hr] = 1000.0 * (1 + torch.arange(C, device=dev()) % 3) * (1 - 2 * (torch.arange(C, device=dev()) % 2))
    return t.to(dtype)


def colsum_ref(t):
    """(fp64 column sums, the L2 norm of each column's terms) of the values the kernel reads."""
    return t.sum(0, dtype=torch.float64), torch.linalg.vector_norm(t, 2, dim=0, dtype=torch.float64)


def colsum_variants(dtype, C):
    """(ld, base offset in elements, the form this variant is written for)."""
    if dtype == torch.float32:
        return [(C, 0, FORM_GENERIC), (C + 8, 0, FORM_GENERIC), (C + 8, 2, FORM_GENERIC)]
    f16 = FORM_16B if C in (768, 1024, 3072, 4096) else FORM_GENERIC
    # ld = C + 4: every other row starts 8 bytes off a 16-byte boundary; base + 4 elements: every row does
    return [(C, 0, f16), (C + 8, 0, f16), (C + 4, 0, FORM_GENERIC), (C + 8, 4, FORM_GENERIC)]


def run_colsum(view, ld, R, C, out, accumulate, red, red_floats):
    return lib().rvlm_k_colsum(view.data_ptr(), int(view.dtype == torch.bfloat16), ld, R, C, out.data_ptr(), accumulate, red.data_ptr(),
                               red_floats, st())


# --------------------------------------------------------------------------------------------------------------------------
# 1. colsum<float | bf16> (bias gradients): generic and 16-byte forms, every chunk regime
# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("R,nch", ROWS)
def test_colsum_elements(R, nch, C, dtype):
    l = lib()
    assert l.rvlm_k_reduce_chunks(R) == nch, f"R = {R}: the dispatchers take {l.rvlm_k_reduce_chunks(R)} chunks, this case is written for {nch}"
    g = torch.Generator(device="cuda").manual_seed(R * 7919 + C)
    need = nch * C
    worst, worst_acc, forms = 0.0, 0.0, set()
    for family in ("randn", "const", "huge"):
        t = rows_input(family, R, C, dtype, g, nch)
        ref, floor = colsum_ref(t)
        variants = colsum_variants(dtype, C)
        for ld, off, form in (variants if family == "randn" else variants[1:2]):
            buf, view = in_nan(t, ld, off)
            got_form = l.rvlm_k_colsum_form(int(dtype == torch.bfloat16), C, ld, view.data_ptr() % 16)
            assert got_form == form, f"{tname(dtype)} C {C} ld {ld} base +{off}: colsum takes form {got_form}, this case is written for {form}"
            forms.add(form)
            red = red_scratch(need)
            obuf, out = out_guarded(C, NAN)                     # accumulate = 0 must not read the output
            L.check(run_colsum(view, ld, R, C, out, 0, red, need), "colsum")
            torch.cuda.synchronize()
            name = f"colsum {tname(dtype)} R {R} C {C} ld {ld} base +{off} {family}"
            assert guards_intact(obuf, C) and red_guard_intact(red, need), f"{name}: wrote outside its output or its scratch"
            if family == "const":
                assert torch.equal(out.double(), ref), f"{name}: a sum of exactly representable partials is not exact"
            else:
                worst = max(worst, assert_elems(name, out, ref, floor, BAR_COLSUM, dims=("col",)))
            if ld == C + 8 and off == 0 and family != "const":
                prior = torch.randn(C, generator=g, device=dev()) * float(R) ** 0.5
                obuf, out = out_guarded(C, prior)
                red = red_scratch(need)
                L.check(run_colsum(view, ld, R, C, out, 1, red, need), "colsum")
                torch.cuda.synchronize()
                assert guards_intact(obuf, C) and red_guard_intact(red, need), f"{name} accumulate: wrote outside its output or its scratch"
                worst_acc = max(worst_acc, assert_elems(name + " accumulate", out, ref + prior.double(), floor + prior.double().abs(),
                                                        BAR_COLSUM, dims=("col",)))
    if dtype == torch.bfloat16 and C % 256 == 0:
        assert forms == {FORM_GENERIC, FORM_16B}
    record("train_kernels_colsum", R=R, C=C, bf16=int(dtype == torch.bfloat16), worst=worst, worst_accumulate=worst_acc)


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("R,nch", [(3, 1), (257, 16), (4112, 128)])
def test_colsum_refuses_short_scratch(R, nch, dtype):
    """red_floats one short of reduce_chunks(R) x C: RVLM_ERR_STATE, nothing launched - output and scratch as they were."""
    C = 768
    t = torch.ones(R, C, device=dev()).to(dtype)
    need = nch * C
    red = torch.full((need + GUARD,), SENT, device=dev())
    obuf, out = out_guarded(C, SENT)
    rc = run_colsum(t, C, R, C, out, 0, red, need - 1)
    torch.cuda.synchronize()
    assert rc == L.RVLM_ERR_STATE, rc
    assert bool((obuf == SENT).all()) and bool((red == SENT).all())
    L.check(run_colsum(t, C, R, C, out, 0, red, need), "colsum")          # exactly enough is enough
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((C,), float(R), device=dev()))


# --------------------------------------------------------------------------------------------------------------------------
# 2. ln_param_grad<float | bf16> (LayerNorm affine gradients)
# --------------------------------------------------------------------------------------------------------------------------
def ln_x_input(family, R, C, g):
    """The LayerNorm's fp32 input.  offset: rows of large mean and small variance (mean 100 .. 700, deviation 0.01): x - mean cancels
    five digits, and a row read with another row's statistics is wrong by hundreds of deviations."""
    if family == "offset":
        return 100.0 * (1 + torch.arange(R, device=dev()) % 7).float()[:, None] + 0.01 * torch.randn(R, C, generator=g, device=dev())
    return torch.randn(R, C, generator=g, device=dev()) * 1.5 + 0.25 * torch.randn(R, 1, generator=g, device=dev())


def ln_stats(x):
    """(mean, rstd) of every row as the forward stores them: fp32 (evaluated in fp64, eps 1e-5)."""
    xd = x.double()
    mu = xd.mean(1)
    var = ((xd - mu[:, None]) ** 2).mean(1)
    return mu.float(), (var + 1e-5).rsqrt().float()


def ln_ref(dy, x, mean, rstd):
    """fp64 evaluation of the kernel's formula on what it reads: (dgamma, its terms' norm, dbeta, its terms' norm)."""
    terms = dy.double() * ((x.double() - mean.double()[:, None]) * rstd.double()[:, None])
    return terms.sum(0), terms.norm(dim=0), dy.sum(0, dtype=torch.float64), torch.linalg.vector_norm(dy, 2, dim=0, dtype=torch.float64)


def stats_nan(v, length):
    """A statistics vector at the front of a NaN-filled buffer of `length` floats (an index beyond the rows reads NaN)."""
    buf = torch.full((length,), NAN, device=dev())
    buf[:v.numel()] = v
    return buf


def run_ln(dyv, lddy, xv, ldx, mean, rstd, R, C, dg, db, accumulate, red, red_floats):
    return lib().rvlm_k_ln_param_grad(dyv.data_ptr(), int(dyv.dtype == torch.bfloat16), lddy, xv.data_ptr(), ldx, mean.data_ptr(),
                                      rstd.data_ptr(), R, C, dg.data_ptr(), db.data_ptr(), accumulate, red.data_ptr(), red_floats, st())


def check_ln(name, dyv, lddy, xv, ldx, mean, rstd, R, C, refs, g, accumulate_too):
    """One call with accumulate = 0 onto NaN outputs and (accumulate_too) one with accumulate = 1 onto two different known tensors;
    dgamma and dbeta are judged separately.  Returns (worst dgamma, worst dbeta, worst of the accumulate call)."""
    nch = lib().rvlm_k_reduce_chunks(R)
    need = 2 * nch * C
    rg, fg, rb, fb = refs
    red = red_scratch(need)
    gbuf, dg = out_guarded(C, NAN)
    bbuf, db = out_guarded(C, NAN)
    L.check(run_ln(dyv, lddy, xv, ldx, mean, rstd, R, C, dg, db, 0, red, need), "ln_param_grad")
    torch.cuda.synchronize()
    assert guards_intact(gbuf, C) and guards_intact(bbuf, C) and red_guard_intact(red, need), f"{name}: wrote outside its outputs or its scratch"
    wg = assert_elems(name + " dgamma", dg, rg, fg, BAR_LN, dims=("col",))
    wb = assert_elems(name + " dbeta", db, rb, fb, BAR_LN, dims=("col",))
    wa = 0.0
    if accumulate_too:
        pg = torch.randn(C, generator=g, device=dev()) * float(R) ** 0.5
        pb = torch.randn(C, generator=g, device=dev()) * float(R) ** 0.5 + 3.0
        gbuf, dg = out_guarded(C, pg)
        bbuf, db = out_guarded(C, pb)
        red = red_scratch(need)
        L.check(run_ln(dyv, lddy, xv, ldx, mean, rstd, R, C, dg, db, 1, red, need), "ln_param_grad")
        torch.cuda.synchronize()
        assert guards_intact(gbuf, C) and guards_intact(bbuf, C) and red_guard_intact(red, need), f"{name} accumulate: wrote outside"
        wa = max(assert_elems(name + " accumulate dgamma", dg, rg + pg.double(), fg + pg.double().abs(), BAR_LN, dims=("col",)),
                 assert_elems(name + " accumulate dbeta", db, rb + pb.double(), fb + pb.double().abs(), BAR_LN, dims=("col",)))
    return wg, wb, wa


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("R,nch", ROWS)
def test_ln_param_grad_elements(R, nch, C, dtype):
    l = lib()
    assert l.rvlm_k_reduce_chunks(R) == nch, f"R = {R}: the dispatchers take {l.rvlm_k_reduce_chunks(R)} chunks, this case is written for {nch}"
    g = torch.Generator(device="cuda").manual_seed(R * 104729 + C)
    variants = [(C, C), (C + 8, C + 8)] + ([(C + 4, C + 8)] if dtype == torch.bfloat16 else [])      # (lddy, ldx)
    worst = [0.0, 0.0, 0.0]
    for family in ("randn", "const", "huge", "offset"):
        dy = rows_input("randn" if family == "offset" else family, R, C, dtype, g, nch)
        x = ln_x_input(family, R, C, g)
        mean, rstd = ln_stats(x)
        refs = ln_ref(dy, x, mean, rstd)
        mbuf, rbuf = stats_nan(mean, R + GUARD), stats_nan(rstd, R + GUARD)
        for lddy, ldx in (variants if family == "randn" else variants[1:2]):
            _, dyv = in_nan(dy, lddy)
            _, xv = in_nan(x, ldx)
            name = f"ln_param_grad {tname(dtype)} R {R} C {C} lddy {lddy} ldx {ldx} {family}"
            w = check_ln(name, dyv, lddy, xv, ldx, mbuf, rbuf, R, C, refs, g, accumulate_too=(lddy == C + 8 and family != "const"))
            worst = [max(a, b) for a, b in zip(worst, w)]
            if family == "const":       # dbeta of constant columns: exact partial sums
                gbuf, dg = out_guarded(C, NAN)
                bbuf, db = out_guarded(C, NAN)
                red = red_scratch(2 * nch * C)
                L.check(run_ln(dyv, lddy, xv, ldx, mbuf, rbuf, R, C, dg, db, 0, red, 2 * nch * C), "ln_param_grad")
                torch.cuda.synchronize()
                assert torch.equal(db.double(), refs[2]), f"{name}: dbeta of constant columns is not exact"
    record("train_kernels_ln_param_grad", R=R, C=C, bf16=int(dtype == torch.bfloat16), worst_dgamma=worst[0], worst_dbeta=worst[1],
           worst_accumulate=worst[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("S,W", [(257, 1024), (50, 768)])
@pytest.mark.parametrize("B,nch", [(4, 1), (128, 1), (256, 16), (300, 16)])
def test_ln_param_grad_class_token_tail(B, nch, S, W, dtype):
    """The call of the class-token tail (ln_2 of the last block): R = B rows, x = the class rows of the [B * S, W] residual stream
    (ldx = S * W), dy [B, W] contiguous, mean / rstd COMPACT - the tail's forward LayerNorm over the same B strided rows stores the
    statistics of image b at index b, and the backward reads them there.  Every other row of x is NaN, and so is every statistic
    beyond B (in a buffer as long as the token rows: an index scaled by S stays inside it and reads NaN)."""
    l = lib()
    assert l.rvlm_k_reduce_chunks(B) == nch
    g = torch.Generator(device="cuda").manual_seed(B * 31 + W)
    worst = [0.0, 0.0, 0.0]
    for family in ("randn", "huge", "offset"):
        dy = rows_input("randn" if family == "offset" else family, B, W, dtype, g, nch)
        x = ln_x_input(family, B, W, g)
        mean, rstd = ln_stats(x)
        refs = ln_ref(dy, x, mean, rstd)
        xbuf = torch.full((B * S + 8, W), NAN, device=dev())
        xbuf[0:B * S:S] = x
        name = f"ln_param_grad tail {tname(dtype)} B {B} S {S} W {W} {family}"
        w = check_ln(name, in_nan(dy, W)[1], W, xbuf, S * W, stats_nan(mean, B * S), stats_nan(rstd, B * S), B, W, refs, g, accumulate_too=True)
        worst = [max(a, b) for a, b in zip(worst, w)]
    record("train_kernels_ln_param_grad_tail", B=B, S=S, W=W, bf16=int(dtype == torch.bfloat16), worst_dgamma=worst[0], worst_dbeta=worst[1],
           worst_accumulate=worst[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=tname)
@pytest.mark.parametrize("R,nch", [(3, 1), (257, 16), (4112, 128)])
def test_ln_param_grad_refuses_short_scratch(R, nch, dtype):
    C = 768
    dy = torch.ones(R, C, device=dev()).to(dtype)
    x = torch.randn(R, C, device=dev())
    mean, rstd = ln_stats(x)
    need = 2 * nch * C
    red = torch.full((need + GUARD,), SENT, device=dev())
    gbuf, dg = out_guarded(C, SENT)
    bbuf, db = out_guarded(C, SENT)
    rc = run_ln(dy, C, x, C, mean, rstd, R, C, dg, db, 0, red, need - 1)
    torch.cuda.synchronize()
    assert rc == L.RVLM_ERR_STATE, rc
    assert bool((gbuf == SENT).all()) and bool((bbuf == SENT).all()) and bool((red == SENT).all())
    L.check(run_ln(dy, C, x, C, mean, rstd, R, C, dg, db, 0, red, need), "ln_param_grad")
    torch.cuda.synchronize()
    assert torch.equal(db, torch.full((C,), float(R), device=dev()))


# --------------------------------------------------------------------------------------------------------------------------
# 3. reduce_partials16_kernel at chunk counts that are no multiple of 16
# --------------------------------------------------------------------------------------------------------------------------
def transposed_arm_tiles(M, N, K):
    """64-row tiles (= partial rows handed to reduce_partials16_kernel) of transpose_split for this weight gradient: splits * Kc / 64
    with the plan of csrc/gemm_bf16.hip wgrad_split_plan (slabs never the limit through the hook)."""
    tiles, nk128 = (N // 256) * (K // 256), (M + 127) // 128
    sp = min(max(1, min(16, 256 // tiles)), nk128)
    return sp * ((nk128 + sp - 1) // sp) * 128 // 64


@pytest.mark.parametrize("M,N,K,rt", [(300, 768, 256, 6), (257 * 7, 256, 256, 30), (257 * 9, 1024, 3072, 40), (257 * 24, 1024, 1536, 100)])
def test_reduce_partials_odd_chunk_counts_through_wgrad(M, N, K, rt):
    """Through colsum the second pass only ever sees 1, 16 or 128 partial rows (1 is covered above at every R < 256).  The transposed
    arm of rvlm_k_wgrad_bf16 - the library's hook (rvlm_k_wgrad_set_transposed; the engine itself has no switch to that arm) - emits
    one partial row per 64-row tile: 6, 30, 40, 100.  The bias gradient per element, both accumulate modes."""
    l = lib()
    assert transposed_arm_tiles(M, N, K) == rt and rt % 16 != 0
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    dy = torch.randn(M, N, generator=g, device=dev()).bfloat16()
    hr = M - 1
    dy[hr] = (100.0 * (1 + torch.arange(N, device=dev()) % 3)).bfloat16()       # the last row: the short tile's
    X = torch.randn(M, K, generator=g, device=dev()).bfloat16()
    _, dyv = in_nan(dy, N + 64, tail_rows=4096)
    _, xv = in_nan(X, K + 8, tail_rows=4096)
    ref, floor = colsum_ref(dy)
    nb = l.rvlm_k_wgrad_work_bytes(M, N, K)
    work = torch.empty(nb, dtype=torch.uint8, device=dev())
    dW = torch.empty(N, K, device=dev())
    prior = torch.randn(N, generator=g, device=dev()) * float(M) ** 0.5
    l.rvlm_k_wgrad_set_transposed(1)
    try:
        obuf, db = out_guarded(N, NAN)
        L.check(l.rvlm_k_wgrad_bf16(dyv.data_ptr(), N + 64, xv.data_ptr(), K + 8, M, N, K, dW.data_ptr(), K, 0, db.data_ptr(),
                                    work.data_ptr(), nb, st()), "wgrad")
        torch.cuda.synchronize()
        assert guards_intact(obuf, N)
        w0 = assert_elems(f"wgrad transposed arm dbias M {M} N {N} ({rt} partial rows)", db, ref, floor, BAR_COLSUM, dims=("col",))
        obuf, db = out_guarded(N, prior)
        L.check(l.rvlm_k_wgrad_bf16(dyv.data_ptr(), N + 64, xv.data_ptr(), K + 8, M, N, K, dW.data_ptr(), K, 1, db.data_ptr(),
                                    work.data_ptr(), nb, st()), "wgrad")
        torch.cuda.synchronize()
        assert guards_intact(obuf, N)
        w1 = assert_elems(f"wgrad transposed arm dbias accumulate M {M} N {N}", db, ref + prior.double(), floor + prior.double().abs(),
                          BAR_COLSUM, dims=("col",))
    finally:
        l.rvlm_k_wgrad_set_transposed(0)
    record("train_kernels_reduce_partials_odd", M=M, N=N, K=K, partial_rows=rt, worst=w0, worst_accumulate=w1)


# --------------------------------------------------------------------------------------------------------------------------
# 4. pos_cls_grad, gather_patch_rows, transpose_pad
# --------------------------------------------------------------------------------------------------------------------------
# (5, 197, 100): S * W = 19 700 is no multiple of the 256-thread workgroup; (128, 257, 1024): the training step at B = 128
EMBED_SHAPES = [(1, 17, 192), (3, 50, 768), (128, 257, 1024), (5, 197, 100)]


@pytest.mark.parametrize("B,S,W", EMBED_SHAPES)
def test_pos_cls_grad_elements(B, S, W):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + S + W)
    ld = W + 8
    dtok = torch.randn(B * S, W, generator=g, device=dev())
    dtok[(B - 1) * S:] *= 100.0                                  # the last image dominates: dropping it is an O(1) error
    _, dv = in_nan(dtok, ld)
    ref = dtok.view(B, S, W).sum(0, dtype=torch.float64)
    floor = torch.linalg.vector_norm(dtok.view(B, S, W), 2, dim=0, dtype=torch.float64)
    if (B, S, W) == (5, 197, 100):
        assert (S * W) % 256 != 0
    pbuf, dpos = out_guarded(S * W, NAN)
    cbuf, dcls = out_guarded(W, NAN)
    L.check(l.rvlm_k_pos_cls_grad(dv.data_ptr(), ld, B, S, W, dpos.data_ptr(), dcls.data_ptr(), 0, st()), "pos_cls_grad")
    torch.cuda.synchronize()
    assert guards_intact(pbuf, S * W) and guards_intact(cbuf, W)
    name = f"pos_cls_grad B {B} S {S} W {W}"
    w0 = assert_elems(name, dpos.view(S, W), ref, floor, BAR_POS, dims=("token", "col"))
    assert torch.equal(dcls.view(torch.int32), dpos[:W].view(torch.int32)), f"{name}: dcls is not row 0 of dpos bit for bit"
    # accumulate: dpos onto a known tensor, dcls onto that tensor's row 0 (equal bits again), then dcls onto a tensor of its own
    prior = torch.randn(S, W, generator=g, device=dev()) * float(B) ** 0.5
    own = torch.randn(W, generator=g, device=dev()) * float(B) ** 0.5 - 2.0
    w1 = 0.0
    for pc in (prior[0], own):
        pbuf, dpos = out_guarded(S * W, prior)
        cbuf, dcls = out_guarded(W, pc)
        L.check(l.rvlm_k_pos_cls_grad(dv.data_ptr(), ld, B, S, W, dpos.data_ptr(), dcls.data_ptr(), 1, st()), "pos_cls_grad")
        torch.cuda.synchronize()
        assert guards_intact(pbuf, S * W) and guards_intact(cbuf, W)
        w1 = max(w1, assert_elems(name + " accumulate", dpos.view(S, W), ref + prior.double(), floor + prior.double().abs(), BAR_POS,
                                  dims=("token", "col")))
        w1 = max(w1, assert_elems(name + " accumulate dcls", dcls, ref[0] + pc.double(), floor[0] + pc.double().abs(), BAR_POS, dims=("col",)))
        if pc is not own:
            assert torch.equal(dcls.view(torch.int32), dpos[:W].view(torch.int32)), f"{name} accumulate: dcls is not row 0 of dpos bit for bit"
    record("train_kernels_pos_cls_grad", B=B, S=S, W=W, worst=w0, worst_accumulate=w1)


# (9, 197, 768): 1.35 M elements, just over the 4 096 x 256 threads of the capped grid; (128, 257, 1024) wraps 32 times
@pytest.mark.parametrize("bf16_out", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,S,W", EMBED_SHAPES + [(9, 197, 768)])
def test_gather_patch_rows_bits(B, S, W, bf16_out):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + S + W)
    ld, ldp = W + 8, W + 16
    dtok = torch.randn(B * S, W, generator=g, device=dev())
    # every 5th row: exact ties of the bf16 rounding (low half 0x8000) on both parities of the kept mantissa's last bit
    ties = dtok[::5].contiguous().view(torch.int32)
    dtok[::5] = ((ties & -65536) | 0x8000).view(torch.float32)
    dtok[0::S] = NAN                                              # the class rows are never read
    _, dv = in_nan(dtok, ld)
    rows = B * (S - 1)
    assert (B, S, W) not in ((9, 197, 768), (128, 257, 1024)) or rows * W > 4096 * 256
    odt = torch.bfloat16 if bf16_out else torch.float32
    obuf = torch.full((rows + 2 * GUARD, ldp), SENT, dtype=odt, device=dev())
    out = obuf[GUARD:GUARD + rows]
    L.check(l.rvlm_k_gather_patch_rows(dv.data_ptr(), ld, B, S, W, out.data_ptr(), ldp, bf16_out, st()), "gather_patch_rows")
    torch.cuda.synchronize()
    want = dtok.view(B, S, W)[:, 1:].reshape(rows, W)
    assert not bool(want.isnan().any())
    want = want.to(odt)                                           # torch rounds to nearest even
    ibits = torch.int16 if bf16_out else torch.int32
    same = out[:, :W].contiguous().view(ibits) == want.contiguous().view(ibits)
    bad = (~same).nonzero()
    assert bad.numel() == 0, f"gather_patch_rows B {B} S {S} W {W}: {bad.shape[0]} elements differ, first at (patch row, col) {bad[0].tolist()}"
    assert bool((out[:, W:] == SENT).all()), "pad columns of d_patch were written"
    assert bool((obuf[:GUARD] == SENT).all()) and bool((obuf[GUARD + rows:] == SENT).all()), "rows outside d_patch were written"


# R = 1; C = 588 (conv1 at P = 14, 3 * 14 * 14); Rp > R by more than one 64-row tile (195 -> 448, 65 -> 200)
@pytest.mark.parametrize("R,C,Rp", [(1, 588, 64), (64, 64, 64), (128, 192, 128), (100, 588, 128), (257, 100, 320), (195, 1024, 448),
                                    (1028, 588, 1088), (65, 65, 200), (4112, 1024, 4160)])
def test_transpose_pad_bits(R, C, Rp):
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(R * 100 + C)
    t = torch.randn(R, C, generator=g, device=dev()).bfloat16()
    _, tv = in_nan(t, C + 8)
    ldo = Rp + 24
    obuf = torch.full((C + 2 * GUARD, ldo), SENT, dtype=torch.bfloat16, device=dev())
    out = obuf[GUARD:GUARD + C]
    L.check(l.rvlm_k_transpose_pad(tv.data_ptr(), C + 8, R, C, out.data_ptr(), ldo, Rp, st()), "transpose_pad")
    torch.cuda.synchronize()
    name = f"transpose_pad R {R} C {C} Rp {Rp}"
    same = out[:, :R].contiguous().view(torch.int16) == t.t().contiguous().view(torch.int16)
    bad = (~same).nonzero()
    assert bad.numel() == 0, f"{name}: {bad.shape[0]} elements differ, first at out[{bad[0].tolist()}]"
    pad = out[:, R:Rp].contiguous().view(torch.int16)
    assert bool((pad == 0).all()), f"{name}: rows R .. Rp - 1 are not all +0 ({int((pad != 0).sum())} elements)"
    assert bool((out[:, Rp:] == SENT).all()), f"{name}: wrote beyond column Rp"
    assert bool((obuf[:GUARD] == SENT).all()) and bool((obuf[GUARD + C:] == SENT).all()), f"{name}: wrote outside [C, Rp]"


# --------------------------------------------------------------------------------------------------------------------------
# 5. rvlm_adamw_step
# --------------------------------------------------------------------------------------------------------------------------
LR, B1, B2 = 1e-3, 0.9, 0.999


def adamw_fp64(p, g, m, v, step, lr, b1, b2, eps, wd, grad_scale):
    """torch.optim.AdamW as documented (decoupled weight decay, no amsgrad), in fp64:
        theta <- theta - lr * wd * theta;  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2
        mhat = m / (1 - b1^t);  vhat = v / (1 - b2^t);  theta <- theta - lr * mhat / (sqrt(vhat) + eps)
    on the gradient the kernel sees: fp32(g * grad_scale).  Returns (p, m, v, the scale of p's error: |p| + the update with the two
    terms of m added by magnitude - where b1 m and (1 - b1) g cancel, the update is small but its rounding error is not)."""
    gd = (g * grad_scale).double()
    p, m0, v = p.double(), m.double(), v.double()
    scale = p.abs()
    p = p - lr * wd * p
    m = b1 * m0 + (1 - b1) * gd
    v = b2 * v + (1 - b2) * gd * gd
    per_m = lr / (1 - b1 ** step) / ((v / (1 - b2 ** step)).sqrt() + eps)
    return p - per_m * m, m, v, scale + per_m * (b1 * m0.abs() + (1 - b1) * gd.abs())


@pytest.mark.parametrize("wd,eps,grad_scale", [(0.0, 1e-8, 1.0), (1e-4, 1e-8, 0.125), (1e-2, 1e-6, 0.5)])
@pytest.mark.parametrize("n", [1, 255, 1024, 1025, 4096 * 256 + 3, 8 * 4096 * 256 + 1])
def test_adamw_step_elements(n, wd, eps, grad_scale):
    """One update from a given state at step 1, 2, 1 400 and 20 000 (bias corrections from 0.1 / 0.001 to 1), per element against the
    documented update in fp64 and against torch.optim.AdamW on the CPU in fp32 (its state advanced by setting state['step']); p, m and
    v are all checked, and the elements behind n.  The launch covers 4 096 x 256 threads at most: 4 096 x 256 + 3 and 8 x 4 096 x 256
    + 1 elements take the grid-stride loop once and eight times over.  The gradient holds exact zeros (on elements whose moments are
    zero too: the denominator is eps alone) and entries of +-1e4."""
    l = lib()
    g = torch.Generator(device="cuda").manual_seed(n % 100003 + int(wd * 1e4))
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "torch": 0.0}
    for step in (1, 2, 1400, 20000):
        p0 = 1e-2 * torch.randn(n, generator=g, device=dev())      # weights of the update's own size: an error of the update shows in p
        grad = 0.1 * torch.randn(n, generator=g, device=dev())
        m0 = 0.05 * torch.randn(n, generator=g, device=dev()) if step > 1 else torch.zeros(n, device=dev())
        v0 = (0.05 * torch.randn(n, generator=g, device=dev())) ** 2 if step > 1 else torch.zeros(n, device=dev())
        idx = torch.arange(n, device=dev())
        zero = idx % 7 == 3
        grad[zero] = 0.0; m0[zero] = 0.0; v0[zero] = 0.0          # gradient, moments all exactly zero: 0 / eps
        m0[idx % 14 == 3] = 1e-10 if step > 1 else 0.0             # ... and a moment of 1e-10 over eps alone
        grad[idx % 11 == 5] = 1e4
        grad[idx % 11 == 6] = -1e4
        gdev = grad / grad_scale                                   # the kernel multiplies by grad_scale (powers of two: exact)
        bufs = []
        for t in (p0, m0, v0):
            b = torch.full((n + 2 * GUARD,), SENT, device=dev())
            b[GUARD:GUARD + n] = t
            bufs.append(b)
        dp, dm, dv = (b[GUARD:GUARD + n] for b in bufs)
        L.check(l.rvlm_adamw_step(dp.data_ptr(), gdev.data_ptr(), dm.data_ptr(), dv.data_ptr(), n, LR, B1, B2, eps, wd, step, grad_scale, st()),
                "adamw")
        torch.cuda.synchronize()
        for b in bufs:
            assert guards_intact(b, n), f"adamw n {n}: wrote outside its {n} elements"
        rp, rm, rv, pscale = adamw_fp64(p0, gdev, m0, v0, step, LR, B1, B2, eps, wd, grad_scale)
        name = f"adamw n {n} step {step} wd {wd} eps {eps} grad_scale {grad_scale}"
        gs = (gdev * grad_scale).double().abs()
        worst["p"] = max(worst["p"], assert_elems(name + " p", dp, rp, pscale, BAR_ADAMW["p"], dims=("element",)))
        worst["m"] = max(worst["m"], assert_elems(name + " m", dm, rm, m0.double().abs() + gs, BAR_ADAMW["m"], dims=("element",)))
        worst["v"] = max(worst["v"], assert_elems(name + " v", dv, rv, rv, BAR_ADAMW["v"], dims=("element",)))
        # torch.optim.AdamW itself (CPU, fp32, single-tensor path)
        pt = p0.cpu().clone().requires_grad_(True)
        opt = torch.optim.AdamW([pt], lr=LR, betas=(B1, B2), eps=eps, weight_decay=wd, foreach=False)
        opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.cpu().clone(), "exp_avg_sq": v0.cpu().clone()}
        pt.grad = (gdev * grad_scale).cpu()
        opt.step()
        assert float(opt.state[pt]["step"]) == step
        wt = max(assert_elems(name + " p vs torch", dp.cpu(), pt.detach(), pscale.cpu(), BAR_ADAMW_TORCH, dims=("element",)),
                 assert_elems(name + " m vs torch", dm.cpu(), opt.state[pt]["exp_avg"], m0.cpu().double().abs() + gs.cpu(), BAR_ADAMW_TORCH,
                              dims=("element",)),
                 assert_elems(name + " v vs torch", dv.cpu(), opt.state[pt]["exp_avg_sq"], rv.cpu(), BAR_ADAMW_TORCH, dims=("element",)))
        worst["torch"] = max(worst["torch"], wt)
    record("train_kernels_adamw", n=n, wd=wd, eps=eps, grad_scale=grad_scale, worst_p=worst["p"], worst_m=worst["m"], worst_v=worst["v"],
           worst_vs_torch=worst["torch"])
