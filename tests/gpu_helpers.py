"""Helpers shared by the -m gpu tests (call the C ABI of librvlm.so through ctypes)."""
import numpy as np
import torch

from robustvlm_amd import _lib as L


def dev():
    return torch.device("cuda:0")


def st():
    return L.stream_ptr()


def lib():
    return L.load()


def cos_sim(a, b):
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def rel_max(a, b):
    a = a.double()
    b = b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def pad_rows(t, mult=128):
    """Copy of a 2-D tensor whose storage is readable for round_up(rows, mult) rows."""
    r = (t.shape[0] + mult - 1) // mult * mult
    buf = torch.zeros(r, t.shape[1], dtype=t.dtype, device=t.device)
    buf[: t.shape[0]] = t
    return buf


K_128, K_PERSISTENT, K_SPLITK, K_STRIP = 1, 4, 16, 32   # include/rvlm_kernels.h RVLM_GEMM_K_*


def persistent_expected(M, N, K):
    """Kernel families rvlm_k_gemm_set_variant(3) must launch for an [M,K] x [N,K]^T problem."""
    if M >= 256 and N % 256 == 0 and K % 128 == 0:
        return K_PERSISTENT | (K_STRIP if M % 256 else 0)
    return None


def record(name, **values):
    """Append measured parity numbers to gpurun_out/parity_metrics.jsonl (evidence for DESIGN.md / profiles/)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_metrics.jsonl"), "a") as f:
            f.write(json.dumps(dict(test=name, **{k: float(v) for k, v in values.items()})) + "\n")
    except OSError:
        pass


def gemm_bf16(A, Bw, epi=0, bias=None, residual=None, h_pre=None, act=0, expect=None):
    """A [M,K] bf16, Bw [N,K] bf16 (cuda).  Returns (out, out_pre).  ``expect``: bit mask of kernel families
    (K_*) that must have run - the dispatcher may not silently route a test to another kernel."""
    l = lib()
    M, K = A.shape
    N = Bw.shape[0]
    Ap = pad_rows(A.contiguous())
    Bc = Bw.contiguous()
    out_dtype = torch.float32 if epi in (1, 4) else torch.bfloat16
    out = torch.zeros(M, N, dtype=out_dtype, device=A.device)
    out_pre = torch.zeros(M, N, dtype=torch.bfloat16, device=A.device) if epi == 2 else None
    L.check(l.rvlm_k_gemm_bf16_nt(Ap.data_ptr(), K, Bc.data_ptr(), K, M, N, K, Ap.shape[0], epi,
                                  L.ptr(bias), out.data_ptr(), N, L.ptr(out_pre), L.ptr(h_pre),
                                  L.ptr(residual), act, st()), "gemm_bf16")
    torch.cuda.synchronize()
    if expect is not None:
        ran = l.rvlm_k_gemm_last_kernels()
        assert ran == expect, \
            f"GEMM [{M},{K}]x[{N},{K}]^T epi {epi}: kernel families {ran:#x} ran, expected {expect:#x}"
    return out, out_pre


def act_ref(h, act):
    if act == 0:
        return h * torch.sigmoid(1.702 * h)
    return torch.nn.functional.gelu(h)


def dact_ref(h, act):
    h = h.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(act_ref(h, act).sum(), h)
    return g


def attn_ref(qkv, B, H, S):
    """fp64 reference of softmax(q k^T / 8) v on packed qkv [B*S, 3W]; returns o [B*S, W]."""
    W = H * 64
    q, k, v = qkv.double().reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    o = torch.softmax(s, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * S, W)


def row_rel_l2(got, ref):
    """Relative L2 error of every row (the last dimension) in fp64.  The rows of one group (the second-to-last dimension: the tokens of
    one (image, head) for attention, all rows of a matrix otherwise) share a floor: a row's error norm is divided by max(its reference
    norm, 0.05 x the group's median row norm), so that rows whose true value is nearly zero (keys nobody attends to under a peaked
    softmax) are judged on an absolute scale instead of being exempted or made to flake."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).norm(dim=-1)
    nrm = ref.norm(dim=-1)
    floor = 0.05 * nrm.median(dim=-1, keepdim=True).values
    return err / torch.maximum(nrm, floor).clamp_min(1e-300)


def assert_rows(name, got, ref, bar, dims=("b", "h", "row")):
    """Every row of ``got`` within ``bar`` of ``ref`` (row_rel_l2); the message names the worst row.  Returns the worst value."""
    e = row_rel_l2(got, ref)
    flat = int(torch.nan_to_num(e, nan=float("inf")).argmax())          # a NaN row is the worst row
    idx = np.unravel_index(flat, tuple(e.shape))
    worst = float(e.flatten()[flat])
    where = ", ".join(f"{n} {i}" for n, i in zip(dims[len(dims) - len(idx):], idx))
    assert worst <= bar, f"{name}: worst row ({where}) has relative L2 error {worst:.3e} > {bar:.1e}"
    return worst


def elem_rel(got, ref, floor):
    """Element-wise |got - ref| / max(|ref|, floor) in fp64.  ``floor`` (broadcast against ref) is the absolute scale of an element:
    for a sum of R terms the L2 norm of its terms (sqrt(R) x their RMS), so that a sum that nearly cancels is judged against the size
    of what was added up instead of against its own near-zero value."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs() / torch.maximum(ref.abs(), floor.double().expand_as(ref)).clamp_min(1e-300)


def assert_elems(name, got, ref, floor, bar, dims=("row", "col")):
    """Every element of ``got`` within ``bar`` of ``ref`` (elem_rel); the message names the worst element.  Returns the worst value."""
    e = elem_rel(got, ref, floor)
    flat = int(torch.nan_to_num(e, nan=float("inf")).argmax())          # a NaN element is the worst element
    idx = np.unravel_index(flat, tuple(e.shape))
    worst = float(e.flatten()[flat])
    where = ", ".join(f"{n} {i}" for n, i in zip(dims[len(dims) - len(idx):], idx))
    assert worst <= bar, (f"{name}: worst element ({where}) is {float(got.flatten()[flat])!r}, reference {float(ref.flatten()[flat])!r}: "
                          f"error {worst:.3e} of its scale > {bar:.1e}")
    return worst
