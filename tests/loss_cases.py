"""Inputs and plain torch restatements for the loss-kernel tests (csrc/loss_kernels.hip), shared by tests/test_loss_host.py (which
anchors the restatements to the reference's recorded outputs in tests/golden/) and tests/test_gpu_loss_kernels.py (which holds the
kernels to them).  Every case is a deterministic function of (family, C or D, B, seed): a seeded CPU generator, then values placed
by construction, so the property a family promises (which lane holds which rank, where the ties are) does not depend on the draw.

The kernels give one 64-lane wave to a row and lane i reads elements i, i + 64, ...: "lane" below is index % 64."""
import itertools
import zlib

import numpy as np
import torch

LANES = 64


def _gen(family, n, B, seed):
    fid = zlib.crc32(family.encode()) % 9973
    return torch.Generator().manual_seed(((fid * 1000003 + n) * 1013 + B) * 1019 + seed)


def _other_label(g, y, C):
    """A label per row that differs from y (C >= 2)."""
    t = torch.randint(0, C, y.shape, generator=g)
    return torch.where(t == y, (t + 1) % C, t)


# ---------------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------------
def dlr_ref(x, y):
    """The untargeted DLR loss (autoattack/autopgd_base.py:195-201) in the dtype of x, in the reference's operation order."""
    x_sorted, ind_sorted = x.sort(dim=1)
    ind = (ind_sorted[:, -1] == y).to(x.dtype)
    u = torch.arange(x.shape[0])
    return -(x[u, y] - x_sorted[:, -2] * ind - x_sorted[:, -1] * (1. - ind)) / (x_sorted[:, -1] - x_sorted[:, -3] + 1e-12)


def dlr_targeted_ref(x, y, y_target):
    """The targeted DLR loss (autoattack/autopgd_base.py:613-618) in the dtype of x, in the reference's operation order."""
    x_sorted, _ = x.sort(dim=1)
    u = torch.arange(x.shape[0])
    return -(x[u, y] - x[u, y_target]) / (x_sorted[:, -1] - .5 * (x_sorted[:, -3] + x_sorted[:, -4]) + 1e-12)


def grad_of_sum(fn, x, *args):
    """(fn(x, *args), d sum(fn) / d x) by autograd, in the dtype of x."""
    xr = x.detach().clone().requires_grad_(True)
    val = fn(xr, *args)
    (g,) = torch.autograd.grad(val.sum(), xr)
    return val.detach(), g


def ce_ref(logits, y):
    """fp64 (loss [B], d sum(loss) / d logits [B, C]) of cross entropy: logsumexp - logit[y], softmax - onehot."""
    x = logits.double()
    lse = torch.logsumexp(x, dim=1)
    u = torch.arange(x.shape[0])
    grad = torch.exp(x - lse[:, None])
    grad[u, y] -= 1.0
    return lse - x[u, y], grad


def head_ce_ref(emb, T, y, scale):
    """fp64 (loss [B], d sum(loss) / d emb) of cross_entropy(emb @ (scale T)) by autograd."""
    e = emb.double().detach().clone().requires_grad_(True)
    val = torch.nn.functional.cross_entropy(e @ (scale * T.double()), y, reduction="none")
    (g,) = torch.autograd.grad(val.sum(), e)
    return val.detach(), g


def l2_ref(e, r):
    """fp64 per-sample sum_d (e - r)^2."""
    return ((e.double() - r.double()) ** 2).sum(dim=1)


def cosine_ref(a, b):
    """fp64 a.b / sqrt(max(|a|^2 |b|^2, 1e-16)) per row (the formula include/rvlm.h documents for rvlm_cosine_rows)."""
    a, b = a.double(), b.double()
    ab, aa, bb = (a * b).sum(1), (a * a).sum(1), (b * b).sum(1)
    return ab / torch.sqrt(torch.clamp(aa * bb, min=1e-16))


def argmax_first(logits):
    """First-index arg-max per row (np.argmax guarantees the first occurrence), as an int64 numpy array."""
    return np.argmax(logits.detach().cpu().numpy(), axis=1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# DLR logit families
# ---------------------------------------------------------------------------------------------------------------------------
DLR_FAMILIES = ("randn", "one_lane", "two_two", "ends", "ranks", "ties")
TOP4 = (40.0, 36.5, 33.25, 30.125)      # distinct, well above randn * 3 (clamped to 15 where these are placed)
_PERMS4 = list(itertools.permutations(range(4)))


def dlr_families(C):
    """The families that fit C classes."""
    fits = {"randn": C >= 3, "one_lane": C >= 256, "two_two": C >= 66, "ends": C >= 3, "ranks": C >= 3, "ties": C >= 3}
    return [f for f in DLR_FAMILIES if fits[f]]


def _tie_catalogue(C):
    """(top values by rank, tied ranks, where y goes) of the `ties` rows that fit C: two-way ties at ranks (1,2) .. (4,5) with y
    inside the pair (its smaller or its larger index) and outside it, and one three-way tie at the top."""
    tops = {(1, 2): (20., 20., 18., 17., 16.), (2, 3): (20., 18., 18., 17., 16.), (3, 4): (20., 19., 18., 18., 16.),
            (4, 5): (20., 19., 18., 17., 17.)}
    rows = []
    for n, (pair, vals) in enumerate(tops.items()):
        if pair[1] > C:
            continue
        rows.append((vals, pair, "low" if n % 2 == 0 else "high"))
        rows.append((vals, pair, "out"))
    rows.append(((20., 20., 20., 17., 16.), (1, 2, 3), "mid"))
    return rows


def dlr_case(family, C, B, seed=0):
    """-> dict(x [B, C] fp32, y [B], y_target [B] (never equal to y), ties: bool - compare gradients per distinct value,
    value_only [B] bool - rows whose gradient is not compared (den = 1e-12))."""
    g = _gen("dlr_" + family, C, B, seed)
    x = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    yt = None
    value_only = torch.zeros(B, dtype=torch.bool)
    if family == "randn":
        y[::3] = x[::3].argmax(1)                          # rows with the label on top (the ind = 1 branch)
    elif family == "one_lane":
        assert C >= 4 * LANES
        x.clamp_(max=15.0)
        for b in range(B):
            r = (17 * seed + 5 * b + C) % LANES            # every lane has >= 4 elements when C >= 256
            slots = torch.randperm((C - r + LANES - 1) // LANES, generator=g)[:4].sort().values
            perm = _PERMS4[(b + seed) % 24]                 # which rank the lane meets first, second, ...
            for k in range(4):
                x[b, r + LANES * int(slots[k])] = TOP4[perm[k]]
            top = x[b].argsort(descending=True)
            if b % 3 != 2:
                y[b] = top[b % 3]                           # the label on top, second, or (b % 3 == 2) wherever it fell
    elif family == "two_two":
        assert C >= LANES + 2
        x.clamp_(max=15.0)
        for b in range(B):
            la, lb = (int(v) for v in torch.randperm(min(LANES, C - LANES), generator=g)[:2])
            for lane, ranks in ((la, (0, 2)), (lb, (1, 3))):
                s = torch.randperm((C - lane + LANES - 1) // LANES, generator=g)[:2]
                x[b, lane + LANES * int(s[0])] = TOP4[ranks[0]]
                x[b, lane + LANES * int(s[1])] = TOP4[ranks[1]]
            if b % 2 == 0:
                y[b] = x[b].argsort(descending=True)[(b // 2) % 4]
    elif family == "ends":
        x.clamp_(max=15.0)
        x[:, C - 1] = TOP4[0]
        x[:, 0] = TOP4[1]
        y[0::3] = C - 1
        y[1::3] = 0
    elif family == "ranks":
        assert all(len(set(row.tolist())) == C for row in x), "a draw with equal logits: choose another seed"
        order = x.argsort(dim=1, descending=True)
        yt = torch.empty_like(y)
        for b in range(B):
            ry = min(b % 5 + 1, C)
            rt = b % 4 + 1
            if rt == ry or rt > C:
                rt = rt % min(4, C) + 1
            y[b], yt[b] = order[b, ry - 1], order[b, rt - 1]
    elif family == "ties":
        x = (x.clamp(max=10.0) * 2).round() / 2
        cat = _tie_catalogue(C)
        yt = torch.empty_like(y)
        for b in range(B):
            vals, tied, where = cat[(b + seed + C) % len(cat)]
            n = min(5, C)
            idx = torch.randperm(C, generator=g)[:n].tolist()
            if where != "out" and len(tied) == 2 and C >= 2 * LANES + 5:   # the tied pair inside one lane
                i = idx[tied[0] - 1] % (C - LANES)
                pair = [i, i + LANES]
                rest = [j for j in torch.randperm(C, generator=g).tolist() if j not in pair][:n - 2]
                idx = rest[:tied[0] - 1] + pair + rest[tied[0] - 1:]
            for k in range(n):
                x[b, idx[k]] = vals[k]
            members = sorted(idx[r - 1] for r in tied)
            if where == "out":
                y[b] = [idx[r - 1] for r in range(1, n + 1) if r not in tied][b % (n - 2)] if n > 2 else idx[0]
            else:
                y[b] = {"low": members[0], "high": members[-1], "mid": members[1]}[where]
            cand = [j for j in idx[:4] if j != int(y[b])]
            yt[b] = cand[b % len(cand)]
            value_only[b] = len(tied) == 3
    else:
        raise ValueError(family)
    if yt is None:
        yt = _other_label(g, y, C)
    assert not bool((yt == y).any())
    return dict(x=x.float().contiguous(), y=y, y_target=yt, ties=family == "ties", value_only=value_only)


# ---------------------------------------------------------------------------------------------------------------------------
# cross-entropy logit families
# ---------------------------------------------------------------------------------------------------------------------------
CE_FAMILIES = ("randn5", "scaled", "offset", "dominant", "ties")


def ce_families(C):
    return [f for f in CE_FAMILIES if f != "ties" or C >= 2]


def ce_case(family, C, B, seed=0):
    """-> (logits [B, C] fp32, y [B])."""
    g = _gen("ce_" + family, C, B, seed)
    y = torch.randint(0, C, (B,), generator=g)
    if family == "randn5":
        x = torch.randn(B, C, generator=g) * 5
    elif family == "scaled":                                # what the zero-shot head produces: 100 x cosines of unit vectors
        e = torch.nn.functional.normalize(torch.randn(B, 64, generator=g, dtype=torch.float64), dim=1)
        T = torch.nn.functional.normalize(torch.randn(64, C, generator=g, dtype=torch.float64), dim=0)
        x = (e @ T) * 100.0
    elif family == "offset":                                # expf overflows here without the max subtraction
        x = torch.randn(B, C, generator=g) * 30 + 1.0e4
    elif family == "dominant":                              # p - 1 cancels at the label
        x = torch.randn(B, C, generator=g)
        x[torch.arange(B), y] = x.max(dim=1).values + 40.0
    elif family == "ties":                                  # the maximum occurs twice; the label is the later index
        x = torch.randn(B, C, generator=g) * 5
        top = x.max(dim=1).values + 1.0
        for b in range(B):
            i, j = sorted(torch.randperm(C, generator=g)[:2].tolist())
            x[b, i] = x[b, j] = top[b]
            y[b] = j
    else:
        raise ValueError(family)
    return x.float().contiguous(), y


def unit_rows(B, D, g):
    return torch.nn.functional.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1).float()


def head_case(B, D, C, seed=0):
    """-> (emb [B, D] with unit-norm rows, T [D, C] with unit-norm columns, y [B]), fp32."""
    g = _gen("head", D * 2048 + C, B, seed)
    emb = unit_rows(B, D, g)
    T = unit_rows(C, D, g).t().contiguous()
    return emb, T, torch.randint(0, C, (B,), generator=g)
