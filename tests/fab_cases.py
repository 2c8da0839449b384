"""Inputs of the FAB projection tests that are too large to store: rows of any length made by integer arithmetic (no random
generator whose stream could change), shared by tests/golden/make_golden_fab.py (which stores what the reference returns for
them) and the tests (which rebuild them)."""
import numpy as np


def _uniform(n, salt):
    """n reproducible values in [0, 1): a 32-bit multiplicative hash of the index."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(16)
    return h.astype(np.float64) / 4294967296.0


def hashed_row(D, salt, offset, zero_fraction=0.1):
    """(t [D] in [0, 1], w [D] with about zero_fraction exact zeros, b) as float32; b = w.t + offset."""
    t = _uniform(D, 3 * salt + 1).astype(np.float32)
    w = ((_uniform(D, 3 * salt + 2) - 0.5) * 2.0).astype(np.float32)
    w[_uniform(D, 3 * salt + 3) < zero_fraction] = 0.0
    b = np.float32(np.dot(w.astype(np.float64), t.astype(np.float64)) + offset)
    return t, w, b


def closed_form_lambda(t, w, b):
    """The contract in float64 by sorting: (lambda, feasible) with d_i = dir_i min(lambda, room_i)."""
    t, w = t.astype(np.float64), w.astype(np.float64)
    c = float(b) - float(np.dot(w, t))
    up = (w > 0) if c > 0 else (w < 0)
    room = np.where(w == 0, 0.0, np.where(up, 1.0 - t, t))
    aw, c = np.abs(w), abs(c)
    if c == 0 or aw.sum() == 0:
        return 0.0, c == 0
    if (aw * room).sum() <= c:
        return float(room.max()), (aw * room).sum() == c
    order = np.argsort(room)
    r, a = room[order], aw[order]
    sat = np.concatenate([[0.0], np.cumsum(a * r)])[:-1]       # sum of a r over the rooms before position k
    rest = a.sum() - np.concatenate([[0.0], np.cumsum(a)])[:-1]  # sum of a from position k on
    f_at = sat + r * rest                                       # f(room_k)
    k = int(np.searchsorted(f_at, c, side="left"))              # first k with f(room_k) >= c
    return float((c - sat[k]) / rest[k]), True
