"""tests/golden/token_apgd_tiny.npz (made by tests/golden/make_golden_token_apgd.py from the reference's apgd()): reading it, and the
lossless packing of its images that keeps the file under the size limit for a committed file.

An iterate ``a`` of an attack on the image ``x`` is stored against a prediction ``p`` of it - L-inf: ``clip(x + sign(a - x) * eps, 0,
1)``, where most pixels of an APGD iterate end; L2: ``x`` - as the XOR of the two float32 bit patterns, byte plane by byte plane
(plane j = byte j of every element), plus the sign plane.  Where the prediction is exact the XOR is zero, elsewhere its leading bytes
are; zlib does the rest.  Both directions are numpy float32 / integer arithmetic: bit-exact on every host."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_apgd_tiny.npz")


def _predict(x, sign, eps):
    return np.clip(x + sign.astype(np.float32) * np.float32(eps), np.float32(0), np.float32(1)).astype(np.float32)


def pack(a, x, eps):
    """(sign int8 like a, planes uint8 [4, a.size]) of the float32 array ``a`` against ``x`` (same shape); eps = 0: predict x."""
    a, x = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(x, np.float32)
    sign = np.sign(a - x).astype(np.int8) if eps else np.zeros(a.shape, np.int8)
    xor = a.view(np.uint32) ^ _predict(x, sign, eps).view(np.uint32)
    return sign, np.ascontiguousarray(xor.astype("<u4").reshape(-1).view(np.uint8).reshape(-1, 4).T)


def unpack(sign, planes, x, eps):
    x = np.ascontiguousarray(x, np.float32)
    xor = np.ascontiguousarray(planes.T).view("<u4").reshape(x.shape).astype(np.uint32)
    return (xor ^ _predict(x, sign, eps).view(np.uint32)).view(np.float32)


def pack_eps(case):
    return case["eps"] if case["norm"] == "linf" else 0.0


_cache = {}


def load():
    """(cases: list of dicts, get(name) -> dict(x, pert_init, x_best, x_last, loss_best, trace, step_seen)); arrays are numpy."""
    if "d" not in _cache:
        d = np.load(PATH)
        _cache["d"] = d
        _cache["cases"] = json.loads(str(d["cases"]))
    d, cases = _cache["d"], _cache["cases"]
    by_name = {c["name"]: c for c in cases}

    def get(name):
        if name in _cache:
            return _cache[name]
        c, x = by_name[name], d["x"]
        e = pack_eps(c)
        x_best = unpack(d[name + "/x_best_sign"], d[name + "/x_best"], x, e)
        x_last = x_best.copy()
        idx = d[name + "/x_last_idx"]
        if len(idx):
            x_last[idx] = unpack(d[name + "/x_last_sign"], d[name + "/x_last_rows"], x[idx], e)
        _cache[name] = dict(x=x, pert_init=pert_init(c["norm"], c["eps"], d["u"]), x_best=x_best, x_last=x_last,
                            loss_best=d[name + "/loss_best"], trace=d[name + "/trace"], step_seen=d[name + "/step_seen"])
        return _cache[name]
    return cases, get


def pert_init(norm, eps, u):
    """The start perturbation of a case from the stored direction u in [-1, 1]: L-inf eps * u, L2 0.5 eps u / |u|_2 (float32)."""
    u = np.asarray(u, np.float32)
    if norm == "linf":
        return (np.float32(eps) * u).astype(np.float32)
    nrm = np.sqrt((u.astype(np.float64) ** 2).reshape(u.shape[0], -1).sum(1)).astype(np.float32).reshape(-1, 1, 1, 1)
    return (np.float32(0.5 * eps) * u / nrm).astype(np.float32)
