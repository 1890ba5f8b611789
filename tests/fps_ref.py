"""Numpy restatement of dpf_fps (include/dpf_hip.h: the farthest-point sampling block), round for round, in fp32 with the operation
order written out:

    d(i, j) = (dx*dx + dy*dy) + dz*dz,  dx = x_i - x_j (the same per axis), every fp32 operation rounded on its own;
    sel_0 = start, mind_0[i] = d(i, sel_0); sel_t = the lowest index attaining max_i mind_(t-1)[i],
    mind_t[i] = min(mind_(t-1)[i], d(i, sel_t)); radius2[t] = max_i mind_t[i].

The argmax is the kernel's packed key: mind >= +0 never NaN, so its bit pattern orders as an unsigned integer; the key is
bits(mind) << 32 | (0xffffffff - index) and its plain maximum is the largest mind at the lowest index.  A cloud with a non-finite
coordinate or a start outside [0, n) is refused: index -1, radius2 NaN, status -1.  Finite coordinates whose differences or squares
overflow give +inf, an ordinary maximum: not refused."""
import numpy as np

REFUSED = -1


def dist2(pts, j):
    """(n,) fp32 squared distances of every point to point j, each operation an fp32 array operation of its own"""
    with np.errstate(over="ignore"):
        dx = pts[:, 0] - pts[j, 0]
        dy = pts[:, 1] - pts[j, 1]
        dz = pts[:, 2] - pts[j, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        s = xx + yy
        return s + zz


def packed_argmax(mind):
    """(index, the maximum's fp32 value) by the packed 64-bit key"""
    bits = mind.view(np.uint32).astype(np.uint64)
    idx = np.arange(mind.shape[0], dtype=np.uint64)
    key = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
    best = key.max()
    hi = np.array([int(best) >> 32], dtype=np.uint32).view(np.float32)[0]
    return int(0xFFFFFFFF - (int(best) & 0xFFFFFFFF)), hi


def fps(pts, k, start=0):
    """pts (n, 3) -> (index (k,) int32, radius2 (k,) fp32, status)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n = pts.shape[0]
    assert pts.shape == (n, 3) and 1 <= k <= n
    index = np.full((k,), -1, dtype=np.int32)
    radius2 = np.full((k,), np.nan, dtype=np.float32)
    if not np.isfinite(pts).all() or not 0 <= int(start) < n:
        return index, radius2, REFUSED
    sel = int(start)
    mind = np.full((n,), np.inf, dtype=np.float32)
    for t in range(k):
        index[t] = sel
        mind = np.minimum(mind, dist2(pts, sel))
        assert mind.dtype == np.float32
        sel, radius2[t] = packed_argmax(mind)
    return index, radius2, 0


def fps_batch(clouds, k, start=None):
    """clouds (B, n, 3) -> index (B, k) int32, radius2 (B, k) fp32, status (B,) int32"""
    B = clouds.shape[0]
    out = [fps(clouds[b], k, 0 if start is None else int(start[b])) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


# ---- the clouds of the tests, from a seed ------------------------------------------------------------------------------------
KINDS = ("gauss", "lattice", "dup", "same", "line")


def make_cloud(kind, n, seed):
    """(n, 3) fp32.  gauss: tie-free in practice; lattice: small integers, full of exact ties and repeats; dup: half the points
    are copies of the other half; same: one position; line: collinear, equally spaced"""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, 3)).astype(np.float32)
    if kind == "lattice":
        return rng.integers(-4, 5, size=(n, 3)).astype(np.float32)
    if kind == "dup":
        half = rng.standard_normal(((n + 1) // 2, 3)).astype(np.float32)
        return np.concatenate([half, half])[:n][rng.permutation(n)]
    if kind == "same":
        return np.tile(rng.standard_normal((1, 3)).astype(np.float32), (n, 1))
    if kind == "line":
        step = np.array([1.0, -2.0, 0.5], dtype=np.float32)
        return (rng.permutation(n).astype(np.float32)[:, None] * step[None, :]).astype(np.float32)
    raise ValueError(kind)
