"""Numpy restatement of the sliced-Wasserstein contract (include/dpf_hip.h: the dpf_swd_* block), with the operation order written
out:

    p(l, i) = ((x * tx + y * ty) + z * tz) + 0.0f      every fp32 operation an array operation of its own; -0 becomes +0
    order(l, .) = the permutation sorting the keys (p, i) ascending: np.lexsort on (index, value)
    sorted(l, r) = p(l, order(l, r))
    sumsq = sum_l sum_r (double) fl32(sa - sb)^2       float64
    grad_a(i, axis) = fl32(grad_cost * (2 / (L n)) * sum_l (double) g(l, i) * (double) theta(l, axis)),  g(l, i) = fl32(sa - sb) at
                      the rank of point i of a in direction l; grad_b the same with the sign reversed at the ranks of b's points

A cloud with a non-finite coordinate, direction component or projection is refused: sorted NaN, order -1, status -1."""
import numpy as np

REFUSED = -1


def project(pts, dirs):
    """(L, n) fp32 projections of pts (n, 3) on dirs (L, 3)"""
    pts = np.asarray(pts, dtype=np.float32)
    dirs = np.asarray(dirs, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        xx = pts[None, :, 0] * dirs[:, None, 0]
        yy = pts[None, :, 1] * dirs[:, None, 1]
        zz = pts[None, :, 2] * dirs[:, None, 2]
        s = xx + yy
        s = s + zz
        s = s + np.float32(0.0)
    assert s.dtype == np.float32
    return s


def tables(pts, dirs):
    """pts (n, 3), dirs (L, 3) -> (sorted (L, n) fp32, order (L, n) int32, status)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    n, L = pts.shape[0], dirs.shape[0]
    p = project(pts, dirs)
    if not (np.isfinite(pts).all() and np.isfinite(dirs).all() and np.isfinite(p).all()):
        return np.full((L, n), np.nan, dtype=np.float32), np.full((L, n), -1, dtype=np.int32), REFUSED
    idx = np.arange(n)
    order = np.stack([np.lexsort((idx, p[l])) for l in range(L)]).astype(np.int32)
    return np.take_along_axis(p, order.astype(np.int64), axis=1), order, 0


def tables_batch(clouds, dirs):
    """clouds (B, n, 3) -> sorted (B, L, n), order (B, L, n), status (B,)"""
    out = [tables(c, dirs) for c in clouds]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


def sumsq(sa, sb, refused=False):
    """float64 sum over (l, r) of the squared fp32 differences of two sorted tables (L, n)"""
    if refused:
        return np.float64(np.nan)
    d = sa.astype(np.float32) - sb.astype(np.float32)
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    return (d * d).sum(dtype=np.float64)


def distance(ss, L, n):
    """the fp32 distance from a float64 sum: one rounding"""
    return np.float32(np.float64(ss) / np.float64(L * n))


def grad(ta, tb, dirs, grad_cost):
    """two tables (sorted, order, status) of one pair -> (grad_a, grad_b, bound_a, bound_b): the (n, 3) fp32 gradients and the
    (n, 3) float64 bound terms sum_l |g * theta| at a's and at b's points"""
    (sa, oa, sta), (sb, ob, stb) = ta, tb
    L, n = sa.shape
    zero = np.zeros((n, 3), dtype=np.float32)
    if sta != 0 or stb != 0:
        return zero, zero.copy(), np.zeros((n, 3)), np.zeros((n, 3))
    g = sa - sb
    assert g.dtype == np.float32
    g = g.astype(np.float64)
    th = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    scale = np.float64(np.float32(grad_cost)) * (2.0 / (np.float64(L) * n))
    out = []
    for o, sign in ((oa, 1.0), (ob, -1.0)):
        at = np.empty((L, n), dtype=np.float64)                 # g at the points, not at the ranks
        np.put_along_axis(at, o.astype(np.int64), g, axis=1)
        s = np.einsum("li,la->ia", at, th)
        bound = np.einsum("li,la->ia", np.abs(at), np.abs(th))
        out.append(((sign * scale * s).astype(np.float32), bound))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- the clouds and directions of the tests, from a seed ---------------------------------------------------------------------
KINDS = ("gauss", "same", "lattice", "sorted", "reverse", "negzero", "wide")


def make_dirs(kind, L, seed=0):
    """(L, 3) fp32.  gauss: unit Gaussian rows; axis: the coordinate axes and their negatives in turn; dyadic: small multiples of
    1/4 (exact products with lattice clouds); negzero: components among -1, -0, +0, 1"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "gauss":
        d = rng.standard_normal((L, 3))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if kind == "axis":
        eye = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
        return np.ascontiguousarray(eye[np.arange(L) % 6]) + np.float32(0.0)
    if kind == "dyadic":
        d = rng.integers(-8, 9, size=(L, 3)).astype(np.float32) / np.float32(4.0)
        d[(d == 0).all(axis=1), 0] = 1.0
        return d
    if kind == "negzero":
        return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=(L, 3))
    raise ValueError(kind)


def make_cloud(kind, n, seed):
    """(n, 3) fp32.  gauss: tie-free in practice; same: one position; lattice: small integers, whole runs of ties under axis
    directions; sorted / reverse: ascending / descending along every axis; negzero: zeros of both signs and +-1, so products and sums
    of -0 arise; wide: magnitudes spanning 2^-60 .. 2^60"""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, 3)).astype(np.float32)
    if kind == "same":
        return np.tile(rng.standard_normal((1, 3)).astype(np.float32), (n, 1))
    if kind == "lattice":
        return rng.integers(-4, 5, size=(n, 3)).astype(np.float32)
    if kind == "sorted":
        return np.sort(rng.standard_normal((n, 3)).astype(np.float32), axis=0)
    if kind == "reverse":
        return np.ascontiguousarray(np.sort(rng.standard_normal((n, 3)).astype(np.float32), axis=0)[::-1])
    if kind == "negzero":
        return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=(n, 3))
    if kind == "wide":
        mag = np.exp2(rng.uniform(-60.0, 60.0, size=(n, 3)))
        return (mag * rng.choice([-1.0, 1.0], size=(n, 3))).astype(np.float32)
    raise ValueError(kind)
