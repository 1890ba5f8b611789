"""Numpy restatement of dpf_knn (include/dpf_hip.h: the k-nearest-neighbours block), in fp32 with the operation order written out:

    d(i, j) = (dx*dx + dy*dy) + dz*dz,  dx = c_j.x - q_i.x (the same per axis), every fp32 operation rounded on its own;
    eligible: every j in [0, m), without j == i under exclude_same_index (by index, never by distance);
    result: the k eligible candidates with the smallest key (d, j), ascending.

The order is a STABLE sort of a row of distances: among equal distances the lowest index comes first, in the list and at the cut.
The excluded candidate is given +inf, which no real distance reaches (coordinates are bounded by 2^61, so d <= 3 * 2^124) and k never
reaches (k <= m - 1).  A slot with a coordinate that is not finite or exceeds 2^61 in magnitude, in either set, is refused: dist NaN,
index -1, status -1.  The spacing statistic and the gradient of sum(g * dist) are restated in float64."""
import numpy as np

REFUSED = -1
LIMIT = np.float32(2.0 ** 61)


def dist2(query, cloud):
    """(n, m) fp32 squared distances, each operation an fp32 array operation of its own"""
    dx = cloud[None, :, 0] - query[:, None, 0]
    dy = cloud[None, :, 1] - query[:, None, 1]
    dz = cloud[None, :, 2] - query[:, None, 2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    s = xx + yy
    d = s + zz
    assert d.dtype == np.float32
    return d


def in_range(pts):
    with np.errstate(invalid="ignore"):
        return bool((np.abs(pts) <= LIMIT).all())                                            # (NaN fails the comparison)


def knn(query, cloud, k, exclude_same_index=False):
    """query (n, 3), cloud (m, 3) -> (dist (n, k) fp32, index (n, k) int32, status)"""
    query = np.ascontiguousarray(query, dtype=np.float32)
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    n, m = query.shape[0], cloud.shape[0]
    assert query.shape == (n, 3) and cloud.shape == (m, 3) and 1 <= k <= (m - 1 if exclude_same_index else m)
    if not (in_range(query) and in_range(cloud)):
        return np.full((n, k), np.nan, dtype=np.float32), np.full((n, k), -1, dtype=np.int32), REFUSED
    d = dist2(query, cloud)
    assert np.isfinite(d).all()
    if exclude_same_index:
        same = np.arange(min(n, m))
        d[same, same] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    dist = np.take_along_axis(d, order, axis=1)
    assert np.isfinite(dist).all()
    return dist, order.astype(np.int32), 0


def knn_batch(query, cloud, k, exclude_same_index=False):
    """query (B, n, 3), cloud (B, m, 3) -> dist (B, n, k) fp32, index (B, n, k) int32, status (B,) int32"""
    out = [knn(query[b], cloud[b], k, exclude_same_index) for b in range(query.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32))


def brute_force(query, cloud, k, exclude_same_index=False):
    """the same selection from float64 distances by an explicit sort of (d, j) pairs: what the restatement is checked against"""
    q, c = np.asarray(query, dtype=np.float64), np.asarray(cloud, dtype=np.float64)
    dist = np.empty((q.shape[0], k), dtype=np.float64)
    index = np.empty((q.shape[0], k), dtype=np.int32)
    for i in range(q.shape[0]):
        pairs = sorted((float(((c[j] - q[i]) ** 2).sum()), j) for j in range(c.shape[0]) if not (exclude_same_index and j == i))[:k]
        dist[i] = [p[0] for p in pairs]
        index[i] = [p[1] for p in pairs]
    return dist, index


def spacing(cloud, k=1):
    """(mean, cv) of the distance to the k-th nearest other point, float64 on the fp32 squared distances"""
    s = np.sqrt(knn(cloud, cloud, k, True)[0][:, k - 1].astype(np.float64))
    mean = s.mean()
    return mean, np.sqrt(((s - mean) ** 2).mean()) / mean


def grad(query, cloud, index, g):
    """float64 gradients of sum(g * dist) with the indices constant, and the sums of the absolute values of the terms that make up
    each entry (what the rounding bound of an fp32 evaluation scales with): grad_query, grad_cloud, abs_query, abs_cloud"""
    q, c, g = np.asarray(query, dtype=np.float64), np.asarray(cloud, dtype=np.float64), np.asarray(g, dtype=np.float64)
    term = 2.0 * g[:, :, None] * (q[:, None, :] - c[index])                                  # (n, k, 3)
    mag = 2.0 * np.abs(g)[:, :, None] * (np.abs(q)[:, None, :] + np.abs(c[index]))
    gq, aq = term.sum(1), mag.sum(1)
    gc, ac = np.zeros_like(c), np.zeros_like(c)
    np.add.at(gc, index.reshape(-1), -term.reshape(-1, 3))
    np.add.at(ac, index.reshape(-1), mag.reshape(-1, 3))
    return gq, gc, aq, ac


# ---- the clouds of the tests, from a seed ------------------------------------------------------------------------------------
def make_cloud(kind, n, seed):
    """(n, 3) fp32.  gauss: tie-free in practice; lattice: small integers, every operation exact, full of ties and repeats; dup: half
    the points are copies of the other half; same: one position"""
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
    raise ValueError(kind)


def grid(a, b, c):
    """the a x b x c unit lattice, (a * b * c, 3) fp32, x fastest"""
    z, y, x = np.meshgrid(np.arange(c), np.arange(b), np.arange(a), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
