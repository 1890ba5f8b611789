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


# ---- worst-case candidate orders and the ends of the served range (tests/test_gpu_knn_edges.py) ------------------------------------
ORIGIN = np.zeros((1, 3), dtype=np.float32)


def ascending(m, seed):
    """the gauss cloud of (m, seed) in ascending fp32 distance (dist2) from the origin: a query near the origin meets its neighbours
    first and accepts next to nothing afterwards"""
    pts = make_cloud("gauss", m, seed)
    return np.ascontiguousarray(pts[np.argsort(dist2(ORIGIN, pts)[0], kind="stable")])


def descending(m, seed):
    """ascending's reverse: for a query near the origin almost every candidate is nearer than everything before it, so it enters the
    list at its head, whatever the capacity"""
    return np.ascontiguousarray(ascending(m, seed)[::-1])


def near_origin(n, seed, radius=1e-3):
    """(n, 3) fp32 queries within `radius` of the origin (uniform in the inscribed cube)"""
    side = radius / np.sqrt(3.0)
    return np.random.default_rng(seed).uniform(-side, side, size=(n, 3)).astype(np.float32)


def shells(m):
    """the innermost m points of the integer lattice [-6, 6]^3 (x fastest), stable-sorted by descending squared radius: from a lattice
    query every distance is an exact integer, and from the origin they never increase and come in long runs of equal values, each run
    in ascending lattice order"""
    c = grid(13, 13, 13) - np.float32(6.0)
    r2 = (c.astype(np.int64) ** 2).sum(1)
    order = np.argsort(-r2, kind="stable")
    assert 1 <= m <= c.shape[0]
    return np.ascontiguousarray(c[order[c.shape[0] - m:]])


def improvements(d, kcap):
    """d (m,) or (n, m) distances in candidate order -> per row the number of candidates STRICTLY below the kcap-th smallest of the
    candidates before them (+inf while fewer than kcap came before): the insertions a list of capacity kcap performs, which is the
    deferred queue's traffic under an exact threshold.  A stale threshold can only let more through.  An excluded candidate is +inf."""
    rows = np.atleast_2d(np.asarray(d))
    best = np.full((rows.shape[0], kcap), np.inf, dtype=np.float64)
    count = np.zeros(rows.shape[0], dtype=np.int64)
    for j in range(rows.shape[1]):
        col = rows[:, j].astype(np.float64)
        count += col < best[:, -1]
        best = np.sort(np.concatenate([best, col[:, None]], axis=1), axis=1)[:, :kcap]
    return count if np.ndim(d) == 2 else int(count[0])


ORDER_SLOTS = ("hot everywhere", "cold everywhere", "even lanes hot", "lanes 0-31 hot", "lane 37 of wave 1 hot")
STAND_OFF = np.float32(8.0)


def order_batch(m=1025, n=320, seed=11):
    """The candidate-order cases as one batch of five slots -> (query (5, n, 3), cloud (5, m, 3), hot (5, n) bool).  Query i of a slot
    is lane i % 64 of wave i // 64.  A hot query lies within 1e-3 of the origin and meets `descending`: every candidate improves its
    list.  Slot 1 meets `ascending` with the same queries: cold.  An ordinary query is a gauss point scaled by STAND_OFF = 8: from 8
    sigma away the descending radial order is nearly a shuffle (a unit-scale gauss query sees its distances fall with the radius too and
    improves 540 times of 1025 at capacity 32; at 8 sigma 155 times), which is what makes its lane idle beside a hot one."""
    desc, asc = descending(m, seed), ascending(m, seed)
    near = near_origin(n, seed + 1)
    far = make_cloud("gauss", n, seed + 2) * STAND_OFF
    lane = np.arange(n)
    hot = np.stack([np.ones(n, bool), np.zeros(n, bool), lane % 2 == 0, lane % 64 < 32, lane == 64 + 37])
    query = np.where(hot[:, :, None] | (np.arange(5) == 1)[:, None, None], near[None], far[None])
    return query, np.stack([desc, asc, desc, desc, desc]), hot


def launch_batch(B=32769, n=2, m=5, seed=7):
    """(query (B, n, 3), cloud (B, m, 3)) of small integers: more slots than one launch takes, full of ties"""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, size=(B, n, 3)).astype(np.float32), rng.integers(-4, 5, size=(B, m, 3)).astype(np.float32)


def poison(query, cloud, launch=32768):
    """copies with one NaN in a query of the last slot of the first launch and one in the cloud of the first slot of the second"""
    q, c = query.copy(), cloud.copy()
    q[launch - 1, -1, 1] = np.nan
    c[launch, 0, 2] = np.nan
    return q, c


def longest_run(row):
    """the length of the longest run of equal neighbouring values"""
    edges = np.flatnonzero(np.diff(row) != 0)
    return int(np.diff(np.concatenate([[-1], edges, [len(row) - 1]])).max())


def make_range_cloud(kind, n, seed):
    """(n, 3) fp32 at the ends of the served range.  tiny: gauss x 2^-70 (exact), whose squared distances are fp32 subnormals with a
    handful of significant bits -- gradual underflow decides the order, and ties abound; huge: uniform in +-2^61 with both bounds
    present in every axis of the first two points, so the largest distance is 3 * 2^124; wide: per-coordinate magnitudes 2^-60 .. 2^60
    with random signs"""
    rng = np.random.default_rng(seed)
    if kind == "tiny":
        return make_cloud("gauss", n, seed) * np.float32(2.0 ** -70)
    if kind == "huge":
        p = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32) * LIMIT
        p[0], p[1] = LIMIT, -LIMIT
        return p
    if kind == "wide":
        mag = np.exp2(rng.uniform(-60.0, 60.0, size=(n, 3)))
        return (mag * rng.choice([-1.0, 1.0], size=(n, 3))).astype(np.float32)
    raise ValueError(kind)


SUBNORMAL = np.float32(2.0 ** -126)


def subnormal_share(d):
    """the share of distances that are positive fp32 subnormals"""
    return float(((d > 0) & (d < SUBNORMAL)).mean())


# ---- mutated restatements: what the inputs above must tell apart from the contract (tests/test_knn_ref_cpu.py) ---------------------
def knn_highest_index_first(query, cloud, k, exclude_same_index=False):
    """the tie rule the wrong way round: among equal distances the HIGHEST index first"""
    d = dist2(np.ascontiguousarray(query, dtype=np.float32), np.ascontiguousarray(cloud, dtype=np.float32))
    if exclude_same_index:
        same = np.arange(min(d.shape))
        d[same, same] = np.inf
    back = np.ascontiguousarray(d[:, ::-1])
    order = np.argsort(back, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(back, order, axis=1), (d.shape[1] - 1 - order).astype(np.int32), 0


def flush(a):
    """fp32 with every subnormal replaced by a zero of its sign"""
    return np.where(np.abs(a) < SUBNORMAL, np.copysign(np.float32(0.0), a), a).astype(np.float32)


def dist2_flushed(query, cloud):
    """dist2 on hardware that flushes subnormal results to zero: every product and sum flushed"""
    dx = cloud[None, :, 0] - query[:, None, 0]
    dy = cloud[None, :, 1] - query[:, None, 1]
    dz = cloud[None, :, 2] - query[:, None, 2]
    return flush(flush(flush(dx * dx) + flush(dy * dy)) + flush(dz * dz))


def knn_flushed(query, cloud, k, exclude_same_index=False):
    d = dist2_flushed(np.ascontiguousarray(query, dtype=np.float32), np.ascontiguousarray(cloud, dtype=np.float32))
    if exclude_same_index:
        same = np.arange(min(d.shape))
        d[same, same] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order.astype(np.int32), 0


def status_at_slot_mod(status, launch=32768):
    """the statuses a kernel would leave that wrote slot b's at b mod `launch` (a second launch that forgot its first slot), over a
    buffer that held 0: the later write wins"""
    out = np.zeros_like(status)
    for b in range(status.shape[0]):
        out[b % launch] = status[b]
    return out
