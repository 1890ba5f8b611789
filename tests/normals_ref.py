"""Numpy restatement of dpf_normals (include/dpf_hip.h: the point-cloud normals block), in float64 with the operation order written
out.  Every function works on N neighbourhoods at once; every arithmetic step is one numpy array operation, so it rounds on its own.

    valid:      every one of the k indices in [0, m) and every gathered coordinate finite and at most 2^61 in magnitude; a point that
                is not valid gets flag 1 and NaN in every floating output
    centroid:   c_a = (p_0,a + p_1,a + ... + p_k-1,a) / k, added in ascending s, one division by (double) k
    covariance: C_ab = sum_s (p_s,a - c_a) * (p_s,b - c_b), each product rounded on its own, added in ascending s from the s = 0
                term; no division; stored xx, xy, xz, yy, yz, zz
    Jacobi:     SWEEPS sweeps over (0, 1), (0, 2), (1, 2); a rotation is skipped where the off-diagonal entry is exactly 0; else
                theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with sgn(0) = +1,
                c = 1 / sqrt(t^2 + 1), s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and with r the third index
                a_rp, a_rq = c a_rp - s a_rq, s a_rp + c a_rq;  the columns p, q of V (initially the identity) turn the same way
    order:      a stable three-element compare network (0, 1), (1, 2), (0, 1) on the diagonal, swapping only where the left value is
                strictly greater: the lower column goes first among equals; the normal is the column of the smallest eigenvalue
    unit:       divided once by sqrt((x^2 + y^2) + z^2)
    sign:       canonical -- the component of largest magnitude is positive, the lowest axis among equal magnitudes; with a viewpoint w
                whose three coordinates are finite, t = ((n_x (w_x - c_x)) + n_y (w_y - c_y)) + n_z (w_z - c_z) and t < 0 flips it."""
import numpy as np

SWEEPS = 6
MIN_K, MAX_K = 3, 32
LIMIT = 2.0 ** 61
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                                                    # (p, q, the third index)
SLOT = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}                    # cov's order: xx, xy, xz, yy, yz, zz


def covariance(pts):
    """pts (N, k, 3), any float dtype -> (centroid (N, 3), cov (N, 6)) float64"""
    p = np.asarray(pts).astype(np.float64)
    k = p.shape[1]
    total = p[:, 0].copy()
    for s in range(1, k):
        total = total + p[:, s]
    centroid = total / np.float64(k)
    d = p - centroid[:, None, :]
    cov = np.empty((p.shape[0], 6), dtype=np.float64)
    for (a, b), slot in SLOT.items():
        acc = d[:, 0, a] * d[:, 0, b]
        for s in range(1, k):
            acc = acc + d[:, s, a] * d[:, s, b]
        cov[:, slot] = acc
    return centroid, cov


def full(cov):
    """cov (N, 6) -> the symmetric matrices (N, 3, 3)"""
    m = np.empty(cov.shape[:-1] + (3, 3), dtype=np.float64)
    for (a, b), slot in SLOT.items():
        m[..., a, b] = m[..., b, a] = cov[..., slot]
    return m


def jacobi(cov, sweeps=SWEEPS):
    """cov (N, 6) -> (diagonal (N, 3), V (N, 3, 3), the largest |off-diagonal| left (N,)): unsorted"""
    a = full(cov)
    n = a.shape[0]
    v = np.zeros((n, 3, 3), dtype=np.float64)
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                apq = a[:, p, q].copy()
                go = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                root = np.sqrt(theta * theta + one)
                t = np.where(theta >= 0.0, one, -one) / (np.abs(theta) + root)
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                app, aqq = a[:, p, p] - h, a[:, q, q] + h
                arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                nrp, nrq = c * arp - s * arq, s * arp + c * arq
                a[:, p, p] = np.where(go, app, a[:, p, p])
                a[:, q, q] = np.where(go, aqq, a[:, q, q])
                a[:, p, q] = a[:, q, p] = np.where(go, 0.0, apq)
                a[:, r, p] = a[:, p, r] = np.where(go, nrp, arp)
                a[:, r, q] = a[:, q, r] = np.where(go, nrq, arq)
                for row in range(3):
                    vp, vq = v[:, row, p].copy(), v[:, row, q].copy()
                    v[:, row, p] = np.where(go, c * vp - s * vq, vp)
                    v[:, row, q] = np.where(go, s * vp + c * vq, vq)
    off = np.maximum(np.maximum(np.abs(a[:, 0, 1]), np.abs(a[:, 0, 2])), np.abs(a[:, 1, 2]))
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v, off


def sort3(lam, v):
    """the stable compare network: ascending eigenvalues (N, 3) and their columns (N, 3, 3)"""
    lam, v = lam.copy(), v.copy()
    for i, j in ((0, 1), (1, 2), (0, 1)):
        swap = lam[:, i] > lam[:, j]
        li, lj = lam[:, i].copy(), lam[:, j].copy()
        lam[:, i], lam[:, j] = np.where(swap, lj, li), np.where(swap, li, lj)
        vi, vj = v[:, :, i].copy(), v[:, :, j].copy()
        v[:, :, i], v[:, :, j] = np.where(swap[:, None], vj, vi), np.where(swap[:, None], vi, vj)
    return lam, v


def unit(vec):
    x, y, z = vec[:, 0], vec[:, 1], vec[:, 2]
    norm = np.sqrt((x * x + y * y) + z * z)
    return vec / norm[:, None]


def canonical_flip(vec):
    """(N,) bool: True where the canonical sign is the opposite of vec's"""
    ax, ay, az = np.abs(vec[:, 0]), np.abs(vec[:, 1]), np.abs(vec[:, 2])
    pick, mag = vec[:, 0], ax
    take = ay > mag
    pick, mag = np.where(take, vec[:, 1], pick), np.where(take, ay, mag)
    take = az > mag
    pick = np.where(take, vec[:, 2], pick)
    return pick < 0.0


def canonical(vec):
    return np.where(canonical_flip(vec)[:, None], -vec, vec)


def orient(vec, centroid, viewpoint):
    """vec (N, 3) canonical, centroid (N, 3), viewpoint (3,) fp32, one for all, or (N, 3), one a row, or None -> the oriented normals"""
    if viewpoint is None:
        return vec
    w = np.asarray(viewpoint, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = (vec[:, 0] * (w[..., 0] - centroid[:, 0]) + vec[:, 1] * (w[..., 1] - centroid[:, 1])) + vec[:, 2] * (w[..., 2] - centroid[:, 2])
    flip = np.isfinite(w).all(-1) & (t < 0.0)                                                # (a non-finite viewpoint is no viewpoint)
    return np.where(flip[:, None], -vec, vec)


def eigen(cov, sweeps=SWEEPS):
    """cov (N, 6) -> (the unit eigenvector of the smallest eigenvalue, canonical sign (N, 3); eigenvalues ascending (N, 3))"""
    lam, v, _ = jacobi(cov, sweeps)
    lam, v = sort3(lam, v)
    return canonical(unit(v[:, :, 0])), lam


def flags(cloud, index):
    """cloud (m, 3) fp32, index (n, k) -> (n,) int32: 1 where an index is out of [0, m) or a gathered coordinate is out of range"""
    m = cloud.shape[0]
    inside = (index >= 0) & (index < m)
    safe = np.where(inside, index, 0)
    with np.errstate(invalid="ignore"):
        good = (np.abs(cloud[safe]) <= np.float32(LIMIT)).all(-1)                            # (NaN fails the comparison)
    return (~(inside & good).all(-1)).astype(np.int32)


def normals(cloud, index, viewpoint=None, sweeps=SWEEPS):
    """one slot: cloud (m, 3) fp32, index (n, k) integers, viewpoint (3,) or None ->
    (normal (n, 3), eigenvalues (n, 3), cov (n, 6), all float64; flag (n,) int32)"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32)
    index = np.asarray(index)
    n, k = index.shape
    assert MIN_K <= k <= MAX_K
    flag = flags(cloud, index)
    ok = flag == 0
    normal, lam, cov = (np.full((n, c), np.nan) for c in (3, 3, 6))
    if ok.any():
        centroid, cv = covariance(cloud[index[ok]])
        vec, ev = eigen(cv, sweeps)
        normal[ok], lam[ok], cov[ok] = orient(vec, centroid, viewpoint), ev, cv
    return normal, lam, cov, flag


def normals_batch(clouds, index, viewpoint=None):
    """clouds (B, m, 3), index (B, n, k), viewpoint None, (3,) or (B, 3) -> the four outputs stacked over the slots"""
    out = []
    for b in range(index.shape[0]):
        w = None if viewpoint is None else (viewpoint if np.ndim(viewpoint) == 1 else viewpoint[b])
        out.append(normals(clouds[b], index[b], w))
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def surface_variation(lam):
    total = (lam[..., 0] + lam[..., 1]) + lam[..., 2]
    with np.errstate(all="ignore"):
        return np.where(total == 0.0, 0.0, lam[..., 0] / total)


# ---- the four bounds (each 2^-46 in the tests), measured against numpy.linalg.eigh of the same covariance ---------------------------
def measures(cov, vec, lam):
    """cov (N, 6), vec (N, 3), lam (N, 3) -> the worst (residual / lmax, | |v| - 1 |, eigenvalue error / lmax, sin(angle) * gap /
    lmax over the neighbourhoods whose gap exceeds 2^-20 lmax) and the number of neighbourhoods the fourth was measured on.
    A neighbourhood whose covariance is all zero has lmax = 0: its residual and eigenvalues must be exactly 0, and it counts as 0."""
    a = full(cov)
    w, u = np.linalg.eigh(a)
    lmax = np.maximum(np.abs(w).max(-1), np.abs(lam).max(-1))
    scale = np.where(lmax > 0.0, lmax, 1.0)
    res = np.linalg.norm(np.einsum("nab,nb->na", a, vec) - lam[:, :1] * vec, axis=1)
    ev = np.abs(lam - w).max(-1)
    assert (res[lmax == 0.0] == 0.0).all() and (ev[lmax == 0.0] == 0.0).all()
    norm = np.abs(np.sqrt((vec * vec).sum(-1)) - 1.0)
    gap = w[:, 1] - w[:, 0]
    clear = gap > 2.0 ** -20 * lmax
    sin = np.linalg.norm(np.cross(vec, u[:, :, 0]), axis=1)
    angle = (sin * gap / scale)[clear]
    return (res / scale).max(), norm.max(), (ev / scale).max(), (angle.max() if clear.any() else 0.0), int(clear.sum())


# ---- the neighbourhoods and clouds of the tests, from a seed -------------------------------------------------------------------------
KINDS = ("gauss", "squashed", "planar", "collinear", "offset", "lattice", "equal", "scaled")
SMALL_KINDS = ("tiny", "denormal")                  # gauss x 2^-70: the covariance near 2^-140; x 2^-135: the fp32 coordinates subnormal
SMALL_SCALE = {"tiny": 2.0 ** -70, "denormal": 2.0 ** -135}


def neighbourhoods(kind, count, k, seed):
    """(count, k, 3) fp32: the eight kinds the sweep count was chosen on, and the two small scales"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((count, k, 3))
    if kind == "gauss":
        p = g
    elif kind == "squashed":
        p = g * np.array([1.0, 1.0, 1e-3])
    elif kind == "planar":                                                                    # a random plane through a random point
        e = np.linalg.qr(rng.standard_normal((count, 3, 3)))[0]
        p = g[:, :, :1] * e[:, None, :, 0] + g[:, :, 1:2] * e[:, None, :, 1] + rng.standard_normal((count, 1, 3))
    elif kind == "collinear":
        p = g[:, :, :1] * rng.standard_normal((count, 1, 3)) + rng.standard_normal((count, 1, 3))
    elif kind == "offset":
        p = 100.0 + 1e-3 * g
    elif kind == "lattice":
        p = rng.integers(-4, 5, size=(count, k, 3)).astype(np.float64)
    elif kind == "equal":
        p = np.repeat(g[:, :1], k, axis=1)
    elif kind == "scaled":
        p = 1e18 * g
    elif kind in SMALL_KINDS:
        p = SMALL_SCALE[kind] * g
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def make_cloud(kind, n, seed):
    """(n, 3) fp32 clouds for the device tests.  scaled: 1e18 g with g cut at +-2.25, so that every coordinate stays inside the 2^61 =
    2.3e18 that dpf_knn and dpf_normals serve (a plain 1e18 g would have a slot refused at its first 2.4-sigma coordinate); tiny,
    denormal: g x 2^-70 and g x 2^-135 (SMALL_SCALE) -- the second's fp32 coordinates are subnormal"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    if kind == "gauss":
        p = g
    elif kind == "offset":
        p = 100.0 + 1e-3 * g
    elif kind == "scaled":
        p = 1e18 * np.clip(g, -2.25, 2.25)
    elif kind == "same":
        p = np.tile(g[:1], (n, 1))
    elif kind == "squashed":
        p = g * np.array([1.0, 1.0, 1e-3])
    elif kind == "lattice":
        p = rng.integers(-3, 4, size=(n, 3)).astype(np.float64)
    elif kind in SMALL_KINDS:
        p = SMALL_SCALE[kind] * g
    else:
        raise ValueError(kind)
    return p.astype(np.float32)
