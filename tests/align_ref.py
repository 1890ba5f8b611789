"""Numpy restatement of dpf_rigid_fit and dpf_icp (include/dpf_hip.h: the rigid-alignment block), with the operation order written out.
One slot at a time; every array step is one numpy operation and every scalar step one Python float operation, so each rounds on its own.

    transform:  y_a = fp32(((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) * s + t_a) in float64, one rounding to fp32; a y that is not finite or
                exceeds 2^61 has no match (index -1, dist +inf, weight 0)
    match:      d = (dx*dx + dy*dy) + dz*dz, dx = c_j.x - y.x, fp32; the smallest (d, j), the lowest index among ties; with a trim
                d > max_dist2 gives index -1, weight 0
    sums:       eighteen float64 quantities over p' = p - a, q' = q - c (the pivots: point 0 of either set); a block is 256 consecutive
                points, summed by the tree  for stride = 128 .. 1: x[i] += x[i + stride];  the blocks are added in ascending order
    solve:      Horn's 4 x 4 matrix, SWEEPS cyclic Jacobi sweeps over (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) with dpf_normals' rotation,
                the column of the largest diagonal entry as a unit quaternion; degenerate slots keep their transform
    icp:        iters times (match, solve from the ORIGINAL source points), then one more match under the returned transform"""
import math

import numpy as np

SWEEPS = 7                              # shipped: FLOOR_SWEEPS + 2
FLOOR_SWEEPS = 5                        # the smallest count at which every kind reaches its rounding floor (measured: test_align_ref_cpu.py)
BLOCK = 256
NSUMS = 18
LIMIT = 2.0 ** 30                       # a coordinate, an init entry or a weight above it refuses the slot
YLIMIT = 2.0 ** 61                      # a transformed point above it has no match
MIN_INLIERS = 3
DEGENERATE, REFUSED = 1, -1
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# The bound on R, t and s between two float64 solutions of one problem (here: against an SVD solution; on the device: the kernel's
# solve against this file's solve of the kernel's own sums).  Relative: |dR| <= BOUND, |ds| <= BOUND * s, |dt| <= BOUND * (|t| + s *
# the source's largest coordinate + the target's).  Measured in test_align_ref_cpu.py: the worst deviation over the kinds there is
# 8.7e-14 (planar: a rank-2 M), times 8 for the device's own sqrt and division sequences; never looser than 2^-40.
WORST_MEASURED = 8.8e-14
ALIGN_BOUND = min(8 * WORST_MEASURED, 2.0 ** -40)

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float64)            # R row-major, t, s


def pack(R, t, s=1.0):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3), [np.float64(s)]])


def unpack(T):
    T = np.asarray(T, dtype=np.float64)
    return T[:9].reshape(3, 3), T[9:12], T[12]


def transform_points(T, p):
    """T (13,) float64, p (n, 3) fp32 -> (y (n, 3) fp32, usable (n,) bool)"""
    T = np.asarray(T, dtype=np.float64)
    x = np.asarray(p, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        cols = [(((T[3 * a] * x[:, 0] + T[3 * a + 1] * x[:, 1]) + T[3 * a + 2] * x[:, 2]) * T[12] + T[9 + a]).astype(np.float32)
                for a in range(3)]
        y = np.stack(cols, axis=1)
        usable = (np.abs(y) <= np.float32(YLIMIT)).all(-1)                                   # (NaN fails the comparison)
    return y, usable


def distances(y, c):
    """(n, m) fp32: dpf_nndistance's bits"""
    with np.errstate(all="ignore"):
        dx = c[None, :, 0] - y[:, None, 0]
        dy = c[None, :, 1] - y[:, None, 1]
        dz = c[None, :, 2] - y[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def match(src, dst, T, max_dist2=0.0, prev=None):
    """-> (index (n,) int32, dist (n,) fp32, weight (n,) float64, changed int)"""
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    y, usable = transform_points(T, src)
    y = np.where(usable[:, None], y, np.float32(0))
    d = distances(y, dst)
    index = np.argmin(d, axis=1).astype(np.int32)                                            # (the first of equal minima: the lowest index)
    dist = d[np.arange(src.shape[0]), index]
    index = np.where(usable, index, -1).astype(np.int32)
    dist = np.where(usable, dist, np.float32(np.inf)).astype(np.float32)
    md = np.float32(max_dist2)
    if md > 0 and md < np.inf:
        index = np.where(dist > md, -1, index).astype(np.int32)
    weight = (index >= 0).astype(np.float64)
    changed = src.shape[0] if prev is None else int((np.asarray(prev) != index).sum())
    return index, dist, weight, changed


def terms(p, q, w, last, a, c):
    """p, q (n, 3) fp32, w (n,) float64, last (n,) float64 or None (the fit's S_qq), the pivots -> (n, 18) float64"""
    pp = np.asarray(p, dtype=np.float32).astype(np.float64) - np.asarray(a, dtype=np.float32).astype(np.float64)
    qq = np.asarray(q, dtype=np.float32).astype(np.float64) - np.asarray(c, dtype=np.float32).astype(np.float64)
    t = np.zeros((pp.shape[0], NSUMS), dtype=np.float64)
    t[:, 0] = w
    for x in range(3):
        wp = w * pp[:, x]
        t[:, 1 + x] = wp
        t[:, 4 + x] = w * qq[:, x]
        for y in range(3):
            t[:, 7 + 3 * x + y] = wp * qq[:, y]
    t[:, 16] = w * ((pp[:, 0] * pp[:, 0] + pp[:, 1] * pp[:, 1]) + pp[:, 2] * pp[:, 2])
    t[:, 17] = w * ((qq[:, 0] * qq[:, 0] + qq[:, 1] * qq[:, 1]) + qq[:, 2] * qq[:, 2]) if last is None else w * last
    return t


def tree(x):
    """x (256, ...) -> the block's pairwise-tree sum"""
    x = np.array(x, dtype=np.float64)
    assert x.shape[0] == BLOCK
    stride = BLOCK // 2
    while stride >= 1:
        x[:stride] = x[:stride] + x[stride:2 * stride]
        stride //= 2
    return x[0]


def reduce_terms(t):
    """t (n, 18) -> (18,): trees over blocks of 256 (+0.0 past n), the block sums added in ascending order from block 0's"""
    n = t.shape[0]
    nblk = (n + BLOCK - 1) // BLOCK
    padded = np.zeros((nblk * BLOCK,) + t.shape[1:], dtype=np.float64)
    padded[:n] = t
    acc = tree(padded[:BLOCK])
    for blk in range(1, nblk):
        acc = acc + tree(padded[blk * BLOCK:(blk + 1) * BLOCK])
    return acc


def icp_sums(src, dst, index, dist, weight):
    """the eighteen sums of a match: points without one contribute +0.0"""
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    ok = index >= 0
    q = dst[np.where(ok, index, 0)]
    with np.errstate(all="ignore"):
        t = terms(src, q, weight, np.where(ok, dist, np.float32(0)).astype(np.float64), src[0], dst[0])
    t[~ok] = 0.0
    return reduce_terms(t)


def rotate(a, v, p, q):
    """one Jacobi rotation of the symmetric matrix a (lists of Python floats, both halves kept) and of the columns p, q of v"""
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    sq = theta * theta
    root = math.sqrt(sq + 1.0) if sq != math.inf else math.inf
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + root)
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    a[p][p] = a[p][p] - h
    a[q][q] = a[q][q] + h
    a[p][q] = a[q][p] = 0.0
    for r in range(len(a)):
        if r != p and r != q:
            x, y = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * x - s * y
            a[r][q] = a[q][r] = s * x + c * y
    for r in range(len(a)):
        x, y = v[r][p], v[r][q]
        v[r][p] = c * x - s * y
        v[r][q] = s * x + c * y


def horn(M):
    Mxx, Mxy, Mxz = M[0]
    Myx, Myy, Myz = M[1]
    Mzx, Mzy, Mzz = M[2]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (Mxx + Myy) + Mzz
    N[1][1] = (Mxx - Myy) - Mzz
    N[2][2] = (-Mxx + Myy) - Mzz
    N[3][3] = (-Mxx - Myy) + Mzz
    N[0][1] = N[1][0] = Myz - Mzy
    N[0][2] = N[2][0] = Mzx - Mxz
    N[0][3] = N[3][0] = Mxy - Myx
    N[1][2] = N[2][1] = Mxy + Myx
    N[1][3] = N[3][1] = Mzx + Mxz
    N[2][3] = N[3][2] = Myz + Mzy
    return N


def quaternion(N, sweeps=SWEEPS):
    """the unit eigenvector of the largest eigenvalue of N by fixed-sweep Jacobi, canonical sign; N is not changed"""
    a = [list(map(float, row)) for row in N]
    v = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            rotate(a, v, p, q)
    col = 0
    for c in range(1, 4):
        if a[c][c] > a[col][col]:
            col = c
    q = [v[r][col] for r in range(4)]
    norm = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [x / norm for x in q]
    pick, mag = q[0], abs(q[0])
    for x in q[1:]:
        if abs(x) > mag:
            pick, mag = x, abs(x)
    return [-x for x in q] if pick < 0.0 else q


def rotation(q):
    w, x, y, z = q
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    return [[((ww + xx) - yy) - zz, 2.0 * (xy - wz), 2.0 * (xz + wy)],
            [2.0 * (xy + wz), ((ww - xx) + yy) - zz, 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), ((ww - xx) - yy) + zz]]


def solve(S, inliers, a, c, with_scale=False, sweeps=SWEEPS):
    """S (18,) float64, the inlier count, the pivots (3,) fp32 -> (T (13,) or None where the slot is degenerate, the closed-form
    residual sum e of the fit -- meaningful where S[17] is S_qq)"""
    S = [float(x) for x in S]
    W = S[0]
    if inliers < MIN_INLIERS or not W > 0.0:
        return None, math.nan
    M = [[S[7 + 3 * x + y] - (S[1 + x] * S[4 + y]) / W for y in range(3)] for x in range(3)]
    v = S[16] - ((S[1] * S[1] + S[2] * S[2]) + S[3] * S[3]) / W
    vq = S[17] - ((S[4] * S[4] + S[5] * S[5]) + S[6] * S[6]) / W
    if with_scale and not v > 0.0:
        return None, math.nan
    R = rotation(quaternion(horn(M), sweeps))
    tr = None
    for x in range(3):
        row = (R[x][0] * M[0][x] + R[x][1] * M[1][x]) + R[x][2] * M[2][x]
        tr = row if tr is None else tr + row
    s = tr / v if with_scale else 1.0
    a = [float(np.float32(x)) for x in a]
    c = [float(np.float32(x)) for x in c]
    g = [a[x] + S[1 + x] / W for x in range(3)]
    t = [(c[x] + S[4 + x] / W) - s * ((R[x][0] * g[0] + R[x][1] * g[1]) + R[x][2] * g[2]) for x in range(3)]
    T = pack(R, t, s)
    if not np.isfinite(T).all():
        return None, math.nan
    e = ((s * s) * v + vq) - (2.0 * s) * tr
    return T, (e if e > 0.0 else 0.0)


def out_of_range(x):
    with np.errstate(invalid="ignore"):
        return not bool((np.abs(np.asarray(x)) <= LIMIT).all())


def rigid_fit(src, dst, weights=None, with_scale=False, sweeps=SWEEPS):
    """one slot -> dict(T (13,), rmse, sums (18,), status)"""
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    n = src.shape[0]
    w = np.ones(n, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    nan = np.full(13, np.nan)
    if out_of_range(src) or out_of_range(dst) or out_of_range(w) or (w < 0).any():
        return dict(T=nan, rmse=np.nan, sums=np.full(NSUMS, np.nan), status=REFUSED)
    S = reduce_terms(terms(src, dst, w, None, src[0], dst[0]))
    T, e = solve(S, int((w > 0).sum()), src[0], dst[0], with_scale, sweeps)
    if T is None:
        return dict(T=IDENTITY.copy(), rmse=np.nan, sums=S, status=DEGENERATE)
    return dict(T=T, rmse=math.sqrt(e / float(S[0])), sums=S, status=0)


def icp(src, dst, iters=30, max_dist2=0.0, with_scale=False, init=None, sweeps=SWEEPS):
    """one slot -> dict(T, index, dist, rmse (iters + 1,), inliers (iters + 1,), iterations, sums, status, changed (per match run))"""
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    n = src.shape[0]
    T = IDENTITY.copy() if init is None else np.asarray(init, dtype=np.float64).reshape(13).copy()
    rmse, inl = np.full(iters + 1, np.nan), np.zeros(iters + 1, dtype=np.int32)
    if out_of_range(src) or out_of_range(dst) or out_of_range(T):
        return dict(T=np.full(13, np.nan), index=np.full(n, -1, dtype=np.int32), dist=np.full(n, np.nan, dtype=np.float32), rmse=rmse,
                    inliers=inl, iterations=0, sums=np.full(NSUMS, np.nan), status=REFUSED, changed=[])
    status, iterations, done, prev, changes = 0, iters, False, None, []
    for k in range(iters + 1):
        if done:
            rmse[k], inl[k] = rmse[k - 1], inl[k - 1]
            continue
        index, dist, weight, changed = match(src, dst, T, max_dist2, prev)
        prev = index
        changes.append(changed)
        S = icp_sums(src, dst, index, dist, weight)
        inl[k] = int((weight > 0).sum())
        with np.errstate(all="ignore"):
            rmse[k] = np.sqrt(S[17] / S[0])
        if (k > 0 and changed == 0) or k == iters:
            done, iterations = True, k
            continue
        new, _ = solve(S, int(inl[k]), src[0], dst[0], with_scale, sweeps)
        if new is None:
            done, iterations, status = True, k, DEGENERATE
            continue
        T = new
    return dict(T=T, index=index, dist=dist, rmse=rmse, inliers=inl, iterations=iterations, sums=S, status=status, changed=changes)


def apply(T, p):
    """float64, plain: s R p + t"""
    R, t, s = unpack(T)
    return s * (np.asarray(p, dtype=np.float64) @ R.T) + t


# ---- the clouds of the tests, from a seed ---------------------------------------------------------------------------------------------
def rotation_about(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


FIT_KINDS = ("gauss", "offset", "small", "large", "planar", "reflection", "weighted", "scale")


def make_fit(kind, n, seed):
    """(src (n, 3) fp32, dst (n, 3) fp32, weights (n,) fp32 or None, with_scale): corresponding points, dst a noisy transformed src"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    R, t = random_rotation(rng), rng.standard_normal(3)
    noise, weights, with_scale, s = 0.05, None, False, 1.0
    if kind == "gauss":
        p = g
    elif kind == "offset":
        p, noise = 100.0 + 1e-3 * g, 5e-5
    elif kind == "small":
        p, t, noise = 1e-4 * g, 1e-4 * t, 5e-6
    elif kind == "large":
        p, t, noise = 1e4 * g, 1e4 * t, 500.0
    elif kind == "planar":
        p, noise = g * np.array([1.0, 1.0, 0.0]), 0.0                                        # rank-2 M
    elif kind == "reflection":                                                                # the unconstrained optimum is improper
        p, noise = g * np.array([1.0, 0.6, 0.05]), 0.0
        R = R @ np.diag([1.0, 1.0, -1.0])
    elif kind == "weighted":
        p, weights = g, rng.uniform(0.0, 2.0, n).astype(np.float32)
        weights[rng.permutation(n)[:n // 4]] = 0.0
    elif kind == "scale":
        p, with_scale, s = g, True, 1.7
    elif kind == "collinear":
        p, noise = np.outer(g[:, 0], rng.standard_normal(3)) + 0.5, 0.01
    else:
        raise ValueError(kind)
    q = s * (p @ R.T) + t + noise * rng.standard_normal((n, 3))
    return p.astype(np.float32), q.astype(np.float32), weights, with_scale


PAIR_KINDS = ("gauss", "offset", "lattice", "rotated", "scaled", "far")


def make_pair(kind, n, m, seed):
    """(src (n, 3) fp32, dst (m, 3) fp32) for the matching tests.  gauss: two independent clouds; offset: at 100 with 1e-3 of spread;
    lattice: integer coordinates in -2..2, full of equal distances and duplicated points; rotated: dst holds the source turned by 8
    degrees and shifted by 0.05 (its first min(n, m) points, point 0 in place and the rest in a seeded order); scaled: the same with
    a scale of 1.3; far: a third of the source at 1e3 from everything (for a trim)"""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((m, 3)).astype(np.float32)
    if kind == "offset":
        return (100.0 + 1e-3 * rng.standard_normal((n, 3))).astype(np.float32), (100.0 + 1e-3 * rng.standard_normal((m, 3))).astype(np.float32)
    if kind == "lattice":
        return rng.integers(-2, 3, size=(n, 3)).astype(np.float32), rng.integers(-2, 3, size=(m, 3)).astype(np.float32)
    if kind in ("rotated", "scaled"):
        src = rng.uniform(-1.0, 1.0, size=(n, 3))
        R, t, s = KNOWN_R, KNOWN_T, (1.3 if kind == "scaled" else 1.0)
        moved = s * (src.astype(np.float32).astype(np.float64) @ R.T) + t
        k = min(n, m)
        order = np.concatenate([[0], 1 + rng.permutation(k - 1)]) if k > 1 else np.zeros(1, dtype=np.int64)
        dst = np.concatenate([moved[order], rng.uniform(3.0, 4.0, size=(m - k, 3))])
        return src.astype(np.float32), dst.astype(np.float32)
    if kind == "far":
        src, dst = rng.standard_normal((n, 3)), rng.standard_normal((m, 3))
        src[::3] += 1e3
        return src.astype(np.float32), dst.astype(np.float32)
    raise ValueError(kind)


KNOWN_R = rotation_about([1.0, 2.0, -1.5], 8.0)
KNOWN_T = np.array([0.05, -0.03, 0.04])


def make_init(seed, degrees=5.0):
    """a transform near the identity: a small rotation about a seeded axis, a small shift, s = 1"""
    rng = np.random.default_rng(seed)
    return pack(rotation_about(rng.standard_normal(3), degrees), 0.1 * rng.standard_normal(3), 1.0)
