"""Numpy restatement of dpf_icp_plane (include/dpf_hip.h: the point-to-plane block), with the operation order written out.  One slot
at a time; every array step is one numpy operation and every scalar step one Python float operation, so each rounds on its own.  The
match, the tree and the block order are align_ref.py's (dpf_icp's), called, not restated again.

    terms:      y' = y - c (c = target point 0), r = (n_0 (y_0 - q_0) + n_1 (y_1 - q_1)) + n_2 (y_2 - q_2), a = (y' x n ; n);
                thirty-one sums: W, the upper triangle of sum a a^T row-major, sum a r, S_d, S_r, S_yy; a zero product is +0.0
    solve:      A x = -b, the diagonal times (1 + 2^-40), LDL^T without pivoting, a pivot that is not > 0 drops its unknown
    increment:  the unit quaternion (1; omega / 2) / norm through align_ref.rotation, composed about the pivot
    icp_plane:  iters times (match, solve, compose), then one more match under the returned transform"""
import math

import numpy as np

import align_ref as A

NSUMS = 31
MIN_INLIERS = 6
DAMP = 1.0 + 2.0 ** -40
DEGENERATE, REFUSED = A.DEGENERATE, A.REFUSED
# |R^T R - I| grows by at most this per composition (the operation count), u = 2^-53:
#   the quaternion: each component carries the norm's relative error (three roundings of the sum of squares halved by the root, the
#   root, the division: <= 3.5 u), so | |q|^2 - 1 | <= 7 u and the exact formula's R^T R = |q|^4 I is off by <= 14 u;
#   the formula's entries: at most four roundings of quantities <= 1, <= 3 u an entry, <= 2 sqrt(3) 3 u < 12 u on an entry of R^T R;
#   the product dR R: five roundings an entry, <= 3 u an entry by Cauchy-Schwarz, < 12 u on an entry of R^T R.
ORTHO_PER_COMPOSITION = 40 * 2.0 ** -53
# The bound between the restated solve and numpy.linalg.lstsq on the same damped system: |A (x - x_lstsq)| / |b| in the maximum
# norm.  Measured in test_align_plane_ref_cpu.py over the kinds there: the worst deviation is 7.0e-13 (the fit kind "small"),
# recorded below; the bound is that figure times 8, as align_ref.ALIGN_BOUND was made.
SOLVE_WORST_MEASURED = 7.5e-13
SOLVE_BOUND = 8 * SOLVE_WORST_MEASURED


def tri(i, j):
    return 6 * i - i * (i - 1) // 2 + (j - i)


def ortho_bound(compositions, start=0.0):
    return start + ORTHO_PER_COMPOSITION * compositions


def match(src, dst, normals, T, max_dist2=0.0, prev=None):
    """align_ref.match, then the normal's rule -> (index, dist, weight, changed, y (n, 3) fp32)"""
    index, dist, weight, changed = A.match(src, dst, T, max_dist2, prev)
    y, usable = A.transform_points(T, src)
    nrm = np.asarray(normals, dtype=np.float64)[np.where(index >= 0, index, 0)]
    weight = np.where(np.isfinite(nrm).all(-1), weight, 0.0)
    return index, dist, weight, changed, y


def terms(y, dst, normals, index, dist, weight):
    """(n, 31) float64"""
    dst = np.asarray(dst, dtype=np.float32)
    n = y.shape[0]
    ok = weight > 0
    j = np.where(ok, index, 0)
    yd = np.where(ok[:, None], y, np.float32(0)).astype(np.float64)
    q = dst[j].astype(np.float64)
    nv = np.where(ok[:, None], np.asarray(normals, dtype=np.float64)[j], 0.0)
    c = dst[0].astype(np.float64)
    t = np.zeros((n, NSUMS), dtype=np.float64)
    with np.errstate(all="ignore"):
        yp = [yd[:, x] - c[x] for x in range(3)]
        r = (nv[:, 0] * (yd[:, 0] - q[:, 0]) + nv[:, 1] * (yd[:, 1] - q[:, 1])) + nv[:, 2] * (yd[:, 2] - q[:, 2])
        a = [yp[1] * nv[:, 2] - yp[2] * nv[:, 1], yp[2] * nv[:, 0] - yp[0] * nv[:, 2], yp[0] * nv[:, 1] - yp[1] * nv[:, 0],
             nv[:, 0], nv[:, 1], nv[:, 2]]
        t[:, 0] = 1.0
        for i in range(6):
            for k in range(i, 6):
                t[:, 1 + tri(i, k)] = a[i] * a[k] + 0.0
            t[:, 22 + i] = a[i] * r + 0.0
        t[:, 28] = np.where(ok, dist, np.float32(0)).astype(np.float64)
        t[:, 29] = r * r
        t[:, 30] = (yp[0] * yp[0] + yp[1] * yp[1]) + yp[2] * yp[2]
    t[~ok] = 0.0
    return t


def plane_sums(y, dst, normals, index, dist, weight):
    return A.reduce_terms(terms(y, dst, normals, index, dist, weight))


def system(S):
    """(A (6, 6) symmetric, undamped; b (6,)) of the sums"""
    M = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            M[i, j] = M[j, i] = S[1 + tri(i, j)]
    return M, np.array(S[22:28], dtype=np.float64)


def ldl_solve(S):
    """x (list of 6 floats) and ok (list of 6 bools): the damped A x = -b by the header's LDL^T"""
    S = [float(v) for v in S]
    D, ok = [0.0] * 6, [False] * 6
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = S[1 + tri(j, j)] * DAMP
        for c in range(j):
            d = d - (L[j][c] * L[j][c]) * D[c]
        ok[j] = d > 0.0
        D[j] = d if ok[j] else 0.0
        for i in range(j + 1, 6):
            e = S[1 + tri(j, i)]
            for c in range(j):
                e = e - (L[i][c] * L[j][c]) * D[c]
            L[i][j] = e / d if ok[j] else 0.0
    x = [0.0] * 6
    for i in range(6):
        y = -S[22 + i]
        for c in range(i):
            y = y - L[i][c] * x[c]
        x[i] = y if ok[i] else 0.0
    for i in range(6):
        x[i] = x[i] / D[i] if ok[i] else 0.0
    for i in range(5, -1, -1):
        v = x[i]
        for c in range(i + 1, 6):
            v = v - L[c][i] * x[c]
        x[i] = v if ok[i] else 0.0
    return x, ok


def increment(x):
    """dR (3 x 3 lists) of omega = x[:3]"""
    h = [0.5 * x[0], 0.5 * x[1], 0.5 * x[2]]
    norm = math.sqrt(((1.0 + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2])
    return A.rotation([1.0 / norm, h[0] / norm, h[1] / norm, h[2] / norm])


def compose(T, x, c):
    """the increment x = (omega ; tau) composed onto T about the pivot c (3,) fp32 -> T (13,)"""
    T = [float(v) for v in T]
    c = [float(np.float32(v)) for v in c]
    dR = increment(x)
    R = [[(dR[a][0] * T[b] + dR[a][1] * T[3 + b]) + dR[a][2] * T[6 + b] for b in range(3)] for a in range(3)]
    u = [T[9] - c[0], T[10] - c[1], T[11] - c[2]]
    t = [(((dR[a][0] * u[0] + dR[a][1] * u[1]) + dR[a][2] * u[2]) + c[a]) + x[3 + a] for a in range(3)]
    return A.pack(R, t, 1.0)


def solve(S, inliers, c, T):
    """S (31,), the inlier count, the pivot, the current transform -> (T (13,) or None where the slot is degenerate, step^2)"""
    S = [float(v) for v in S]
    W = S[0]
    if inliers < MIN_INLIERS or not W > 0.0:
        return None, math.nan
    x, _ = ldl_solve(S)
    with np.errstate(all="ignore"):
        new = compose(T, x, c)
        mean = np.float64(S[30]) / np.float64(W)
        step2 = float(np.float64((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + np.float64((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) / mean)
    if not (np.isfinite(new).all() and math.isfinite(step2)):
        return None, math.nan
    return new, step2


def normals_refused(normals):
    v = np.abs(np.asarray(normals, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return bool(((v > A.LIMIT) & (v < np.inf)).any())


def icp_plane(src, dst, normals, iters=30, max_dist2=0.0, tol=1e-7, init=None):
    """one slot -> dict(T, index, dist, rmse, rmse_plane, step, inliers (iters + 1,) each, iterations, sums (31,), status, changed)"""
    src, dst = np.asarray(src, dtype=np.float32), np.asarray(dst, dtype=np.float32)
    normals = np.asarray(normals, dtype=np.float64)
    n = src.shape[0]
    T = A.IDENTITY.copy() if init is None else np.asarray(init, dtype=np.float64).reshape(13).copy()
    nan = np.full(iters + 1, np.nan)
    rmse, rmse_plane, step, inl = nan.copy(), nan.copy(), nan.copy(), np.zeros(iters + 1, dtype=np.int32)
    if A.out_of_range(src) or A.out_of_range(dst) or A.out_of_range(T) or T[12] != 1.0 or normals_refused(normals):
        return dict(T=np.full(13, np.nan), index=np.full(n, -1, dtype=np.int32), dist=np.full(n, np.nan, dtype=np.float32), rmse=rmse,
                    rmse_plane=rmse_plane, step=step, inliers=inl, iterations=0, sums=np.full(NSUMS, np.nan), status=REFUSED, changed=[])
    tol2 = float(tol) * float(tol)
    status, iterations, done, prev, changes, last2 = 0, iters, False, None, [], math.nan
    for k in range(iters + 1):
        if done:
            rmse[k], rmse_plane[k], step[k], inl[k] = rmse[k - 1], rmse_plane[k - 1], step[k - 1], inl[k - 1]
            continue
        index, dist, weight, changed, y = match(src, dst, normals, T, max_dist2, prev)
        prev = index
        changes.append(changed)
        S = plane_sums(y, dst, normals, index, dist, weight)
        inl[k] = int((weight > 0).sum())
        with np.errstate(all="ignore"):
            rmse[k], rmse_plane[k] = np.sqrt(S[28] / S[0]), np.sqrt(S[29] / S[0])
        step[k] = 0.0
        if (k > 0 and changed == 0 and last2 <= tol2) or k == iters:
            done, iterations = True, k
            continue
        new, step2 = solve(S, int(inl[k]), dst[0], T)
        if new is None:
            done, iterations, status = True, k, DEGENERATE
            continue
        T, last2, step[k] = new, step2, math.sqrt(step2)
    return dict(T=T, index=index, dist=dist, rmse=rmse, rmse_plane=rmse_plane, step=step, inliers=inl, iterations=iterations, sums=S,
                status=status, changed=changes)


# ---- the clouds of the tests, from a seed ---------------------------------------------------------------------------------------------
AXES = np.array([1.0, 0.7, 0.4])


def ellipsoid(n, rng):
    """(points (n, 3) float64 on the ellipsoid with the axes 1, 0.7, 0.4; their analytic unit normals)"""
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    p = g * AXES
    nrm = p / AXES ** 2
    return p, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def make_ellipsoid_pair(n, m, seed, degrees=5.0):
    """two independent samplings of one ellipsoid, the source turned by `degrees` about a fixed axis and shifted ->
    (src (n, 3) fp32, dst (m, 3) fp32, normals (m, 3) float64 analytic, the R and t that bring src back onto dst)"""
    rng = np.random.default_rng(seed)
    p, _ = ellipsoid(n, rng)
    q, nq = ellipsoid(m, rng)
    R = A.rotation_about([1.0, 2.0, -1.5], degrees)
    t = np.array([0.03, -0.02, 0.025])
    src = (p - t) @ R                                                                        # R src + t = p
    return src.astype(np.float32), q.astype(np.float32), nq, R, t


def make_planar_target(n, m, seed):
    """a target in the plane z = 0.25 with the normal (0, 0, 1): three degrees of freedom are unconstrained"""
    rng = np.random.default_rng(seed)
    dst = np.concatenate([rng.uniform(-1, 1, (m, 2)), np.full((m, 1), 0.25)], axis=1)
    src = np.concatenate([rng.uniform(-0.8, 0.8, (n, 2)), np.zeros((n, 1))], axis=1) @ A.rotation_about([1.0, 0.3, 0.0], 4.0).T
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (m, 1))
    return src.astype(np.float32), dst.astype(np.float32), nrm


def make_collinear_target(n, m, seed):
    """a target on one line, its normals all in one direction across it"""
    rng = np.random.default_rng(seed)
    d = np.array([1.0, 0.5, -0.25])
    dst = np.outer(rng.uniform(-1, 1, m), d) + 0.1
    src = np.outer(rng.uniform(-1, 1, n), d) + 0.1 + 0.02 * rng.standard_normal((n, 3))
    nrm = np.tile(np.cross(d, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(d, [0.0, 0.0, 1.0])), (m, 1))
    return src.astype(np.float32), dst.astype(np.float32), nrm


def pair_normals(dst, seed):
    """seeded unit normals for the clouds of align_ref.make_pair (any direction serves the bit-level tests)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((np.asarray(dst).shape[0], 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rotation_error_degrees(R, want):
    c = (np.trace(np.asarray(R) @ np.asarray(want).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
