"""Point-to-mesh distance: a float64 oracle, the float32 restatement of the kernel's contract (include/dpf_hip.h) and the cases
the CPU and GPU tests share.  TEST INFRASTRUCTURE, numpy only: never imported by the package.

The oracle is formulated differently from the kernel: per face the minimum of the three point-segment distances and, where
the point's projection falls inside the triangle, the distance to its plane; no region classification, no barycentric solve."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_cases as MC                                                                     # noqa: E402

EPS = 2.0 ** -23
TILE = 256                # csrc/dispatch.h PM_TILE; the GPU test asserts dpf_point_mesh_tile() against it
THIN = np.float32(2.0 ** -14)

# The tolerance constant, MEASURED by tests/test_point_mesh_ref_cpu.py::test_restatement_vs_oracle_measures_the_tolerance: the
# worst |d2_32 - d2_64| / (2^-23 R^2) of restate32 against the oracle over every case below is K_MEASURED; the GPU tolerance is
# atol = K * 2^-23 * R^2 with K = 4 * K_MEASURED (the factor covers contraction and ordering differences between numpy and the
# device compiler).  The CPU test fails if the measurement moves above the recorded value.
K_MEASURED = 1.37        # measured 1.369 (spread300/far: 65 points 100 extents away from faces of eight decades of area)
K = 4.0 * K_MEASURED


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------
def _segment(p, a, b):
    """closest points of the segments a-b to the points p: p (N, 1, 3), a / b (1, F, 3) -> (N, F, 3)"""
    d = b - a
    dd = (d * d).sum(-1, keepdims=True)
    t = np.where(dd > 0, ((p - a) * d).sum(-1, keepdims=True) / np.where(dd > 0, dd, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0) * d


def oracle(v, f, pts):
    """(dmin (N,), D (N, F), C (N, F, 3)): the squared distance to the mesh, to every face, and the closest point on every face."""
    v, p = np.asarray(v, np.float64), np.asarray(pts, np.float64).reshape(-1, 1, 3)
    f = np.asarray(f).astype(np.int64)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    C = D = None
    for s, e in ((a, b), (b, c), (c, a)):
        q = _segment(p, s, e)
        d = ((p - q) ** 2).sum(-1)
        if D is None:
            C, D = q, d
        else:
            better = d < D
            C, D = np.where(better[..., None], q, C), np.where(better, d, D)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1, keepdims=True)
    ok = nn[..., 0] > 0
    h = ((p - a) * n).sum(-1, keepdims=True) / np.where(nn > 0, nn, 1.0)
    q = p - h * n
    inside = ok
    for s, e in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(e - s, q - s) * n).sum(-1) >= 0)
    d = ((p - q) ** 2).sum(-1)
    take = inside & (d < D)
    C, D = np.where(take[..., None], q, C), np.where(take, d, D)
    return D.min(1), D, C


def tied(D, tol):
    """per point the faces within tol of the minimum"""
    return D <= D.min(1, keepdims=True) + tol


# ---- the contract's float32 sequence ---------------------------------------------------------------------------------------
def _f(x):
    return np.asarray(x, np.float32)


def fma(x, y, z):
    """the fused multiply-add of float32 operands (the product is exact in float64)"""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def _dot(x, y):
    return fma(x[..., 2], y[..., 2], fma(x[..., 1], y[..., 1], x[..., 0] * y[..., 0]))


def _clamp01(x):
    return np.fmin(np.fmax(x, np.float32(0)), np.float32(1))          # (fmax / fmin drop a NaN, as the device's do)


def stage32(v, f):
    v, f = _f(v), np.asarray(f).astype(np.int64)
    a = v[f[:, 0]]
    ab, ac = v[f[:, 1]] - a, v[f[:, 2]] - a
    aa, g, cc = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    e = ac - ab
    bb = _dot(e, e)
    det = fma(aa, cc, -(g * g))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = lambda x: np.where(x > 0, np.float32(1) / np.where(x > 0, x, np.float32(1)), np.float32(0)).astype(np.float32)   # noqa: E731
        fat = det > THIN * (aa * cc)
        idet = np.where(fat, np.float32(1) / np.where(fat, det, np.float32(1)), np.float32(0)).astype(np.float32)
    return dict(a=a, ab=ab, ac=ac, aa=aa, g=g, cc=cc, iaa=inv(aa), icc=inv(cc), ibc=inv(bb), idet=idet)


def _point(s, p, v, w):
    q = fma(w[..., None], s["ac"][None], fma(v[..., None], s["ab"][None], np.broadcast_to(s["a"][None], v.shape + (3,))))
    d = p - q
    return q, _dot(d, d)


def pairs32(v, f, pts):
    """(D (N, F) float32, Q (N, F, 3) float32): the contract's distance and closest point of every (point, face) pair"""
    s = stage32(v, f)
    p = _f(pts).reshape(-1, 1, 3)
    zero, one = np.float32(0), np.float32(1)
    with np.errstate(all="ignore"):
        ap = p - s["a"][None]
        d1, d2 = _dot(s["ab"][None], ap), _dot(s["ac"][None], ap)
        d3, d4, d5, d6 = d1 - s["aa"], d2 - s["g"], d1 - s["g"], d2 - s["cc"]
        tab, tac, tbc = _clamp01(d1 * s["iaa"]), _clamp01(d2 * s["icc"]), _clamp01((d4 - d3) * s["ibc"])
        z = np.zeros_like(tab)
        # thin faces: AB, then AC, then BC, a later one only if strictly nearer
        q, d = _point(s, p, tab, z)
        for vv, ww in ((z, tac), (one - tbc, tbc)):
            q2, e = _point(s, p, vv, ww)
            lower = e < d
            q, d = np.where(lower[..., None], q2, q), np.where(lower, e, d)
        vb, vc = fma(s["cc"] + z, d1, -(s["g"] * d2)), fma(s["aa"] + z, d2, -(s["g"] * d1))
        vi, wi = vb * s["idet"], vc * s["idet"]
        vw = [vi, wi]

        def put(c, x, y):
            vw[0], vw[1] = np.where(c, x, vw[0]), np.where(c, y, vw[1])
        put((vi + wi >= one) & (d4 - d3 >= zero) & (d5 - d6 >= zero), one - tbc, tbc)
        put((vb <= zero) & (d2 >= zero) & (d6 <= zero), z, tac)
        put((d6 >= zero) & (d5 <= d6), z, z + one)
        put((vc <= zero) & (d1 >= zero) & (d3 <= zero), tab, z)
        put((d3 >= zero) & (d4 <= d3), z + one, z)
        put((d1 <= zero) & (d2 <= zero), z, z)
        vv = _clamp01(vw[0]).astype(np.float32)
        ww = np.fmin(np.fmax(vw[1], zero), one - vv).astype(np.float32)
        qf, df = _point(s, p, vv, ww)
    thin = (s["idet"] == 0)[None]
    return np.where(thin, d, df).astype(np.float32), np.where(thin[..., None], q, qf).astype(np.float32)


def restate32(v, f, pts):
    """(dist (N,), face (N,), closest (N, 3), D (N, F)): the contract with the lowest-index tie rule (argmin returns the first)"""
    D, Q = pairs32(v, f, pts)
    k = D.argmin(1)
    i = np.arange(len(k))
    return D[i, k], k.astype(np.int32), Q[i, k], D


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def cube():
    """a closed unit cube of 12 triangles centred on the origin"""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32)
    return v, f


def cube_points():
    """on the symmetry axes and the face diagonals, outside and inside: nearest to shared edges, vertices and face centres"""
    pts = []
    for r in (0.0, 0.125, 0.25, 0.75, 1.0, 2.0):
        for ax in np.eye(3):
            pts += [r * ax, -r * ax]
        for d in ((1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 0, -1), (1, 1, 1), (-1, 1, -1)):
            pts.append(r * np.array(d, np.float64))
    for s in (0.5, 0.75):                                   # in and above the faces, along their diagonals
        for t in (-0.25, 0.0, 0.25):
            pts += [[s, t, t], [t, s, -t], [t, t, -s]]
    return np.array(pts, np.float32)


def degenerate_soup():
    """a soup with zero-area faces (three collinear vertices, exactly: a midpoint of representable ends) and faces with a repeated
    vertex spliced in"""
    v, f = MC.soup(40, 301)
    v = np.round(v * 64) / 64                               # (coordinates on a 1/64 grid: midpoints are exact)
    v = np.concatenate([v, [(v[0] + v[1]) / 2, v[5]]]).astype(np.float32)
    extra = np.array([[0, 1, len(v) - 2], [0, len(v) - 2, 1], [3, 3, 9], [4, 7, 7], [8, 2, 8], [6, 6, 6], [5, len(v) - 1, 11]], np.uint32)
    f = np.concatenate([f[:10], extra[:3], f[10:30], extra[3:], f[30:]])
    return v, f


def meshes():
    out = {"one": MC.one_face(), "seven": MC.seven_faces(), "spread300": MC.spread(), "cube": cube(), "degen": degenerate_soup()}
    for name, F, seed in (("tm1", TILE - 1, 201), ("t", TILE, 202), ("tp1", TILE + 1, 203), ("2tp3", 2 * TILE + 3, 204)):
        out[name] = MC.soup(F, seed)
    return out


ORDER = ["one", "seven", "spread300", "cube", "degen", "tm1", "t", "tp1", "2tp3"]
SIZES = (1, 63, 64, 65, 129)


def query_points(v, f, n, seed, far=False):
    """n points: Gaussian around the mesh, then points exactly on vertices, at edge midpoints and at face centroids (float32
    roundings of them), cycled; far: 100 x the mesh's extent away"""
    rng = np.random.RandomState(seed)
    v64 = np.asarray(v, np.float64)
    lo, hi = v64.min(0), v64.max(0)
    centre, extent = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    if far:
        d = rng.standard_normal((n, 3))
        return (centre + 100.0 * extent * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    tri = v64[np.asarray(f).astype(np.int64)]
    pool = [centre + 0.5 * extent * rng.standard_normal((n, 3)), tri[:, 0], (tri[:, 0] + tri[:, 1]) / 2, (tri[:, 1] + tri[:, 2]) / 2,
            tri.mean(1)]
    pts = np.empty((n, 3))
    for i in range(n):
        src = pool[i % len(pool)]
        pts[i] = src[(i // len(pool)) % len(src)]
    return pts.astype(np.float32)


def cases():
    """[(key, mesh name, points (n, 3))]: every mesh at a size of SIZES (cycled), the three-tile soup at every size, far points"""
    ms = meshes()
    out = []
    for i, name in enumerate(ORDER):
        n = SIZES[i % len(SIZES)]
        out.append(("%s/%d" % (name, n), name, query_points(*ms[name], n, 500 + i)))
    for j, n in enumerate(SIZES):
        out.append(("2tp3/%d/b" % n, "2tp3", query_points(*ms["2tp3"], n, 600 + j)))
    for j, name in enumerate(("seven", "spread300", "2tp3")):
        out.append(("%s/far" % name, name, query_points(*ms[name], 65, 700 + j, far=True)))
    out.append(("cube/axes", "cube", cube_points()))
    return out


def radius(v, pts):
    return float(max(np.abs(np.asarray(v, np.float64)).max(), np.abs(np.asarray(pts, np.float64)).max()))
