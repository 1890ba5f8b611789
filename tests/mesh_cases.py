"""Meshes, variates and numpy restatements shared by tools/gen_golden_mesh_sampling.py and the mesh-sampling tests.
TEST INFRASTRUCTURE: never imported by the package.

The meshes come from seeds (numpy's legacy RandomState, whose streams are frozen); the golden file stores the small ones and a
checksum of every one, so a drift of the generator shows.  `restate` is lib/datasets/cloud_sampling.py:4-32 with the variates
as arguments; the generator proves it against the reference's own sample_cloud before it writes anything."""
import zlib

import numpy as np

T = 256                                   # csrc/mesh_sample.hip MS_TILE: faces per scan tile of the cumulative distribution
EDGE_TOL = 2.0 ** -23                     # how far a reference edge can lie from the exact-ratio edge (tests/test_gpu_mesh_sampling.py)
U_MAX = np.nextafter(1.0, 0.0)            # the largest double below 1

SHIFT = (0.00055863, 0.00127477, 0.01701898)            # configs/autoencoding/all_original.yaml
TRANSFORMS = {
    "original": dict(cloud_rescale2orig=True, cloud_recenter2orig=True, cloud_translate=True, cloud_translate_shift=list(SHIFT)),
    "scaled": dict(cloud_scale=True, cloud_scale_scale=2.0),
    "centered": dict(cloud_scale=True, cloud_scale_scale=2.0, cloud_center=True),
}
ORIG_C = np.array([0.1203, -0.4172, 0.3051], np.float32)
ORIG_S = np.float32(1.7345)


def one_face():
    return np.array([[0.1, 0.2, 0.3], [0.7, -0.2, 0.1], [-0.3, 0.5, 0.9]], np.float32), np.array([[0, 1, 2]], np.uint32)


def seven_faces():
    """the first two faces and the last one are degenerate: a repeated vertex, three collinear points, a repeated vertex"""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0.5, -0.5, 0.25]], np.float32)
    f = np.array([[0, 0, 1], [0, 1, 2], [0, 1, 3], [0, 3, 4], [1, 4, 5], [3, 5, 6], [4, 4, 6]], np.uint32)
    return v, f


def spread(F=300, decades=8, seed=11):
    """F separate triangles whose areas fall from ~1e-1 to ~1e-(1 + decades), shuffled"""
    rng = np.random.RandomState(seed)
    size = 10.0 ** (-0.5 * decades * rng.permutation(F) / (F - 1.0))
    centre = rng.random_sample((F, 1, 3)) - 0.5
    v = (centre + size[:, None, None] * (rng.random_sample((F, 3, 3)) - 0.5)).astype(np.float32).reshape(-1, 3)
    return v, np.arange(3 * F, dtype=np.uint32).reshape(F, 3)


def soup(F, seed):
    """F triangles over F // 2 + 3 shared vertices in the unit cube"""
    rng = np.random.RandomState(seed)
    V = F // 2 + 3
    v = (rng.random_sample((V, 3)) - 0.5).astype(np.float32)
    i0 = rng.randint(0, V, size=F)
    f = np.stack([i0, (i0 + rng.randint(1, 4, size=F)) % V, (i0 + rng.randint(4, 8, size=F)) % V], axis=1).astype(np.uint32)
    return v, f


MESHES = {
    "one": one_face, "seven": seven_faces, "spread300": spread,
    "tm1": lambda: soup(T - 1, 101), "t": lambda: soup(T, 102), "tp1": lambda: soup(T + 1, 103), "2tp3": lambda: soup(2 * T + 3, 104),
    "big": lambda: soup(20000, 105), "fifty": lambda: soup(50, 106),
}
STORED = ("one", "seven", "spread300")    # small enough to live in the golden file

# (mesh, cloud_size, return_eval_cloud, seed, force u[0] = 0 and u[1] = U_MAX -- only where two forced samples stay under the
# 2 % cap on samples near a reference edge)
CASES = [(m, 64, True, 1000 + i, m in ("seven", "spread300", "big")) for i, m in enumerate(
    ("one", "seven", "spread300", "tm1", "t", "tp1", "2tp3", "big"))]
CASES += [(m, n, e, 2000 + 100 * j + 10 * i + int(e), False) for j, m in enumerate(("spread300", "2tp3")) for i, n in enumerate((1, 63, 65))
          for e in (False, True)]
CASES += [("seven", 1, False, 2901, False), ("spread300", 64, False, 2902, False),
          ("big", 2048, False, 3000, False), ("big", 2048, True, 3001, True)]
TRANSFORM_CASES = [("2tp3", 65, True, 4000), ("spread300", 64, False, 4001)]     # every entry of TRANSFORMS on each


def case_key(mesh, n, ev, seed):
    return "%s/%d/%d/%d" % (mesh, n, int(ev), seed)


def checksum(v, f):
    return zlib.crc32(np.ascontiguousarray(f).tobytes(), zlib.crc32(np.ascontiguousarray(v).tobytes()))


def pack(meshes):
    """[(vertices, faces)] -> vertices, vertex_bounds, faces, face_bounds as meshes.h5 holds them"""
    vb = np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.uint64)
    fb = np.cumsum([0] + [len(f) for _, f in meshes]).astype(np.uint64)
    return np.concatenate([v for v, _ in meshes]), vb, np.concatenate([f for _, f in meshes]), fb


def draw(seed, S, forced=False):
    """the variates sample_cloud consumes after np.random.seed(seed): choice's uniforms, then s1, then s2"""
    rng = np.random.RandomState(seed)
    u = rng.random_sample(S)
    s1 = rng.random_sample((S, 1)).astype(np.float32)
    s2 = rng.random_sample((S, 1)).astype(np.float32)
    if forced:
        u[0] = 0.0
        if S > 1:
            u[1] = U_MAX
    return u, s1, s2


def areas(v, f):
    polygons = v[f]
    cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
    return np.sqrt((cross ** 2).sum(1)) / 2.0


def reference_edges(v, f):
    """the float64 edges np.random.choice searches: cumsum of the fp32 probabilities, divided by its last element"""
    a = areas(v, f)
    cdf = (a / a.sum()).astype(np.float64).cumsum()
    return cdf / cdf[-1]


def tiled_edges(v, f):
    """the kernel's contract (include/dpf_hip.h): running sums in double inside tiles of T faces, the tile totals summed one
    after the other, (offset + inside) / total"""
    a = areas(v, f).astype(np.float64)
    out, off = np.empty(len(a)), 0.0
    for lo in range(0, len(a), T):
        run = np.cumsum(a[lo:lo + T])                    # (numpy's cumsum adds one after the other)
        off, out[lo:lo + T] = off + run[-1], off + run
    return out / off


def points(v, f, k, s1, s2):
    """the fp32 formula of sample_cloud on the faces k: (S, 3)"""
    s1, s2 = s1.reshape(-1, 1).copy(), s2.reshape(-1, 1).copy()
    cond = (s1 + s2) > 1.
    s1[cond] = 1. - s1[cond]
    s2[cond] = 1. - s2[cond]
    sp = v[f][k]
    return (sp[:, 0] + s1 * (sp[:, 1] - sp[:, 0]) + s2 * (sp[:, 2] - sp[:, 0])).astype(np.float32)


def restate(v, f, u, s1, s2, edges=None):
    """sample_cloud with its variates as arguments: the faces and the (S, 3) points before the split"""
    k = (reference_edges(v, f) if edges is None else edges).searchsorted(u, side="right")
    return k, points(v, f, k, s1, s2)


def split(pts, ev):
    """(S, 3) -> the sample dict's (3, N) arrays"""
    if ev:
        return {"cloud": pts[::2].T, "eval_cloud": pts[1::2].T}
    return {"cloud": pts.T}


def near_edge(u, edges):
    """which u lie within EDGE_TOL of a reference edge"""
    j = np.clip(edges.searchsorted(u), 0, len(edges) - 1)
    d = np.abs(edges[j] - u)
    d = np.minimum(d, np.abs(edges[np.maximum(j - 1, 0)] - u))
    return d <= EDGE_TOL
