"""Mesh-to-cloud distance (per face the nearest point): the column view of tests/point_mesh_ref.py's (point, face) matrices -- a
float64 column oracle, the float32 restatement of the contract (include/dpf_hip.h) with the lowest-point-index tie rule, a
float64 analytic gradient, numpy surface_completeness, and the cases the CPU and GPU tests share.  TEST INFRASTRUCTURE, numpy
only: never imported by the package."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import point_mesh_ref as PR                                                                 # noqa: E402

EPS = PR.EPS
TILE = 256                # csrc/dispatch.h MP_TILE (points per LDS tile) and MP_WG_FACES; the GPU test asserts dpf_mesh_point_tile()

# The tolerance constant of the COLUMN minima, MEASURED by tests/test_mesh_point_ref_cpu.py::
# test_restatement_vs_column_oracle_measures_the_tolerance: the worst |d2_32 - d2_64| / (2^-23 R^2) of restate32_cols against the
# column oracle over every case below.  point_mesh_ref.K_MEASURED was measured on row minima only and need not hold here: a
# face's nearest point can be a far one.  The GPU tolerance is atol = K_COLS * 2^-23 * R^2 with K_COLS = 4 * K_MEASURED_COLS (the
# factor, as for K, covers contraction and ordering differences between numpy and the device compiler).  The CPU test fails if
# the measurement moves above the recorded value.
K_MEASURED_COLS = 3.17   # measured 3.162 (tm1/1: one point, so every face's nearest is that point, near or far; R is only 0.497)
K_COLS = 4.0 * K_MEASURED_COLS


def finite_rows(pts):
    """the indices of the points with three finite coordinates: the others are skipped"""
    return np.flatnonzero(np.isfinite(np.asarray(pts, np.float64)).all(1))


# ---- the float64 column oracle ---------------------------------------------------------------------------------------------------
def oracle_cols(v, f, pts):
    """(dcol (F,), D (n, F), C (n, F, 3), rows (n,)): per face the squared distance to the nearest finite point, the whole matrix
    over the finite points, the closest points, and the indices of those points in pts"""
    rows = finite_rows(pts)
    _, D, C = PR.oracle(v, f, np.asarray(pts)[rows])
    return D.min(0), D, C, rows


def tied_cols(D, tol):
    """per face the (finite) points within tol of the minimum: (n, F) bool"""
    return D <= D.min(0, keepdims=True) + tol


# ---- the contract's float32 sequence, column-wise ----------------------------------------------------------------------------------
def restate32_cols(v, f, pts):
    """(dist (F,), point (F,), closest (F, 3), D (n, F), rows): the contract with the lowest-index tie rule (argmin returns the
    first, and rows ascend)"""
    rows = finite_rows(pts)
    D, Q = PR.pairs32(v, f, np.asarray(pts)[rows])
    k = D.argmin(0)
    j = np.arange(D.shape[1])
    return D[k, j], rows[k].astype(np.int32), Q[k, j], D, rows


# ---- the float64 analytic gradient -------------------------------------------------------------------------------------------------
def grad64(v, f, pts, point, grad_dist):
    """d (sum_f grad_dist[f] * dist[f]) / d pts given the reported nearest points: (N, 3) float64 and the number of faces credited
    to each point (N,).  Face f adds 2 * grad_dist[f] * (p - c) to point[f], c the float64 closest point of face f to p."""
    pts64 = np.asarray(pts, np.float64)
    out, credit = np.zeros_like(pts64), np.zeros(len(pts64), np.int64)
    for j in np.flatnonzero(np.asarray(point) >= 0):
        i = int(point[j])
        _, _, C = PR.oracle(v, np.asarray(f)[j:j + 1], pts64[i:i + 1])
        out[i] += 2.0 * float(grad_dist[j]) * (pts64[i] - C[0, 0])
        credit[i] += 1
    return out, credit


# ---- surface_completeness in float64 -------------------------------------------------------------------------------------------------
def completeness64(dist, area, F, weights="area", threshold=None):
    """the weighted mean of dist[:F] (and the weighted percentage below the threshold) in float64; NaN for a bad slot"""
    d = np.asarray(dist, np.float64)[:F]
    if F == 0 or not np.isfinite(d).all():
        return (np.nan, np.nan) if threshold is not None else np.nan
    w = np.asarray(area, np.float64)[:F] if weights == "area" else np.ones(F)
    w = w / w.sum()
    mean = float((w * d).sum())
    if threshold is None:
        return mean
    return mean, float(100.0 * (w * (d < threshold)).sum())


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
TILE_SIZES = (255, 256, 257, 513)       # a point tile less one, a tile, a tile and one, two tiles and one
REPEAT_AT = (3, 70, 300)                # one point at three indices, in two point tiles
REPEAT_MESH, REPEAT_FACE, REPEAT_N = "tp1", 5, 320


def repeated_cloud():
    """a cloud over REPEAT_MESH whose points REPEAT_AT are all the (float32) centroid of face REPEAT_FACE and whose other points
    lie a hundred extents away: every face's nearest, three times at the same distance"""
    v, f = PR.meshes()[REPEAT_MESH]
    pts = PR.query_points(v, f, REPEAT_N, 1200, far=True)
    c = v.astype(np.float64)[f[REPEAT_FACE].astype(np.int64)].mean(0).astype(np.float32)
    for i in REPEAT_AT:
        pts[i] = c
    return pts


def cases():
    """[(key, mesh name, points (n, 3))]: point_mesh_ref's cases (cube/axes among them: its symmetric points tie exactly on
    several faces), then clouds that cross the 256-point tile, a single point, and the repeated point"""
    ms = PR.meshes()
    out = list(PR.cases())
    for a, name in enumerate(("seven", "2tp3")):
        for j, n in enumerate(TILE_SIZES):
            out.append(("%s/%d/t" % (name, n), name, PR.query_points(*ms[name], n, 1000 + 10 * a + j)))
    out.append(("2tp3/1/t", "2tp3", PR.query_points(*ms["2tp3"], 1, 1100)))
    out.append(("%s/repeat" % REPEAT_MESH, REPEAT_MESH, repeated_cloud()))
    return out
