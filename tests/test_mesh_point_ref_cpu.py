"""The mesh-to-cloud column oracle and the contract's float32 restatement (tests/mesh_point_ref.py), without a GPU: the
restatement against the column oracle on every case of tests/test_gpu_mesh_point.py -- which is where that test's tolerance
constant K_MEASURED_COLS is measured (never against the kernel) -- the tie rule, the analytic gradient against finite
differences, and numpy surface_completeness on a case computed by hand."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_point_ref as MR                                                                 # noqa: E402
import point_mesh_ref as PR                                                                 # noqa: E402


def test_restatement_vs_column_oracle_measures_the_tolerance():
    """the worst |d2_32 - d2_64| / (2^-23 R^2) COLUMN-wise over every case of the GPU test: printed, and recorded as
    mesh_point_ref.K_MEASURED_COLS (the GPU tolerance is 4 x it).  Also what the restatement promises besides: finite results, the
    reported point in the float64 tie set, the closest point on its face."""
    ms = PR.meshes()
    worst, at = 0.0, None
    for key, name, pts in MR.cases():
        v, f = ms[name]
        R = PR.radius(v, pts)
        tol = MR.K_COLS * MR.EPS * R * R
        dcol, D, _, rows = MR.oracle_cols(v, f, pts)
        d32, k, q32, _, rows32 = MR.restate32_cols(v, f, pts)
        assert np.array_equal(rows, rows32) and np.isfinite(d32).all() and np.isfinite(q32).all(), key
        ratio = float(np.abs(d32.astype(np.float64) - dcol).max() / (MR.EPS * R * R))
        print("%-16s R %.3g  worst column ratio %.3f" % (key, R, ratio))
        if ratio > worst:
            worst, at = ratio, key
        j = np.arange(len(f))
        assert MR.tied_cols(D, tol)[np.searchsorted(rows, k), j].all(), key
        on = np.diagonal(PR.oracle(v, f, q32.astype(np.float64))[1])       # closest[j] against face j
        assert np.sqrt(on.max()) <= MR.K_COLS * MR.EPS * R, key
    print("K_MEASURED_COLS = %.3f at %s (recorded %.3f)" % (worst, at, MR.K_MEASURED_COLS))
    assert worst <= MR.K_MEASURED_COLS, "the recorded constant no longer covers the restatement: %.3f > %.3f" % (worst, MR.K_MEASURED_COLS)
    assert worst >= 0.5 * MR.K_MEASURED_COLS, "the recorded constant is stale: measured %.3f, recorded %.3f" % (worst, MR.K_MEASURED_COLS)


def test_column_minimum_is_the_transpose_of_the_row_minimum():
    """one matrix, two minima: the restatement's columns come from the very pairs32 matrix restate32 takes its rows from"""
    v, f = PR.meshes()["2tp3"]
    pts = PR.query_points(v, f, 257, 31)
    d_rows, face, _, D = PR.restate32(v, f, pts)
    d_cols, point, _, D2, rows = MR.restate32_cols(v, f, pts)
    assert np.array_equal(D, D2) and len(rows) == len(pts)
    assert (d_cols[face] <= d_rows).all() and (d_rows[point] <= d_cols).all() and d_rows.min() == d_cols.min()


def test_restatement_ties_go_to_the_lowest_point():
    v, f = PR.meshes()[MR.REPEAT_MESH]
    d32, k, _, D, rows = MR.restate32_cols(v, f, MR.repeated_cloud())
    assert (k == MR.REPEAT_AT[0]).all() and d32[MR.REPEAT_FACE] <= 4 * MR.EPS
    for i in MR.REPEAT_AT[1:]:
        assert np.array_equal(D[i], D[MR.REPEAT_AT[0]])
    v, f = PR.cube()
    pts = PR.cube_points()
    d32, k, _, D, rows = MR.restate32_cols(v, f, pts)
    ties = 0
    for j in range(len(f)):
        same = np.flatnonzero(D[:, j] == d32[j])
        assert k[j] == rows[same[0]]
        ties += len(same) >= 2
    assert ties >= len(f) // 2                                              # the points were chosen to tie


def test_non_finite_points_are_skipped():
    v, f = PR.meshes()["seven"]
    pts = PR.query_points(v, f, 65, 41)
    dirty = pts.copy()
    dirty[0, 1], dirty[17], dirty[64, 2] = np.nan, np.inf, -np.inf
    keep = np.array([i for i in range(65) if i not in (0, 17, 64)])
    a, b = MR.restate32_cols(v, f, dirty), MR.restate32_cols(v, f, pts[keep])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], keep[b[1]]) and np.array_equal(a[2], b[2])
    assert np.array_equal(MR.oracle_cols(v, f, dirty)[0], MR.oracle_cols(v, f, pts[keep])[0])


def test_analytic_gradient_against_finite_differences():
    v, f = PR.meshes()["seven"]
    pts = PR.query_points(v, f, 9, 51, far=True).astype(np.float64) * 0.02 + 0.3     # generic points: no ties, no point on the mesh
    g = np.random.RandomState(3).standard_normal(len(f))
    dcol, D, _, _ = MR.oracle_cols(v, f, pts)
    point = D.argmin(0)
    grad, credit = MR.grad64(v, f, pts, point, g)
    assert credit.sum() == len(f) and (grad[credit == 0] == 0).all()
    h = 1e-6
    for i in range(len(pts)):
        for c in range(3):
            up, dn = pts.copy(), pts.copy()
            up[i, c] += h
            dn[i, c] -= h
            fd = ((MR.oracle_cols(v, f, up)[0] - MR.oracle_cols(v, f, dn)[0]) * g).sum() / (2 * h)
            assert abs(fd - grad[i, c]) <= 1e-6 * max(1.0, np.abs(grad).max()), (i, c, fd, grad[i, c])


def test_surface_completeness_by_hand():
    """one face, the right triangle (0,0,0) (2,0,0) (0,2,0) of area 2, points at heights 1, 2 and 3 above its interior: the face's
    nearest point is the lowest, dist 1; with a second face of area 0.5 whose nearest point is 2 away (dist 4) the area-weighted
    mean is (2 * 1 + 0.5 * 4) / 2.5 = 1.6 and the uniform one 2.5"""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [10, 0, 0], [11, 0, 0], [10, 1, 0]], np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    pts = np.array([[0.5, 0.5, 3.0], [0.5, 0.5, 1.0], [0.25, 1.0, 2.0], [10.25, 0.25, 2.0]])
    dcol, D, _, rows = MR.oracle_cols(v, f[:1], pts[:3])
    assert np.allclose(dcol, [1.0]) and D.argmin(0)[0] == 1
    assert MR.completeness64(dcol, [2.0], 1) == 1.0 and MR.completeness64(dcol, [2.0], 1, "uniform") == 1.0
    dcol, D, _, _ = MR.oracle_cols(v, f, pts)
    area = np.array([2.0, 0.5, 0.0])                                      # (a padded column: ignored)
    dist = np.array([dcol[0], dcol[1], np.nan])
    assert np.allclose(dist[:2], [1.0, 4.0])
    assert abs(MR.completeness64(dist, area, 2) - 1.6) < 1e-15 and abs(MR.completeness64(dist, area, 2, "uniform") - 2.5) < 1e-15
    mean, pct = MR.completeness64(dist, area, 2, "area", threshold=2.0)
    assert abs(mean - 1.6) < 1e-15 and abs(pct - 80.0) < 1e-12
    assert abs(MR.completeness64(dist, area, 2, "uniform", threshold=2.0)[1] - 50.0) < 1e-12
    assert np.isnan(MR.completeness64([np.nan, np.nan], [0.0, 0.0], 2)) and np.isnan(MR.completeness64(dist, area, 3))
