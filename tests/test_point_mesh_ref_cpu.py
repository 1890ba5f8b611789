"""The point-to-mesh oracle and the contract's float32 restatement (tests/point_mesh_ref.py), without a GPU: the oracle against
analytic cases, and the restatement against the oracle on every case of tests/test_gpu_point_mesh.py -- which is where the
GPU test's tolerance constant is measured (never against the kernel)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import point_mesh_ref as PR                                                                 # noqa: E402

TRI = (np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64), np.array([[0, 1, 2]]))


@pytest.mark.parametrize("p,d2,q", [
    ((0.5, 0.5, 3.0), 9.0, (0.5, 0.5, 0.0)),                # above the interior
    ((1.0, -2.0, 0.0), 4.0, (1.0, 0.0, 0.0)),               # beyond edge AB, in the plane outside
    ((-1.0, 1.0, 1.0), 2.0, (0.0, 1.0, 0.0)),               # beyond edge CA
    ((2.0, 2.0, 0.0), 2.0, (1.0, 1.0, 0.0)),                # beyond edge BC
    ((-1.0, -1.0, 1.0), 3.0, (0.0, 0.0, 0.0)),              # beyond vertex A
    ((4.0, -1.0, 0.0), 5.0, (2.0, 0.0, 0.0)),               # beyond vertex B
    ((-1.0, 5.0, 2.0), 14.0, (0.0, 2.0, 0.0)),              # beyond vertex C
    ((1.0, 0.0, 0.0), 0.0, (1.0, 0.0, 0.0)),                # on an edge
    ((0.0, 2.0, 0.0), 0.0, (0.0, 2.0, 0.0)),                # on a vertex
])
def test_oracle_and_restatement_on_one_triangle(p, d2, q):
    dmin, D, C = PR.oracle(*TRI, [p])
    assert abs(dmin[0] - d2) < 1e-14 and np.allclose(C[0, 0], q, atol=1e-14)
    d32, k, q32, _ = PR.restate32(*TRI, [p])
    assert k[0] == 0 and abs(d32[0] - d2) <= 4 * PR.EPS * 25 and np.allclose(q32[0], q, atol=1e-6)


def test_oracle_points_on_faces_have_no_distance():
    v, f = PR.meshes()["2tp3"]
    rng = np.random.RandomState(1)
    w = rng.dirichlet((1, 1, 1), size=len(f))
    pts = (v.astype(np.float64)[f.astype(np.int64)] * w[:, :, None]).sum(1)
    dmin, D, _ = PR.oracle(v, f, pts)
    assert dmin.max() < 1e-28 and D[np.arange(len(f)), np.arange(len(f))].max() < 1e-28


def test_oracle_degenerate_face_is_its_longest_edge():
    v = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [0.25, 0.5, 0.0]], np.float64)
    pts = np.random.RandomState(2).standard_normal((50, 3)) * 2
    for face, ends in (([0, 1, 2], (0, 2)), ([1, 2, 0], (0, 2)), ([0, 0, 3], (0, 3)), ([3, 1, 1], (1, 3)), ([2, 2, 2], (2, 2))):
        dmin, _, _ = PR.oracle(v, np.array([face]), pts)
        q = PR._segment(pts[:, None], v[ends[0]][None, None], v[ends[1]][None, None])[:, 0]
        assert np.allclose(dmin, ((pts - q) ** 2).sum(1), rtol=0, atol=1e-14)
        d32, _, _, _ = PR.restate32(v, np.array([face]), pts)          # and so does the contract: a thin face is its edges
        assert np.isfinite(d32).all() and np.abs(d32 - dmin).max() <= 8 * PR.EPS * 36


def test_oracle_is_translation_invariant():
    v, f = PR.meshes()["seven"]
    pts = PR.query_points(v, f, 65, 3).astype(np.float64)
    t = np.array([0.5, -0.25, 2.0])
    a, b = PR.oracle(v, f, pts)[0], PR.oracle(v.astype(np.float64) + t, f, pts + t)[0]
    assert np.abs(a - b).max() < 1e-14


def test_restatement_vs_oracle_measures_the_tolerance():
    """the worst |d2_32 - d2_64| / (2^-23 R^2) over every case of the GPU test: printed, and recorded as point_mesh_ref.K_MEASURED
    (the GPU tolerance is 4 x it).  Also what the restatement promises besides: finite results, the reported face's true distance
    within the tolerance of the minimum, the closest point on that face."""
    ms = PR.meshes()
    worst = 0.0
    for key, name, pts in PR.cases():
        v, f = ms[name]
        R = PR.radius(v, pts)
        dmin, D, _ = PR.oracle(v, f, pts)
        d32, k, q32, _ = PR.restate32(v, f, pts)
        assert np.isfinite(d32).all() and np.isfinite(q32).all(), key
        ratio = float(np.abs(d32.astype(np.float64) - dmin).max() / (PR.EPS * R * R))
        print("%-16s R %.3g  worst ratio %.3f" % (key, R, ratio))
        worst = max(worst, ratio)
        i = np.arange(len(k))
        assert (D[i, k] - dmin).max() <= PR.K * PR.EPS * R * R, key
        on = np.diagonal(PR.oracle(v, f[k], q32.astype(np.float64))[1])
        assert np.sqrt(on.max()) <= PR.K * PR.EPS * R, key
    print("K_MEASURED = %.3f (recorded %.3f)" % (worst, PR.K_MEASURED))
    assert worst <= PR.K_MEASURED, "the recorded constant no longer covers the restatement: %.3f > %.3f" % (worst, PR.K_MEASURED)
    assert worst >= 0.5 * PR.K_MEASURED, "the recorded constant is stale: measured %.3f, recorded %.3f" % (worst, PR.K_MEASURED)


def test_restatement_ties_go_to_the_lowest_face():
    v, f = PR.cube()
    pts = PR.cube_points()
    d32, k, _, D = PR.restate32(v, f, pts)
    for i in range(len(pts)):
        assert k[i] == np.flatnonzero(D[i] == d32[i])[0]
    assert (np.sum(D == d32[:, None], axis=1) >= 2).sum() >= len(pts) // 2        # the points were chosen to tie
