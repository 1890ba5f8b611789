"""tests/fps_ref.py -- the numpy restatement of dpf_fps's contract that the GPU tests compare with for equality -- against a plain
float64 brute force.  The inputs have small integer coordinates: every fp32 operation of the restatement is exact on them, so the two
must agree exactly, and they are full of exact ties, which is where the packed-key rule (lowest index) has to hold."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fps_ref as R                                                                          # noqa: E402


def brute(pts, k, start=0):
    """float64, every pairwise distance in a matrix, the first index of the maximum"""
    p = np.asarray(pts, dtype=np.float64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    sel, mind, index, radius2 = int(start), np.full(len(p), np.inf), [], []
    for _ in range(k):
        index.append(sel)
        mind = np.minimum(mind, d[:, sel])
        sel = int(np.flatnonzero(mind == mind.max())[0])
        radius2.append(mind.max())
    return np.array(index), np.array(radius2)


@pytest.mark.parametrize("n", (1, 2, 7, 64, 200))
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_lattice_clouds_agree_exactly_with_float64_brute_force(n, seed):
    pts = R.make_cloud("lattice", n, 10 * n + seed)
    start = seed % n
    index, radius2, status = R.fps(pts, n, start)
    bi, br = brute(pts, n, start)
    assert status == 0 and index.dtype == np.int32 and radius2.dtype == np.float32
    assert np.array_equal(index, bi)
    assert np.array_equal(radius2.astype(np.float64), br)
    if n >= 64:                                             # 9^3 positions, small counts: the clouds do hold exact ties
        d = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
        assert (np.sort(d[:, start])[1:] == np.sort(d[:, start])[:-1]).any()


def test_k_equal_n_on_distinct_points_is_a_permutation_and_the_radius_never_increases():
    for kind, n in (("gauss", 97), ("line", 64)):
        pts = R.make_cloud(kind, n, 5)
        assert len({tuple(p) for p in pts.tolist()}) == n
        index, radius2, status = R.fps(pts, n, 3)
        assert status == 0 and sorted(index.tolist()) == list(range(n))
        assert (radius2[1:] <= radius2[:-1]).all() and radius2[-1] == 0 and (radius2[:-1] > 0).all()


def test_the_radius_is_the_squared_hausdorff_distance_to_the_subset():
    pts = R.make_cloud("gauss", 150, 8)
    index, radius2, _ = R.fps(pts, 20)
    for t in (0, 7, 19):
        d = np.stack([R.dist2(pts, int(s)) for s in index[:t + 1]]).min(0)
        assert radius2[t] == d.max()
        d64 = ((pts.astype(np.float64)[:, None, :] - pts.astype(np.float64)[index[:t + 1]][None, :, :]) ** 2).sum(-1).min(1).max()
        assert abs(float(radius2[t]) - d64) <= 4 * 2.0 ** -24 * d64


def test_identical_points_give_the_start_then_index_zero():
    pts = R.make_cloud("same", 10, 1)
    index, radius2, status = R.fps(pts, 10, 4)
    assert status == 0 and index.tolist() == [4] + [0] * 9 and (radius2 == 0).all()


def test_duplicates_repeat_index_zero_once_every_position_is_taken():
    pts = R.make_cloud("dup", 40, 2)
    distinct = len({tuple(p) for p in pts.tolist()})
    index, radius2, _ = R.fps(pts, 40)
    assert len(set(index[:distinct].tolist())) == distinct and (radius2[:distinct - 1] > 0).all()
    assert (radius2[distinct - 1:] == 0).all() and (index[distinct:] == 0).all()


def test_the_start_is_honoured_and_a_bad_one_refused():
    pts = R.make_cloud("gauss", 30, 3)
    for s in (0, 11, 29):
        index, _, status = R.fps(pts, 5, s)
        assert status == 0 and index[0] == s
        assert index[1] == int(np.argmax(((pts.astype(np.float64) - pts[s]) ** 2).sum(-1)))
    for s in (-1, 30, 2 ** 31 - 1):
        index, radius2, status = R.fps(pts, 5, s)
        assert status == R.REFUSED and (index == -1).all() and np.isnan(radius2).all()


@pytest.mark.parametrize("poison", (np.nan, np.inf, -np.inf))
def test_non_finite_input_is_refused(poison):
    pts = R.make_cloud("gauss", 20, 4)
    pts[13, 1] = poison
    index, radius2, status = R.fps(pts, 6)
    assert status == R.REFUSED and (index == -1).all() and np.isnan(radius2).all()
    idx, r2, st = R.fps_batch(np.stack([R.make_cloud("gauss", 20, 4), pts]), 6)
    assert st.tolist() == [0, R.REFUSED] and (idx[0] >= 0).all() and (idx[1] == -1).all()


def test_finite_coordinates_that_overflow_are_not_refused():
    """differences and squares reach +inf; no NaN can arise (only sums of non-negative terms), and +inf is an ordinary maximum:
    ties at +inf go to the lowest index like any other tie"""
    big = np.float32(3.0e38)
    pts = np.array([[big, 0, 0], [-big, 0, 0], [0, 1, 0], [0, 2, 0], [1.0e20, 0, 0], [big, 1, 0]], dtype=np.float32)
    index, radius2, status = R.fps(pts, 6)
    assert status == 0 and not np.isnan(radius2).any()
    # from point 0: points 1 (difference overflows), 2, 3 (the square overflows) and 4 are all at +inf -> the lowest, 1; then 2, 3 and 4
    # are at +inf from both -> 2; then 0 / 1 / 4 / 5 are at +inf from 2, but mind keeps the minimum: 4 still +inf
    assert index.tolist()[:3] == [0, 1, 2] and np.isinf(radius2[0]) and np.isinf(radius2[1])
    assert sorted(index.tolist()) == list(range(6)) and radius2[-1] == 0 and (radius2[1:] <= radius2[:-1]).all()
