"""tests/knn_ref.py, the numpy restatement of dpf_knn, against a float64 brute force that sorts explicit (distance, index) pairs.  On
lattice clouds with small integer coordinates every fp32 operation of the restatement is exact, so the neighbour sets, their order,
the ties and the distances must be EQUAL; on Gaussian clouds the sets agree wherever float64 separates the k-th from the (k+1)-th
distance by more than fp32's rounding."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import knn_ref as R                                                                          # noqa: E402


@pytest.mark.parametrize("exclude", (False, True))
@pytest.mark.parametrize("n,m,k", ((40, 40, 1), (40, 40, 7), (17, 60, 32), (60, 17, 16), (33, 33, 32), (25, 25, 25)))
def test_lattice_clouds_equal_the_float64_brute_force(n, m, k, exclude):
    if exclude and k > m - 1:
        k = m - 1
    cloud = R.make_cloud("lattice", m, 3 * m + k)
    query = cloud if n == m else R.make_cloud("lattice", n, 5 * n + k)
    dist, index, status = R.knn(query, cloud, k, exclude)
    wd, wi = R.brute_force(query, cloud, k, exclude)
    assert status == 0 and dist.dtype == np.float32 and index.dtype == np.int32
    assert np.array_equal(index, wi) and np.array_equal(dist.astype(np.float64), wd)
    ties = sum(int((np.diff(row) == 0).any()) for row in dist)
    assert k == 1 or ties > 0                                                               # (the case does exercise the tie rule)
    if exclude and n == m:
        assert (index != np.arange(n)[:, None]).all()


def test_k_equal_to_the_number_of_eligible_candidates_lists_every_one_of_them():
    cloud = R.make_cloud("lattice", 20, 1)
    _, index, _ = R.knn(cloud, cloud, 20)
    assert (np.sort(index, axis=1) == np.arange(20)).all()
    _, index, _ = R.knn(cloud, cloud, 19, True)
    for i in range(20):
        assert sorted(index[i].tolist()) == [j for j in range(20) if j != i]


def test_duplicates_and_the_exclusion_by_index():
    cloud = R.make_cloud("gauss", 30, 2)
    cloud[11] = cloud[4]                                                                    # a duplicate of point 4 at index 11
    dist, index, _ = R.knn(cloud, cloud, 3)
    assert index[4, :2].tolist() == [4, 11] and index[11, :2].tolist() == [4, 11] and (dist[[4, 11], :2] == 0).all()
    dist, index, _ = R.knn(cloud, cloud, 3, True)
    assert index[4, 0] == 11 and index[11, 0] == 4 and dist[4, 0] == 0 and dist[11, 0] == 0   # the duplicate stays, at distance 0
    assert np.array_equal(R.brute_force(cloud, cloud, 3, True)[1][[4, 11], 0], [11, 4])
    same = R.make_cloud("same", 12, 5)
    dist, index, _ = R.knn(same, same, 5)
    assert (dist == 0).all() and (index == np.arange(5)).all()
    dist, index, _ = R.knn(same, same, 5, True)
    for i in range(12):
        assert index[i].tolist() == [j for j in range(6) if j != i][:5]


def test_gaussian_clouds_agree_with_float64_where_it_separates_the_neighbours():
    query, cloud = R.make_cloud("gauss", 50, 8), R.make_cloud("gauss", 300, 9)
    dist, index, _ = R.knn(query, cloud, 9)
    wd, wi = R.brute_force(query, cloud, 10)
    clear = np.diff(wd, axis=1).min(1) > 1e-5                                               # fp32 error of a distance of ~10: ~1e-6
    assert clear.sum() >= 40 and np.array_equal(index[clear], wi[clear][:, :9])
    assert np.abs(dist - wd[:, :9]).max() < 1e-5 and (np.diff(dist, axis=1) >= 0).all()


def test_refusal():
    cloud = R.make_cloud("gauss", 10, 1)
    for where in ("query", "cloud"):
        for value in (np.nan, np.inf, -np.inf, 2.0 ** 62, -(2.0 ** 62)):
            q, c = cloud.copy(), cloud.copy()
            (q if where == "query" else c)[3, 1] = value
            dist, index, status = R.knn(q, c, 4)
            assert status == R.REFUSED and np.isnan(dist).all() and (index == -1).all() and dist.shape == (10, 4)
    ok = cloud.copy()
    ok[3, 1] = 2.0 ** 61                                                                    # the bound itself is served, and nothing overflows
    ok[4, 1] = -(2.0 ** 61)
    dist, index, status = R.knn(ok, ok, 9, True)
    assert status == 0 and np.isfinite(dist).all() and dist.max() == np.float32(2.0 ** 124)


def test_spacing_and_gradient_formulas():
    g = R.grid(5, 4, 3)
    mean, cv = R.spacing(g, 1)
    assert mean == 1.0 and cv == 0.0                                                        # every lattice point has a neighbour at 1
    rng = np.random.default_rng(0)
    clumped = np.concatenate([rng.standard_normal((30, 3)) * 0.01, rng.standard_normal((30, 3))]).astype(np.float32)
    assert R.spacing(clumped, 1)[1] > 0.5
    # the gradient against central differences of sum(g * d) in float64, the indices held constant
    q, c = rng.standard_normal((6, 3)), rng.standard_normal((9, 3))
    index = R.knn(q.astype(np.float32), c.astype(np.float32), 3)[1]
    w = rng.standard_normal((6, 3))
    f = lambda q, c: (w * ((q[:, None, :] - c[index]) ** 2).sum(-1)).sum()                   # noqa: E731
    gq, gc, aq, ac = R.grad(q, c, index, w)
    h = 1e-6
    for arr, got in ((q, gq), (c, gc)):
        for at in ((0, 0), (3, 2), (5, 1)):
            up, dn = arr.copy(), arr.copy()
            up[at] += h
            dn[at] -= h
            num = (f(up, c) - f(dn, c)) / (2 * h) if arr is q else (f(q, up) - f(q, dn)) / (2 * h)
            assert abs(num - got[at]) < 1e-6
    assert (aq >= np.abs(gq)).all() and (ac >= np.abs(gc)).all()
