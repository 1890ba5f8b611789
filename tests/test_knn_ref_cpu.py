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


# ---- the inputs of tests/test_gpu_knn_edges.py: that they reach what they are for, and that a wrong kernel would show on them --------
def test_candidate_orders_load_the_queue_as_claimed_at_every_capacity():
    """hot lanes improve on >= 0.9 m candidates, ordinary and cold ones on <= 0.25 m, at each list capacity (the GPU test asserts
    the same at the capacity it runs)"""
    m, n = 1025, 320
    query, cloud, hot = R.order_batch(m, n)
    d0 = R.dist2(R.ORIGIN, cloud[0])[0]
    assert (np.diff(d0) < 0).all() and np.array_equal(cloud[1], cloud[0][::-1])              # strictly descending, and its reverse
    assert (np.sqrt((query[0].astype(np.float64) ** 2).sum(1)) <= 1e-3).all()
    assert hot.sum(1).tolist() == [n, 0, n // 2, n // 2, 1] and hot[4, 101]
    shuffled = R.dist2(query[0], R.make_cloud("gauss", m, 11))
    for cap in (4, 8, 16, 32):
        count = np.stack([R.improvements(R.dist2(query[b], cloud[b]), cap) for b in range(5)])
        print("capacity %2d: hot minimum %d, ordinary maximum %d, cold maximum %d, shuffled maximum %d of %d"
              % (cap, count[hot].min(), count[2:][~hot[2:]].max(), count[1].max(), R.improvements(shuffled, cap).max(), m))
        assert count[hot].min() >= 0.9 * m and count[~hot].max() <= 0.25 * m, cap
        assert (count[1] == cap).all()                                                      # ascending: the first `cap` and nothing after


def test_improvements_counts_insertions_under_an_exact_threshold():
    assert R.improvements(np.array([5.0, 4.0, 3.0, 2.0, 1.0]), 2) == 5
    assert R.improvements(np.array([1.0, 2.0, 3.0, 4.0, 5.0]), 2) == 2
    assert R.improvements(np.array([3.0, 3.0, 3.0, 3.0]), 2) == 2                            # strict: an equal distance is no improvement
    assert R.improvements(np.array([3.0, np.inf, 1.0, 2.0, 0.5]), 2) == 4                    # (+inf, the excluded one, never counts)
    assert R.improvements(np.array([[4.0, 3.0, 5.0, 1.0], [1.0, 1.0, 0.0, 0.0]]), 1).tolist() == [3, 2]


def test_shells_are_integer_distances_in_long_descending_runs():
    m = 1025
    cloud = R.shells(m)
    assert cloud.shape == (m, 3) and (cloud == np.round(cloud)).all() and np.abs(cloud).max() <= 6
    assert len({tuple(p) for p in cloud.tolist()}) == m
    d = R.dist2(R.ORIGIN, cloud)[0]
    assert (np.diff(d) <= 0).all() and d[-1] == 0 and (d == np.round(d)).all()
    assert round(float((np.diff(d) == 0).mean()), 2) == 0.97 and R.longest_run(d) == 72
    ends = np.concatenate([np.flatnonzero(np.diff(d)) + 1, [m]])
    for lo, hi in zip(np.concatenate([[0], ends[:-1]]), ends):
        run = cloud[lo:hi]                                                                  # inside a run: the lattice's own (x fastest) order
        key = (run[:, 2] * 13 + run[:, 1]) * 13 + run[:, 0]
        assert (np.diff(key) > 0).all()
    query = np.concatenate([R.ORIGIN, cloud[:7]])
    for k in (1, 5, 32):
        dist, index, _ = R.knn(query, cloud, k)
        wd, wi = R.brute_force(query, cloud, k)
        assert np.array_equal(index, wi) and np.array_equal(dist.astype(np.float64), wd)
    dist, index, _ = R.knn(cloud[:8], cloud, 32, True)
    wd, wi = R.brute_force(cloud[:8], cloud, 32, True)
    assert np.array_equal(index, wi) and np.array_equal(dist.astype(np.float64), wd)


def test_descending_and_huge_agree_with_float64_where_it_separates_the_neighbours():
    """(not `tiny`: float64 does not tie where fp32's subnormals do, so there is nothing to compare)"""
    query, cloud, _ = R.order_batch()
    q = np.concatenate([query[0][:4], query[2][1:4]])                                       # hot ones and ordinary ones
    dist, index, _ = R.knn(q, cloud[0], 9)
    wd, wi = R.brute_force(q, cloud[0], 10)
    clear = (np.diff(wd, axis=1) > 2.0 ** -20 * wd[:, 1:]).all(1)                            # fp32 error of a distance: a few 2^-24 of it
    assert clear.sum() >= 5 and np.array_equal(index[clear], wi[clear][:, :9])
    assert (np.abs(dist - wd[:, :9]) <= 2.0 ** -21 * wd[:, :9]).all()
    huge = R.make_range_cloud("huge", 300, 5)
    dist, index, status = R.knn(huge[:6], huge, 9, True)
    wd, wi = R.brute_force(huge[:6], huge, 10, True)
    clear = (np.diff(wd, axis=1) > 2.0 ** -20 * wd[:, 1:]).all(1)
    assert status == 0 and clear.sum() >= 4 and np.array_equal(index[clear], wi[clear][:, :9])
    assert (np.abs(dist - wd[:, :9]) <= 2.0 ** -21 * wd[:, :9]).all()


def test_the_ends_of_the_range_are_what_they_are_for():
    tiny, huge, wide = (R.make_range_cloud(kd, 300, 5) for kd in ("tiny", "huge", "wide"))
    assert np.array_equal(tiny, R.make_cloud("gauss", 300, 5) * np.float32(2.0 ** -70))
    assert (tiny.astype(np.float64) * 2.0 ** 70 == R.make_cloud("gauss", 300, 5)).all()      # (the scaling is exact)
    d = R.dist2(tiny, tiny)
    assert R.subnormal_share(d) > 0.99 and (d[~((d > 0) & (d < R.SUBNORMAL))] == 0).all()
    assert (np.diff(R.knn(tiny, tiny, 32, True)[0], axis=1) == 0).mean() > 0.01
    assert np.abs(huge).max() == R.LIMIT and (huge == R.LIMIT).any() and (huge == -R.LIMIT).any()
    dist, _, status = R.knn(huge, huge, 299, True)
    assert status == 0 and np.isfinite(dist).all() and dist.max() == np.float32(3 * 2.0 ** 124)
    assert np.abs(wide).max() > 2.0 ** 55 and np.abs(wide).min() < 2.0 ** -55 and R.knn(wide, wide, 32)[2] == 0


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_a_kernel_with_the_wrong_tie_rule_would_show():
    """highest index first among equals: on the lattice of the older tests, and on `shells` and `tiny`"""
    lat, sh, tiny = R.make_cloud("lattice", 300, 3), R.shells(1025), R.make_range_cloud("tiny", 300, 5)
    for cloud, query in ((lat, lat), (sh, np.concatenate([R.ORIGIN, sh[:9]])), (tiny, tiny)):
        for exclude in (False, True):
            assert not same(R.knn_highest_index_first(query, cloud, 5, exclude)[:2], R.knn(query, cloud, 5, exclude)[:2])
    g = R.make_cloud("gauss", 300, 3)                                                       # (and it is the tie rule alone that differs)
    assert same(R.knn_highest_index_first(g, g, 5, True), R.knn(g, g, 5, True))


def test_a_kernel_that_flushes_subnormals_would_show_on_tiny_and_nowhere_else():
    tiny, g = R.make_range_cloud("tiny", 300, 5), R.make_cloud("gauss", 300, 5)
    for exclude in (False, True):
        assert not same(R.knn_flushed(tiny, tiny, 9, exclude)[:2], R.knn(tiny, tiny, 9, exclude)[:2])
        assert same(R.knn_flushed(g, g, 9, exclude), R.knn(g, g, 9, exclude))
    assert (R.knn_flushed(tiny, tiny, 9)[0] == 0).all()


def test_a_status_written_at_the_slot_within_its_launch_would_show():
    query, cloud = R.launch_batch(B=32769, n=1, m=2)                                        # (the statuses need no more)
    q, c = R.poison(query, cloud)
    status = R.knn_batch(q, c, 1)[2]
    assert np.flatnonzero(status).tolist() == [32767, 32768]
    wrong = R.status_at_slot_mod(status)
    assert np.flatnonzero(wrong).tolist() == [0, 32767] and not np.array_equal(wrong, status)
    assert np.array_equal(R.status_at_slot_mod(status[:32768]), status[:32768])              # (one launch: nothing to tell apart)
