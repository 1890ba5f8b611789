"""dpf_normals (and the dpf_knn tables it consumes) where tests/test_gpu_normals.py does not go, against tests/normals_ref.py: cov and
flag bit for bit, the vector and the eigenvalues under the four 2^-46 bounds of that file.

  * PAST ONE LAUNCH: 32769 slots, one more than dispatch::chunk_grid gives a launch, so the second launch's first slot b0 != 0 reaches
    every per-slot pointer: the cloud, the index rows, the four outputs and the per-slot viewpoint;
  * SMALL SCALES: clouds of gauss x 2^-70 and gauss x 2^-135 -- the second's fp32 coordinates are subnormal, and every one of its
    squared distances underflows to 0 in dpf_knn, so its tables are the lowest indices: pinned against tests/knn_ref.py as well.

The other cut of chunk_grid, 2^22 workgroups of one slot, needs 2^30 points; it stays with tests/test_chunk_dispatch_cpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import knn_ref as KR                                                                         # noqa: E402
import normals_ref as R                                                                      # noqa: E402
from test_gpu_normals import hold_bounds, raw, run, same_bits, to                            # noqa: E402

pytestmark = pytest.mark.gpu

B_PAST, LAUNCH = 32769, 32768


def knn_table(query, cloud, k):
    """the device's (dist, index, status) as numpy"""
    from dpf_nets_amd.metrics.knn import knn_index
    return tuple(o.cpu().numpy() for o in knn_index(to(query), to(cloud), k))


def reference(clouds, index):
    """every neighbourhood of the batch at once: (centroid (B, n, 3), cov (B, n, 6))"""
    B, n, k = index.shape
    pts = clouds[np.arange(B)[:, None, None], index]                                         # (B, n, k, 3)
    centroid, cov = R.covariance(pts.reshape(B * n, k, 3))
    return centroid.reshape(B, n, 3), cov.reshape(B, n, 6)


@pytest.mark.parametrize("k", (3, 5))
def test_32769_slots_take_a_second_launch(k):
    n, m = 2, 5
    rng = np.random.default_rng(20 + k)
    clouds = rng.standard_normal((B_PAST, m, 3)).astype(np.float32)
    dist, index, status = knn_table(clouds[:, :n], clouds, k)
    assert (status == 0).all() and np.array_equal(index[[0, LAUNCH - 1, LAUNCH]], KR.knn_batch(clouds[[0, LAUNCH - 1, LAUNCH], :n],
                                                                                                clouds[[0, LAUNCH - 1, LAUNCH]], k)[1])
    centroid, cov = reference(clouds, index)
    plain = run(clouds, index)
    assert (plain[3] == 0).all() and same_bits([plain[2]], [cov])
    assert not R.canonical_flip(plain[0].reshape(-1, 3)).any()
    hold_bounds(plain, "B 32769 k %d" % k)

    # a viewpoint per slot: random ones, then slot 32767's in front of its canonical normals and slot 32768's behind point 0's
    view = (5.0 * rng.standard_normal((B_PAST, 3))).astype(np.float32)
    view[LAUNCH - 1] = (centroid[LAUNCH - 1].mean(0) + 100.0 * plain[0][LAUNCH - 1].sum(0)).astype(np.float32)
    view[LAUNCH] = (centroid[LAUNCH, 0] - 100.0 * plain[0][LAUNCH, 0]).astype(np.float32)
    want_normal = R.orient(plain[0].reshape(-1, 3), centroid.reshape(-1, 3), np.repeat(view, n, axis=0)).reshape(B_PAST, n, 3)
    flipped = (want_normal != plain[0]).any(-1)
    assert flipped[LAUNCH, 0] and not flipped[LAUNCH - 1].any() and 0.2 < flipped.mean() < 0.8
    bad = index.copy()
    bad[LAUNCH, 1, k - 1] = m                                                               # one index out of range: that point alone
    got = run(clouds, bad, view)
    want_flag = np.zeros((B_PAST, n), dtype=np.int32)
    want_flag[LAUNCH, 1] = 1
    ok = want_flag == 0
    assert np.array_equal(got[3], want_flag) and all(np.isnan(o[LAUNCH, 1]).all() for o in got[:3])
    assert np.array_equal(raw(got[0][ok]), raw(want_normal[ok])), np.flatnonzero((got[0] != want_normal).any(-1) & ok)[:8]
    assert np.array_equal(raw(got[1][ok]), raw(plain[1][ok])) and np.array_equal(raw(got[2][ok]), raw(cov[ok]))
    for b in (0, LAUNCH - 1, LAUNCH):                                                       # a slot of either launch: the bits it has alone
        assert same_bits([o[b:b + 1] for o in got], run(clouds[b:b + 1], bad[b:b + 1], view[b])), b


@pytest.mark.parametrize("k", (3, 8, 32))
def test_tiny_and_subnormal_clouds(k):
    n, m = 65, 257
    clouds = np.stack([R.make_cloud(kd, m, 200 + 17 * b + k) for b, kd in enumerate(R.SMALL_KINDS)])
    query = np.stack([R.make_cloud(kd, n, 300 + 17 * b + k) for b, kd in enumerate(R.SMALL_KINDS)])
    sub = (np.abs(clouds[1]) < 2.0 ** -126) & (clouds[1] != 0)
    assert sub.mean() > 0.99 and (np.abs(clouds[0]) >= 2.0 ** -126).mean() > 0.99
    want_knn = KR.knn_batch(query, clouds, k)
    assert KR.subnormal_share(KR.dist2(query[0], clouds[0])) > 0.9 and (want_knn[0][1] == 0).all()
    assert (want_knn[1][1] == np.arange(k)).all()                                            # every distance underflows: the lowest indices
    table = knn_table(query, clouds, k)
    assert same_bits(table, want_knn), [kd for b, kd in enumerate(R.SMALL_KINDS) if not same_bits([t[b] for t in table], [w[b] for w in want_knn])]
    index = table[1]
    got = run(clouds, index)
    want = R.normals_batch(clouds, index)
    assert (got[3] == 0).all() and same_bits(got[2:], want[2:]), k
    assert (np.abs(got[2]).max((1, 2)) > 0).all() and np.abs(got[2][0]).max() < 2.0 ** -130 and np.abs(got[2][1]).max() < 2.0 ** -255
    assert not R.canonical_flip(got[0].reshape(-1, 3)).any()
    for b, kd in enumerate(R.SMALL_KINDS):
        hold_bounds([o[b] for o in got], "k %d %s" % (k, kd))
    # the same points in neighbourhoods of their own (not all the lowest indices): a self-search table of the tiny cloud, and the
    # subnormal cloud under the tiny cloud's table
    own = knn_table(clouds[:1, :n], clouds[:1], k)[1]
    both = run(clouds, np.concatenate([own, own]))
    assert (both[3] == 0).all() and same_bits(both[2:], R.normals_batch(clouds, np.concatenate([own, own]))[2:])
    for b, kd in enumerate(R.SMALL_KINDS):
        hold_bounds([o[b] for o in both], "k %d %s, the tiny cloud's table" % (k, kd))
