"""dpf_knn where random input barely goes, bit for bit against tests/knn_ref.py (whose new inputs tests/test_knn_ref_cpu.py checks, with
the mutated restatements that show what a wrong kernel would change on them):

  * candidate ORDER: clouds sorted by descending distance, so that a lane's deferred queue fills and drains every few groups for the
    whole scan -- everywhere in a wave, and in some lanes beside idle ones (the partial drain: entries past a lane's count are +inf);
    long descending runs of EQUAL distances across drains and tile borders (the lowest index must win against a stale threshold);
  * the ENDS of the served range: squared distances that are fp32 subnormals, coordinates at +-2^61, 120 octaves in one cloud;
  * PAST ONE LAUNCH: 32769 slots, one more than dispatch::chunk_grid gives a launch, so the second launch's first slot b0 != 0 reaches
    every per-slot pointer (status, outputs, both sets);
  * the gradient of a SELF-search, where autograd adds the query's and the cloud's gradient into one leaf.

The other cut of chunk_grid, 2^22 workgroups of one slot, needs 2^30 queries; it stays with tests/test_chunk_dispatch_cpu.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import knn_ref as R                                                                          # noqa: E402
from test_gpu_knn import CAPS, call, guards_intact, inner, run, same_bits, serving, to      # noqa: E402

pytestmark = pytest.mark.gpu

M, N = 1025, 320                                    # four full tiles and a one-candidate tail; one full workgroup plus one wave
KS = (1, 5, 16, 32)                                 # one k under each capacity


def capacity(k, form):
    return CAPS[form] if form else min(c for c in CAPS.values() if c >= k)


def differing(got, want):
    """the slots in which any output differs: what an assertion message shows"""
    return sorted({int(b) for g, w in zip(got[:2], want[:2]) for b in np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).any((1, 2)))})


@functools.lru_cache(maxsize=None)
def order_case():
    query, cloud, hot = R.order_batch(M, N)
    return query, cloud, hot, [R.dist2(query[b], cloud[b]) for b in range(5)]


@functools.lru_cache(maxsize=None)
def order_traffic(cap):
    """(5, N) improvements of the order batch at one capacity, computed once"""
    return np.stack([R.improvements(d, cap) for d in order_case()[3]])


@pytest.mark.parametrize("k", KS)
def test_hot_cold_and_mixed_waves_against_sorted_clouds(k):
    """slots: every lane hot; every lane cold; even lanes hot; lanes 0-31 hot; one hot lane (37 of wave 1) -- R.order_batch.  The
    conditions are the REFERENCE's: a hot lane improves on >= 0.9 m candidates under an exact threshold, every other on <= 0.25 m."""
    query, cloud, hot, _ = order_case()
    want = R.knn_batch(query, cloud, k)
    assert (want[2] == 0).all()
    for form in [0] + serving(k):
        cap = capacity(k, form)
        count = order_traffic(cap)
        print("k %d form %d capacity %d: hot minimum %d, ordinary maximum %d, cold maximum %d of %d"
              % (k, form, cap, count[hot].min(), count[2:][~hot[2:]].max(), count[1].max(), M))
        assert count[hot].min() >= 0.9 * M and count[~hot].max() <= 0.25 * M, (k, form)
        got = run(query, cloud, k, False, form)
        assert same_bits(got, want), (k, form, [R.ORDER_SLOTS[b] for b in differing(got, want)])


@pytest.mark.parametrize("k", KS)
def test_descending_runs_of_equal_distances(k):
    """`shells`: from the origin the distances never increase, 97 % of neighbouring candidates tie and the longest run is 72 -- more
    than a queue holds; runs straddle the tile borders at 256 and 512, and a run ends exactly at 768 and at 1024"""
    cloud = R.shells(M)
    d = R.dist2(R.ORIGIN, cloud)[0]
    assert (np.diff(d) <= 0).all() and round(float((np.diff(d) == 0).mean()), 2) == 0.97 and R.longest_run(d) == 72
    assert d[255] == d[256] and d[511] == d[512] and d[767] > d[768] and d[1023] > d[1024] == 0
    rng = np.random.default_rng(3)
    query = np.concatenate([R.ORIGIN, rng.integers(-6, 7, size=(N - 1, 3)).astype(np.float32)])
    for q, exclude in ((query, False), (cloud[:N], True)):
        want = R.knn_batch(q[None], cloud[None], k, exclude)
        assert k == 1 or (np.diff(want[0], axis=2) == 0).mean() > 0.5
        dq = R.dist2(q, cloud)
        if exclude:
            dq[np.arange(N), np.arange(N)] = np.inf
        for form in [0] + serving(k):
            cap = capacity(k, form)
            count = R.improvements(dq, cap)
            print("k %d form %d capacity %d exclude %d: improvements of query 0 %d, maximum %d of %d" % (k, form, cap, exclude, count[0], count.max(), M))
            assert same_bits(run(q[None], cloud[None], k, exclude, form), want), (k, form, exclude)


@pytest.mark.parametrize("k", (1, 9, 32))
def test_subnormal_distances_the_bound_itself_and_120_octaves(k):
    n = 300
    kinds = ("tiny", "huge", "wide")
    pts = np.stack([R.make_range_cloud(kd, n, 5 + b) for b, kd in enumerate(kinds)])
    for exclude in (False, True):
        want = R.knn_batch(pts, pts, k, exclude)
        assert (want[2] == 0).all() and np.isfinite(want[0]).all()
        for form in [0] + serving(k):
            got = run(pts, pts, k, exclude, form)
            assert same_bits(got, want), (k, exclude, form, [kinds[b] for b in differing(got, want)])
    d = R.dist2(pts[0], pts[0])
    print("tiny: %.4f of the distances are positive subnormals" % R.subnormal_share(d))
    assert R.subnormal_share(d) > 0.9
    assert (pts[1] == R.LIMIT).any() and (pts[1] == -R.LIMIT).any() and R.dist2(pts[1], pts[1]).max() == np.float32(3 * 2.0 ** 124)


# ---- 32769 slots: the second launch ------------------------------------------------------------------------------------------------
B_PAST, LAUNCH = 32769, 32768


@functools.lru_cache(maxsize=None)
def past_case(exclude):
    """the batch, its restatement, and the poisoned batch's: the same but for the two refused slots"""
    query, cloud = R.launch_batch(B_PAST)
    want = R.knn_batch(query, cloud, 3, exclude)
    pq, pc = R.poison(query, cloud)
    bad = [LAUNCH - 1, LAUNCH]
    refused = [w.copy() for w in want]
    for b in bad:
        slot = R.knn(pq[b], pc[b], 3, exclude)
        assert slot[2] == R.REFUSED
        refused[0][b], refused[1][b], refused[2][b] = slot
    return query, cloud, want, pq, pc, refused


@pytest.mark.parametrize("exclude", (0, 1))
@pytest.mark.parametrize("form", (0, 4))
def test_32769_slots_take_a_second_launch(form, exclude):
    n, m, k = 2, 5, 3
    query, cloud, want, pq, pc, refused = past_case(bool(exclude))
    assert (want[2] == 0).all() and (np.diff(want[0], axis=2) == 0).any()
    q, c = to(query), to(cloud)
    rc, bufs = call(q, c, k, exclude, form)
    got = inner(bufs, B_PAST, n, k)
    assert rc == 0 and guards_intact(bufs)
    assert same_bits(got, want), differing(got, want)[:8]
    for b in (0, LAUNCH - 1, LAUNCH):                                                       # a slot of either launch: the bits it has alone
        assert same_bits([o[b:b + 1] for o in got], run(query[b:b + 1], cloud[b:b + 1], k, bool(exclude), form)), b
    rc, bufs = call(to(pq), to(pc), k, exclude, form)
    got = inner(bufs, B_PAST, n, k)
    assert rc == 0 and guards_intact(bufs)
    assert np.flatnonzero(got[2]).tolist() == [LAUNCH - 1, LAUNCH] and (got[2][[LAUNCH - 1, LAUNCH]] == R.REFUSED).all()
    assert np.flatnonzero(np.isnan(got[0]).any((1, 2))).tolist() == [LAUNCH - 1, LAUNCH] and np.isnan(got[0][[LAUNCH - 1, LAUNCH]]).all()
    assert np.flatnonzero((got[1] == -1).any((1, 2))).tolist() == [LAUNCH - 1, LAUNCH] and (got[1][[LAUNCH - 1, LAUNCH]] == -1).all()
    assert same_bits(got, refused), differing(got, refused)[:8]
    assert not np.array_equal(R.status_at_slot_mod(refused[2]), refused[2])                 # (a status written at b mod 32768 would differ)


# ---- the gradient of a self-search --------------------------------------------------------------------------------------------------
def test_self_search_gradient_sums_both_roles_into_one_leaf():
    """x (2, 130, 3), k = 5, dist = knn_points(x, x, k, exclude_self=True), loss = sum(w * dist).

    The bound.  tests/test_gpu_knn.py derives, for u = 2^-24: the query-role gradient of an entry is within 2 k u aq of float64 and
    the cloud-role gradient within 2 count u ac (aq, ac: the sums of the magnitude bounds of the entry's terms in each role; count:
    the number of lists the point appears in, at least 1).  Autograd then adds the two with ONE rounded addition, at most u of
    |gq + gc| <= aq + ac up to O(u).  Together |err| <= (2 k + 1) u aq + (2 count + 1) u ac."""
    from dpf_nets_amd.metrics import knn_points
    B, n, k = 2, 130, 5
    xs = np.stack([R.make_cloud(kd, n, 31 + 17 * b) for b, kd in enumerate(("gauss", "dup"))])
    w = np.random.default_rng(4).standard_normal((B, n, k)).astype(np.float32)
    index = R.knn_batch(xs, xs, k, True)[1]
    u = 2.0 ** -24
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for _ in range(3):
            x = to(xs).requires_grad_(True)
            dist, idx = knn_points(x, x, k, exclude_self=True)
            assert np.array_equal(idx.cpu().numpy(), index) and (idx != torch.arange(n, device=idx.device)[None, :, None]).all()
            (dist * to(w)).sum().backward()
            grads.append((x.grad.cpu().numpy(),))
        assert same_bits(grads[1], grads[0]) and same_bits(grads[2], grads[0])
        xcf = to(xs).transpose(1, 2).contiguous().requires_grad_(True)
        (knn_points(xcf, xcf, k, exclude_self=True, channels_first=True, return_index=False) * to(w)).sum().backward()
        assert xcf.grad.shape == (B, 3, n) and same_bits((xcf.grad.transpose(1, 2).cpu().numpy(),), grads[0])
    finally:
        torch.use_deterministic_algorithms(was)
    for b in range(B):
        gq, gc, aq, ac = R.grad(xs[b], xs[b], index[b], w[b])
        count = np.maximum(np.bincount(index[b].reshape(-1), minlength=n), 1)[:, None]
        bound = (2 * k + 1) * u * aq + (2 * count + 1) * u * ac
        err = np.abs(grads[0][0][b] - (gq + gc))
        print("slot %d: error / bound max %.3f (largest |gradient| %.3f)" % (b, (err / bound).max(), np.abs(gq + gc).max()))
        assert (bound > 0).all() and (err <= bound).all(), b
        assert np.abs(gq + gc).max() > 0.1 and np.abs(gc).max() > 0.1
