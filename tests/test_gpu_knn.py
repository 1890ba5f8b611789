"""dpf_knn on the GPU against the numpy restatement of its contract (tests/knn_ref.py; the restatement itself is checked against a
float64 brute force in tests/test_knn_ref_cpu.py).  The contract is bit-defined, so dist, index and status are compared for
EQUALITY; the only tolerances in this file belong to the Python surface's tensor arithmetic (the gradient and the spacing
statistic) and are derived where they are used."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import knn_ref as R                                                                          # noqa: E402

pytestmark = pytest.mark.gpu

KMAX = 32
CAPS = {1: 4, 2: 8, 3: 16, 4: 32}                   # forced form -> list capacity
SENTINEL_I, SENTINEL_F, GUARD = -7777, -12345.5, 256
KINDS = ("gauss", "lattice", "dup")                 # the slots of a batch of 3: tie-free, full of ties, duplicates at distance 0


def dev():
    return torch.device("cuda", 0)


def L():
    from dpf_nets_amd import _lib
    return _lib


def K():
    from dpf_nets_amd.metrics import knn
    return knn


def serving(k):
    return [f for f, cap in CAPS.items() if cap >= k]


def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def run(query, cloud, k, exclude=False, form=0, channels_first=False):
    """numpy or tensor sets -> numpy dist, index, status"""
    q = to(query) if isinstance(query, np.ndarray) else query
    c = to(cloud) if isinstance(cloud, np.ndarray) else cloud
    return tuple(o.cpu().numpy() for o in K().knn_index(q, c, k, exclude, channels_first, form))


def raw(v):
    return np.ascontiguousarray(v).view(np.uint8)


def same_bits(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(raw(g), raw(w)) for g, w in zip(got, want))


def batch(n, seed, kinds=KINDS):
    return np.stack([R.make_cloud(kd, n, seed + 17 * b) for b, kd in enumerate(kinds)])


# k: either side of every list capacity; m: "every candidate is a neighbour" and the LDS tile's edges; n: the lane, wave and workgroup
# edges.  The whole product, three slots a call.
@pytest.mark.parametrize("k", (1, 2, 4, 5, 8, 9, 16, 17, 32))
def test_sizes_at_the_kernel_edges(k):
    for m in (k, 255, 256, 257, 513):
        cloud = batch(m, 1000 * k + m)
        for n in (1, 63, 64, 65, 257):
            query = cloud[:, :n] if n <= m and (n + m) % 2 else batch(n, 7000 * k + n)       # (a self-search where it fits, else apart)
            for exclude in ((False, True) if m > k else (False,)):
                want = R.knn_batch(query, cloud, k, exclude)
                assert (want[2] == 0).all()
                got = run(query, cloud, k, exclude)
                assert same_bits(got, want), (k, m, n, exclude)
                if n == 257 or m == 513:                                                    # every forced capacity >= k gives form 0's bits
                    for form in serving(k):
                        assert same_bits(run(query, cloud, k, exclude, form), want), (k, m, n, exclude, form)


def test_two_clouds_of_2048_points_k_16():
    pts = batch(2048, 5, ("gauss", "lattice"))
    want = R.knn_batch(pts, pts, 16, True)
    assert same_bits(run(pts, pts, 16, True), want)
    assert same_bits(run(pts, pts, 16, True, 4), want)


@pytest.mark.parametrize("k", (1, 4, 9, 32))
def test_ties(k):
    n = 300
    lat = R.make_cloud("lattice", n, 3)[None]                                               # 729 positions at most: repeats and equal distances
    for exclude in (False, True):
        want = R.knn_batch(lat, lat, k, exclude)
        assert k == 1 or (np.diff(want[0], axis=2) == 0).any()
        for form in [0] + serving(k):
            assert same_bits(run(lat, lat, k, exclude, form), want), (exclude, form)
    same = R.make_cloud("same", n, 4)[None]
    dist, index, status = run(same, same, k)
    assert (dist == 0).all() and (index == np.arange(k)).all() and status[0] == 0
    dist, index, status = run(same, same, k, True)
    assert (dist == 0).all() and status[0] == 0
    for i in (0, 1, k - 1, k, k + 1, n - 1):                                                # 0..k with i removed
        assert index[0, i].tolist() == [j for j in range(k + 1) if j != i][:k], i
    assert same_bits((dist, index, status), R.knn_batch(same, same, k, True))


def test_layouts_strides_a_broadcast_cloud_and_shared_memory():
    n, m, k, B = 130, 333, 6, 3
    qs, cs = batch(n, 40), batch(m, 50)
    want = R.knn_batch(qs, cs, k)
    q, c = to(qs), to(cs)
    assert same_bits(run(q, c, k), want)
    qcf, ccf = q.transpose(1, 2).contiguous(), c.transpose(1, 2).contiguous()               # (B, 3, N)
    assert same_bits(run(qcf, ccf, k, channels_first=True), want)
    assert same_bits(run(q.transpose(1, 2), ccf, k, channels_first=True), want)             # a (B, 3, N) view of point-major memory
    big = torch.full((2 * B + 1, m + 9, 5), float("nan"), device=dev())                     # anything read outside the slice would refuse
    view = big[1::2, 4:4 + m, 1:4]
    view.copy_(c)
    assert not view.is_contiguous() and same_bits(run(q, view, k), want)
    bigq = torch.full((B + 2, 3, 2 * n + 6), float("nan"), device=dev())
    viewq = bigq[1:1 + B, :, 3:3 + 2 * n:2]
    viewq.copy_(qcf)
    assert same_bits(run(viewq, ccf, k, channels_first=True), want)
    one = c[1:2].expand(B, m, 3)                                                            # cloud stride 0
    assert one.stride(0) == 0
    assert same_bits(run(q, one, k), R.knn_batch(qs, np.repeat(cs[1:2], B, axis=0), k))
    oneq = q[2:3].expand(B, n, 3)
    assert same_bits(run(oneq, c, k, True), R.knn_batch(np.repeat(qs[2:3], B, axis=0), cs, k, True))
    for exclude in (False, True):                                                           # query and cloud: the same memory
        assert same_bits(run(c, c, k, exclude), R.knn_batch(cs, cs, k, exclude)), exclude
    assert same_bits(run(c[:, :n], c, k, True), R.knn_batch(cs[:, :n], cs, k, True))        # overlapping views of it


def test_a_slot_gives_the_same_bits_alone_first_and_last_of_70():
    n, m, k = 200, 300, 7
    rng = np.random.default_rng(5)
    mq, mc = R.make_cloud("gauss", n, 90), R.make_cloud("dup", m, 91)
    want = R.knn_batch(mq[None], mc[None], k, True)
    oq, oc = rng.standard_normal((69, n, 3)).astype(np.float32), rng.standard_normal((69, m, 3)).astype(np.float32)
    assert same_bits(run(mq[None], mc[None], k, True), want)
    first = run(np.concatenate([mq[None], oq[:2]]), np.concatenate([mc[None], oc[:2]]), k, True)
    last = run(np.concatenate([oq, mq[None]]), np.concatenate([oc, mc[None]]), k, True)
    assert same_bits([o[:1] for o in first], want) and same_bits([o[-1:] for o in last], want)
    assert (last[2] == 0).all()
    for b in (0, 35, 68):
        assert same_bits([o[b:b + 1] for o in last], R.knn_batch(oq[b:b + 1], oc[b:b + 1], k, True)), b


@pytest.mark.parametrize("form", (0, 4))
def test_refused_slots_touch_no_neighbour(form):
    n, m, k = 300, 600, 5                                                                   # two workgroups of queries, three tiles
    qs = np.stack([R.make_cloud("gauss", n, 60 + b) for b in range(8)])
    cs = np.stack([R.make_cloud("gauss", m, 80 + b) for b in range(8)])
    qs[1, n - 1, 2] = np.nan                        # a query of the SECOND workgroup: the first must refuse its rows too
    cs[3, m // 2, 0] = -np.inf
    cs[4, m - 1, 1] = 2.0 ** 62
    qs[6, 0, 0] = -(2.0 ** 62)
    qs[7, 5, 1] = 2.0 ** 61                         # the bound itself is served
    want = R.knn_batch(qs, cs, k)
    assert want[2].tolist() == [0, -1, 0, -1, -1, 0, -1, 0]
    got = run(qs, cs, k, False, form)
    assert same_bits(got, want)
    bad = [1, 3, 4, 6]
    assert np.isnan(got[0][bad]).all() and (got[1][bad] == -1).all() and np.isfinite(got[0][[0, 2, 5, 7]]).all()
    clean_q, clean_c = qs[[0, 2, 5, 7]], cs[[0, 2, 5, 7]]                                    # the neighbours' bits without the refused slots
    assert same_bits([o[[0, 2, 5, 7]] for o in got], run(clean_q, clean_c, k, False, form))


def guarded(count, dtype, sentinel):
    buf = torch.full((GUARD + count + GUARD,), sentinel, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + count]


def call(q, c, k, exclude=0, form=0, want_status=True):
    """the C entry itself on dense (B, n, 3) / (B, m, 3) tensors, every output between sentinel-filled guards"""
    lib, B, n, m = L().lib(), q.shape[0], q.shape[1], c.shape[1]
    dbuf, dist = guarded(B * n * k, torch.float32, SENTINEL_F)
    ibuf, index = guarded(B * n * k, torch.int32, SENTINEL_I)
    sbuf, status = guarded(B, torch.int32, SENTINEL_I)
    rc = lib.dpf_knn(B, n, q.data_ptr(), n * 3, 3, 1, m, c.data_ptr(), m * 3, 3, 1, k, exclude, form, dist.data_ptr(), index.data_ptr(),
                     status.data_ptr() if want_status else None, L().current_stream())
    torch.cuda.synchronize()
    return rc, [b.cpu().numpy() for b in (dbuf, ibuf, sbuf)]


def inner(bufs, B, n, k):
    return bufs[0][GUARD:-GUARD].reshape(B, n, k), bufs[1][GUARD:-GUARD].reshape(B, n, k), bufs[2][GUARD:-GUARD]


def guards_intact(bufs):
    return all((b[:GUARD] == s).all() and (b[-GUARD:] == s).all() for b, s in zip(bufs, (SENTINEL_F, SENTINEL_I, SENTINEL_I)))


@pytest.mark.parametrize("n,m,k", ((1, 5, 5), (65, 257, 3), (257, 300, 17), (300, 64, 32)))
def test_nothing_is_written_outside_the_outputs_and_a_null_status_is_accepted(n, m, k):
    B = 3
    qs, cs = batch(n, 70), batch(m, 71)
    cs[2, 0, 0] = np.nan                                                                    # (a refused slot's fill stays inside too)
    want = R.knn_batch(qs, cs, k)
    q, c = to(qs), to(cs)
    for form in [0] + serving(k):
        rc, bufs = call(q, c, k, 0, form)
        assert rc == 0 and guards_intact(bufs) and same_bits(inner(bufs, B, n, k), want), (n, form)
        rc, bufs = call(q, c, k, 0, form, want_status=False)
        assert rc == 0 and guards_intact(bufs) and (bufs[2] == SENTINEL_I).all(), (n, form)
        assert same_bits(inner(bufs, B, n, k)[:2], want[:2]), (n, form)


def test_return_codes():
    lib, st = L().lib(), L().current_stream()
    t = to(R.make_cloud("gauss", 40, 1)[None])
    dbuf, dist = guarded(40 * KMAX, torch.float32, SENTINEL_F)
    ibuf, index = guarded(40 * KMAX, torch.int32, SENTINEL_I)

    def rc(B=1, n=40, q=t.data_ptr(), m=40, c=t.data_ptr(), k=4, ex=0, form=0, d=dist.data_ptr(), i=index.data_ptr()):
        return lib.dpf_knn(B, n, q, n * 3, 3, 1, m, c, m * 3, 3, 1, k, ex, form, d, i, None, st)

    assert lib.dpf_knn_max_k() == KMAX
    assert rc(B=0) == 0                                                                     # nothing to do, nothing launched
    for bad in (dict(B=-1), dict(n=0), dict(m=0), dict(k=0), dict(m=10, k=11), dict(m=10, k=10, ex=1), dict(form=-1), dict(form=5),
                dict(q=None), dict(c=None), dict(d=None), dict(i=None)):
        assert rc(**bad) == -1, bad
    assert rc(k=KMAX + 1) == -2                                                             # above the largest list
    for k, form in ((5, 1), (9, 2), (17, 3), (32, 3)):
        assert rc(k=k, form=form) == -2, (k, form)                                          # a forced capacity below k
    torch.cuda.synchronize()
    assert (dbuf.cpu().numpy() == SENTINEL_F).all() and (ibuf.cpu().numpy() == SENTINEL_I).all()
    assert rc(m=10, k=10) == 0 and rc(m=10, k=9, ex=1) == 0 and rc(k=KMAX, form=4) == 0
    torch.cuda.synchronize()


def test_three_runs_give_identical_bits():
    pts = batch(1500, 3)
    runs = [run(pts, pts, 12, True) for _ in range(3)]
    assert same_bits(runs[1], runs[0]) and same_bits(runs[2], runs[0])


@pytest.mark.parametrize("n,m", ((257, 513), (1000, 300)))
def test_k_1_equals_the_pinned_chamfer_kernel_both_ways(n, m):
    """finite, in-range clouds: dpf_nndistance's result / result_i, and result2 / result2_i with the sets swapped, bit for bit"""
    B = 3
    a, b = batch(n, 11), batch(m, 12)
    ta, tb = to(a), to(b)
    r1, r2 = torch.empty((B, n), device=dev()), torch.empty((B, m), device=dev())
    i1, i2 = torch.empty((B, n), dtype=torch.int32, device=dev()), torch.empty((B, m), dtype=torch.int32, device=dev())
    assert L().lib().dpf_nndistance(B, n, ta.data_ptr(), m, tb.data_ptr(), r1.data_ptr(), i1.data_ptr(), r2.data_ptr(), i2.data_ptr(),
                                    L().current_stream()) == 0
    fwd, bwd = run(ta, tb, 1), run(tb, ta, 1)
    assert same_bits((fwd[0][:, :, 0], fwd[1][:, :, 0]), (r1.cpu().numpy(), i1.cpu().numpy()))
    assert same_bits((bwd[0][:, :, 0], bwd[1][:, :, 0]), (r2.cpu().numpy(), i2.cpu().numpy()))


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_knn_points_shapes_dtypes_and_errors():
    from dpf_nets_amd.metrics import knn_points
    qs, cs = batch(50, 1), batch(80, 2)
    want = R.knn_batch(qs, cs, 6)
    dist, index = knn_points(to(qs), to(cs), 6)
    assert dist.shape == (3, 50, 6) and dist.dtype == torch.float32 and index.shape == (3, 50, 6) and index.dtype == torch.int64
    assert np.array_equal(raw(dist.cpu().numpy()), raw(want[0])) and np.array_equal(index.cpu().numpy(), want[1].astype(np.int64))
    only = knn_points(to(qs), to(cs), 6, return_index=False)
    assert torch.is_tensor(only) and torch.equal(only, dist)
    dcf, icf = knn_points(to(qs).transpose(1, 2).contiguous(), to(cs).transpose(1, 2).contiguous(), 6, channels_first=True)
    assert torch.equal(dcf, dist) and torch.equal(icf, index)
    dx, ix = knn_points(to(cs), to(cs), 6, exclude_self=True)
    assert np.array_equal(ix.cpu().numpy(), R.knn_batch(cs, cs, 6, True)[1]) and (ix != torch.arange(80, device=dev())[None, :, None]).all()
    with pytest.raises(RuntimeError):
        knn_points(torch.from_numpy(qs), torch.from_numpy(cs), 6)
    with pytest.raises(RuntimeError):
        knn_points(to(qs).double(), to(cs).double(), 6)
    with pytest.raises(RuntimeError):
        knn_points(to(qs)[:2], to(cs), 6)
    for k, ex in ((0, False), (81, False), (80, True), (33, False)):
        with pytest.raises(ValueError):
            knn_points(to(qs), to(cs), k, exclude_self=ex)
    bad = cs.copy()
    bad[1, 7, 0] = np.nan
    with pytest.raises(ValueError, match="slot 1 of 3"):
        knn_points(to(qs), to(bad), 6)
    badq = qs.copy()
    badq[2, 0, 1] = 2.0 ** 62
    with pytest.raises(ValueError, match="slot 2 of 3"):
        knn_points(to(badq), to(cs), 6)


def test_knn_gather_is_torch_gather():
    from dpf_nets_amd.metrics import knn_points, knn_gather
    qs, cs = batch(33, 3), batch(70, 4)
    feats = torch.randn((3, 70, 5), device=dev(), generator=torch.Generator(device=dev()).manual_seed(1))
    _, index = knn_points(to(qs), to(cs), 4)
    got = knn_gather(feats, index)
    assert got.shape == (3, 33, 4, 5)
    for s in range(4):
        assert torch.equal(got[:, :, s], torch.gather(feats, 1, index[:, :, s, None].expand(-1, -1, 5)))
    near = knn_gather(to(cs), index)                                                        # the neighbours themselves
    assert np.array_equal(near.cpu().numpy(), np.stack([cs[b][index[b].cpu().numpy()] for b in range(3)]))


def test_gradients_against_float64_and_bit_equal_repeats_under_deterministic_mode():
    """B = 2, n = 65, m = 130, k = 5, loss = sum(w * dist) so that the incoming gradient is w exactly.

    The bound, from the operation count in fp32 (u = 2^-24).  An entry of a gradient is a sum of T terms 2 w (q - c): per term one
    rounded subtraction (error <= u |q - c| <= u (|q| + |c|)), an exact doubling and one rounded product -- at most 2 u (1 + u) of
    the term's magnitude bound 2 |w| (|q| + |c|); then T - 1 rounded additions, each at most u of a partial sum that the sum S of the
    magnitude bounds dominates.  Together (T + 1) u (1 + O(u)) S, whatever the order of the additions; T >= 1 gives T + 1 <= 2 T, and
    the bound used is 2 T u S: c = 2 in c * k * 2^-24 * sum|terms|.  T = k for a query; for a cloud point T is the number of lists
    it appears in (at least 1 in the bound, so that an unlisted point must get exactly 0)."""
    from dpf_nets_amd.metrics import knn_points
    B, n, m, k = 2, 65, 130, 5
    qs, cs = batch(n, 21, ("gauss", "dup")), batch(m, 22, ("gauss", "dup"))
    w = np.random.default_rng(2).standard_normal((B, n, k)).astype(np.float32)
    index = R.knn_batch(qs, cs, k)[1]
    u = 2.0 ** -24
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for _ in range(3):
            q, c = to(qs).requires_grad_(True), to(cs).requires_grad_(True)
            dist, idx = knn_points(q, c, k)
            assert np.array_equal(idx.cpu().numpy(), index) and not idx.requires_grad
            (dist * to(w)).sum().backward()
            grads.append((q.grad.cpu().numpy(), c.grad.cpu().numpy()))
        assert same_bits(grads[1], grads[0]) and same_bits(grads[2], grads[0])
        qcf, ccf = to(qs).transpose(1, 2).contiguous().requires_grad_(True), to(cs).transpose(1, 2).contiguous().requires_grad_(True)
        (knn_points(qcf, ccf, k, channels_first=True, return_index=False) * to(w)).sum().backward()
        assert qcf.grad.shape == (B, 3, n) and ccf.grad.shape == (B, 3, m)
        assert same_bits((qcf.grad.transpose(1, 2).cpu().numpy(), ccf.grad.transpose(1, 2).cpu().numpy()), grads[0])
    finally:
        torch.use_deterministic_algorithms(was)
    gq, gc = grads[0]
    for b in range(B):
        wq, wc, aq, ac = R.grad(qs[b], cs[b], index[b], w[b])
        count = np.maximum(np.bincount(index[b].reshape(-1), minlength=m), 1)[:, None]
        eq, ec = np.abs(gq[b] - wq), np.abs(gc[b] - wc)
        print("slot %d: query error / bound max %.3f, cloud error / bound max %.3f"
              % (b, (eq / np.maximum(2 * k * u * aq, 1e-300)).max(), (ec / np.maximum(2 * count * u * ac, 1e-300)).max()))
        assert (eq <= 2 * k * u * aq).all() and (ec <= 2 * count * u * ac).all(), b
        assert np.abs(wq).max() > 0.1 and np.abs(wc).max() > 0.1


def test_neighbour_spacing_against_the_restatement_and_zero_cv_on_a_lattice():
    """Tolerance.  The k-th squared distances are the kernel's bits on both sides; then float64: a correctly rounded root per point,
    and sums of n non-negative terms, each within n * 2^-53 relative whatever their order.  The mean carries n * 2^-53; a deviation
    s - mean inherits the mean's error at mean / std = 1 / cv of its own size, twice in the square, and the sum of squares, its
    root and the quotient add theirs: with cv >= 1/4 (asserted) no more than 16 n 2^-53 relative in all -- the stated constant."""
    from dpf_nets_amd.metrics import neighbour_spacing
    n = 500
    rng = np.random.default_rng(9)
    clumped = np.concatenate([rng.standard_normal((n // 2, 3)) * 0.05, rng.standard_normal((n - n // 2, 3))]).astype(np.float32)
    pts = np.stack([R.make_cloud("gauss", n, 31), clumped])
    tol = 16 * n * 2.0 ** -53
    for k in (1, 4):
        mean, cv = neighbour_spacing(to(pts), k)
        assert mean.shape == (2,) and cv.shape == (2,) and mean.dtype == torch.float64 and cv.dtype == torch.float64
        for b in range(2):
            wm, wcv = R.spacing(pts[b], k)
            print("k %d slot %d: mean %.6f (rel. error %.2e), cv %.6f (rel. error %.2e), tolerance %.2e"
                  % (k, b, wm, abs(float(mean[b]) - wm) / wm, wcv, abs(float(cv[b]) - wcv) / wcv, tol))
            assert wcv >= 0.25 and abs(float(mean[b]) - wm) <= tol * wm and abs(float(cv[b]) - wcv) <= tol * wcv
        assert cv[1] > cv[0]                                                                # the clumped cloud is the less uniform
    # a full 7 x 6 x 5 unit lattice: every point, corners included, has three neighbours at distance exactly 1, so the first three
    # spacings are constant over the cloud: mean 1 and cv 0
    g = R.grid(7, 6, 5)[None]
    for k in (1, 3):
        mean, cv = neighbour_spacing(to(g), k)
        assert abs(float(mean[0]) - 1.0) <= 16 * g.shape[1] * 2.0 ** -53 and abs(float(cv[0])) <= 16 * g.shape[1] * 2.0 ** -53
    mean, cv = neighbour_spacing(to(g), 4)                                                  # the fourth: 1 inside, sqrt(2) at the corners
    assert cv[0] > 0.01
