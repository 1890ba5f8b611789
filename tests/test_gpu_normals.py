"""dpf_normals on the GPU against the numpy restatement of its contract (tests/normals_ref.py; the restatement itself is held to the
same four bounds against numpy.linalg.eigh in tests/test_normals_ref_cpu.py).  The covariance, the flags and the sign are bit-defined
and compared for EQUALITY; the eigenvalues and the vector are held to the four bounds, each 2^-46 = 64 eps, against eigh of the kernel's
OWN covariance:

    1. |C v - lambda_0 v| <= 2^-46 lambda_max           2. | |v| - 1 | <= 2^-46
    3. every eigenvalue within 2^-46 lambda_max of eigh's
    4. where lambda_1 - lambda_0 > 2^-20 lambda_max:  |v x u_0| (lambda_1 - lambda_0) / lambda_max <= 2^-46

The flag tests feed invalid VALUES that the kernel must reject by its range check; none relies on an out-of-range access."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import normals_ref as R                                                                      # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -46
EPS = 2.0 ** -52
KINDS = ("gauss", "offset", "scaled")               # the slots of a batch of 3
SENTINEL_F, SENTINEL_I, GUARD = -12345.5, -7777, 256


def dev():
    return torch.device("cuda", 0)


def L():
    from dpf_nets_amd import _lib
    return _lib


def M():
    from dpf_nets_amd import metrics
    return metrics


def to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def batch(n, seed, kinds=KINDS):
    return np.stack([R.make_cloud(kd, n, seed + 17 * b) for b, kd in enumerate(kinds)])


def knn(query, cloud, k):
    """numpy (B, n, 3), (B, m, 3) -> the device's (B, n, k) int32 table, every slot served"""
    from dpf_nets_amd.metrics.knn import knn_index
    _, index, status = knn_index(to(query), to(cloud), k)
    assert (status == 0).all()
    return index


def run(cloud, index, viewpoint=None, channels_first=False):
    """-> numpy (normal, eigenvalues, cov, flag)"""
    c = to(cloud) if isinstance(cloud, np.ndarray) else cloud
    i = to(index) if isinstance(index, np.ndarray) else index
    w = to(np.asarray(viewpoint, dtype=np.float32)) if isinstance(viewpoint, (np.ndarray, list, tuple)) else viewpoint
    return tuple(o.cpu().numpy() for o in M().normals_from_index(c, i, w, channels_first, return_cov=True))


def raw(v):
    return np.ascontiguousarray(v).view(np.uint8)


def same_bits(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(raw(g), raw(w)) for g, w in zip(got, want))


def hold_bounds(out, what, angle=True):
    """the four bounds on a run's (normal, eigenvalues, cov) against eigh of that cov; prints the worst of each"""
    normal, lam, cov = (o.reshape(-1, o.shape[-1]) for o in out[:3])
    assert np.isfinite(normal).all() and np.isfinite(lam).all() and (np.diff(lam, axis=1) >= 0).all(), what
    res, norm, ev, ang, measured = R.measures(cov, normal, lam)
    print("%s: residual %.2f eps, | |v| - 1 | %.2f eps, eigenvalues %.2f eps, angle %.2f eps on %d of %d"
          % (what, res / EPS, norm / EPS, ev / EPS, ang / EPS, measured, normal.shape[0]))
    assert res <= BOUND and norm <= BOUND and ev <= BOUND, (what, res, norm, ev)
    if angle:
        assert ang <= BOUND, (what, ang)


# k: either side of every gather capacity (4, 8, 16, 32) and the limits; n: the lane and the wave's edges, more than one workgroup;
# m: "every point is a neighbour" and either side of dpf_knn's tile.  The whole product, three slots a call.
@pytest.mark.parametrize("k", (3, 4, 5, 8, 16, 17, 32))
def test_bits_and_bounds_at_the_kernel_edges(k):
    for m in (k, 255, 257):
        clouds = batch(m, 1000 * k + m)
        squashed = batch(m, 3000 * k + m, ("squashed",))
        for n in (1, 63, 64, 65, 257):
            query = batch(n, 7000 * k + n)
            index = knn(query, clouds, k)
            got = run(clouds, index)
            want = R.normals_batch(clouds, index.cpu().numpy())
            assert (got[3] == 0).all() and same_bits(got[2:], want[2:]), (k, m, n)           # cov and flag: bit for bit
            assert not R.canonical_flip(got[0].reshape(-1, 3)).any(), (k, m, n)              # the sign, given the kernel's own vector
            hold_bounds(got, "k %d m %d n %d" % (k, m, n))
            sq = run(squashed, knn(batch(n, 9000 * k + n, ("squashed",)), squashed, k))
            hold_bounds(sq, "k %d m %d n %d squashed" % (k, m, n))
            assert not R.canonical_flip(sq[0].reshape(-1, 3)).any()


def plane(axis, at, n, seed):
    p = R.make_cloud("gauss", n, seed)
    p[:, axis] = at
    return p


def test_exact_cases():
    n, k = 130, 9
    for axis in range(3):                                                                   # the plane at 0.5 along one axis
        cloud = plane(axis, 0.5, n, 20 + axis)[None]
        normal, lam, cov, flag = run(cloud, knn(cloud, cloud, k))
        e = np.zeros(3)
        e[axis] = 1.0
        assert (flag == 0).all() and (normal == e).all() and (lam[..., 0] == 0.0).all() and (lam[..., 1] > 0).all(), axis
        off = [R.SLOT[tuple(sorted((axis, a)))] for a in range(3)]
        assert (cov[..., off] == 0.0).all(), axis
    same = R.make_cloud("same", n, 30)[None]                                                # all k neighbours at one point
    normal, lam, cov, flag = run(same, knn(same, same, k))
    assert (flag == 0).all() and (cov == 0.0).all() and (lam == 0.0).all() and np.isfinite(normal).all()
    assert (np.abs(np.sqrt((normal * normal).sum(-1)) - 1.0) <= BOUND).all()
    three = batch(n, 31)                                                                    # three points: rank 2
    out = run(three, knn(three, three, 3))
    assert (np.abs(out[1][..., 0]) <= BOUND * out[1][..., 2]).all()
    hold_bounds(out, "k 3 rank 2", angle=False)


def test_ties_on_integer_lattices():
    for k in (4, 8, 27):
        lat = batch(300, 40 + k, ("lattice", "lattice"))
        index = knn(lat, lat, k)
        out = run(lat, index)
        assert (out[3] == 0).all() and not any(np.isnan(o).any() for o in out[:3])
        assert same_bits(out[2:], R.normals_batch(lat, index.cpu().numpy())[2:])
        hold_bounds(out, "lattice k %d" % k, angle=False)
    g = np.stack([np.array([[x, y, z] for z in range(3) for y in range(3) for x in range(3)], dtype=np.float32)])   # the 3 x 3 x 3 block:
    out = run(g, np.arange(27, dtype=np.int32)[None, None, :])                               # its covariance is 18 I: a triple eigenvalue
    assert (out[1] == 18.0).all() and (out[0] == np.array([1.0, 0.0, 0.0])).all()
    hold_bounds(out, "the 3 x 3 x 3 block", angle=False)


def test_orientation():
    n, k = 200, 8
    flat = plane(2, 0.5, n, 50)[None]
    index = knn(flat, flat, k)
    up = np.array([0.0, 0.0, 1.0])
    assert (run(flat, index)[0] == up).all()
    assert (run(flat, index, [0.3, -0.2, 3.0])[0] == up).all()
    assert (run(flat, index, [0.3, -0.2, -3.0])[0] == -up).all()                             # the other side flips the exact normal
    assert (run(flat, index, [5.0, -7.0, 0.5])[0] == up).all()                               # in the plane: t == 0 keeps the canonical sign
    for w in ([np.nan, 0.0, -3.0], [0.0, np.inf, -3.0], [0.0, 0.0, -np.inf]):                # a non-finite viewpoint is no viewpoint
        assert (run(flat, index, w)[0] == up).all(), w
    clouds = batch(n, 51)
    index = knn(clouds, clouds, k)
    plain = run(clouds, index)
    w = np.array([0.5, -1.5, 2.0], dtype=np.float32)
    one = run(clouds, index, w)
    assert same_bits(one[1:], plain[1:])                                                    # a viewpoint changes nothing but the sign
    want = R.normals_batch(clouds, index.cpu().numpy(), w)
    flipped = (one[0] != plain[0]).any(-1)
    assert flipped.any() and not flipped.all() and (one[0][flipped] == -plain[0][flipped]).all()
    # the flip is the restatement's, decided on the kernel's own vector and the bit-defined centroid
    centroid = np.stack([R.covariance(clouds[b][index[b].cpu().numpy()])[0] for b in range(3)])
    assert np.array_equal(one[0].reshape(-1, 3), R.orient(plain[0].reshape(-1, 3), centroid.reshape(-1, 3), w))
    assert same_bits(want[2:], one[2:])
    per_slot = run(clouds, index, np.tile(w, (3, 1)))                                        # (B, 3), stride 3, against the broadcast one
    assert same_bits(per_slot, one)
    ws = np.array([[0.5, -1.5, 2.0], [np.nan, 0.0, 0.0], [-4.0, 0.0, 1.0]], dtype=np.float32)
    mixed = run(clouds, index, ws)
    assert same_bits([o[:1] for o in mixed], [o[:1] for o in one]) and same_bits([o[1:2] for o in mixed], [o[1:2] for o in plain])
    assert same_bits([o[2:] for o in mixed], run(clouds[2:], index[2:], ws[2]))


def test_flags_are_per_point_and_touch_no_neighbour():
    n, m0, k = 150, 200, 6
    clouds = np.stack([R.make_cloud("gauss", m0 + 2, 60 + b) for b in range(4)])
    clouds[3, m0, 1], clouds[3, m0 + 1, 0] = np.nan, 2.0 ** 62                               # two points no list reaches yet
    clouds[0, m0, 2] = 2.0 ** 61                                                            # the bound itself is served
    query = np.stack([R.make_cloud("gauss", n, 70 + b) for b in range(4)])
    index = knn(query, clouds[:, :m0], k).cpu().numpy()
    clean = run(clouds, index)
    assert (clean[3] == 0).all()
    bad = index.copy()
    bad[0, 9, 2] = m0                                                                       # 2^61: valid
    bad[1, 7, 3], bad[1, 149, 0] = -1, -2 ** 31
    bad[2, 0, 5], bad[2, 64, 1] = m0 + 2, 2 ** 31 - 1                                         # m itself and the largest int
    bad[3, 63, 0], bad[3, 100, 4] = m0, m0 + 1                                              # the NaN and the 2^62 coordinate, one list each
    got = run(clouds, bad)
    want_flag = np.zeros((4, n), dtype=np.int32)
    for b, i in ((1, 7), (1, 149), (2, 0), (2, 64), (3, 63), (3, 100)):
        want_flag[b, i] = 1
    assert np.array_equal(got[3], want_flag)
    hit = want_flag == 1
    moved = hit.copy()
    moved[0, 9] = True
    for g, c in zip(got[:3], clean[:3]):
        assert np.isnan(g[hit]).all() and np.array_equal(raw(g[~moved]), raw(c[~moved])) and np.isfinite(g[0, 9]).all()
    assert same_bits(got[2:], R.normals_batch(clouds, bad)[2:])
    refused = run(clouds, np.full((4, n, k), -1, dtype=np.int32))                            # dpf_knn's refused table: flags, and success
    assert (refused[3] == 1).all() and all(np.isnan(o).all() for o in refused[:3])


def test_layouts_strides_a_broadcast_cloud_and_an_int64_index():
    n, m, k, B = 130, 333, 6, 3
    clouds = batch(m, 80)
    c = to(clouds)
    index = knn(batch(n, 81), clouds, k)
    want = run(c, index)
    assert same_bits(want[2:], R.normals_batch(clouds, index.cpu().numpy())[2:])
    ccf = c.transpose(1, 2).contiguous()                                                    # (B, 3, M)
    assert same_bits(run(ccf, index, channels_first=True), want)
    assert same_bits(run(c.transpose(1, 2), index, channels_first=True), want)              # a (B, 3, M) view of point-major memory
    big = torch.full((2 * B + 1, m + 9, 5), float("nan"), device=dev())                     # anything read outside the slice would flag
    view = big[1::2, 4:4 + m, 1:4]
    view.copy_(c)
    assert not view.is_contiguous() and same_bits(run(view, index), want)
    assert same_bits(run(c, index.long()), want)                                            # int64 indices
    assert same_bits(run(c, index.long().transpose(1, 2).contiguous().transpose(1, 2)), want)    # ... and a strided table
    one = c[1:2].expand(B, m, 3)                                                            # cloud stride 0
    assert one.stride(0) == 0
    assert same_bits(run(one, index), run(c[1:2].repeat(B, 1, 1), index))
    w = torch.tensor([[0.1, 0.2, 5.0]], device=dev()).expand(B, 3)                          # a viewpoint expanded over the batch
    assert same_bits(run(c, index, w), run(c, index, [0.1, 0.2, 5.0]))


def test_a_slot_gives_the_same_bits_alone_and_inside_a_batch_of_70_and_two_runs_agree():
    n, m, k = 200, 300, 7
    rng = np.random.default_rng(5)
    mine = R.make_cloud("gauss", m, 90)
    others = rng.standard_normal((69, m, 3)).astype(np.float32)
    query = rng.standard_normal((70, n, 3)).astype(np.float32)
    for at in (0, 37, 69):
        clouds = np.concatenate([others[:at], mine[None], others[at:]])
        index = knn(query[[at] * 70], clouds, k)
        alone = run(clouds[at:at + 1], index[at:at + 1])
        inside = run(clouds, index)
        assert (inside[3] == 0).all() and same_bits([o[at:at + 1] for o in inside], alone), at
        assert same_bits(run(clouds, index), inside)                                        # a second run: the same bits


def guarded(count, dtype, sentinel):
    buf = torch.full((GUARD + count + GUARD,), sentinel, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + count]


@pytest.mark.parametrize("n,m,k", ((1, 5, 5), (65, 257, 3), (257, 300, 17), (300, 64, 32)))
def test_nothing_is_written_outside_the_outputs_and_a_null_cov_is_accepted(n, m, k):
    B = 3
    clouds = batch(m, 100)
    index = knn(batch(n, 101), clouds, k).clone()
    index[2, n - 1, k - 1] = -1                                                             # (a flagged point's fill stays inside too)
    c = to(clouds)
    want = run(c, index)
    lib = L().lib()
    for with_cov in (True, False):
        nbuf, normal = guarded(B * n * 3, torch.float64, SENTINEL_F)
        lbuf, lam = guarded(B * n * 3, torch.float64, SENTINEL_F)
        cbuf, cov = guarded(B * n * 6, torch.float64, SENTINEL_F)
        fbuf, flag = guarded(B * n, torch.int32, SENTINEL_I)
        rc = lib.dpf_normals(B, n, m, c.data_ptr(), m * 3, 3, 1, index.data_ptr(), k, None, 0, normal.data_ptr(), lam.data_ptr(),
                             cov.data_ptr() if with_cov else None, flag.data_ptr(), L().current_stream())
        torch.cuda.synchronize()
        assert rc == 0
        for buf, s in ((nbuf, SENTINEL_F), (lbuf, SENTINEL_F), (cbuf, SENTINEL_F), (fbuf, SENTINEL_I)):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == s).all() and (h[-GUARD:] == s).all()
        got = [normal.cpu().numpy().reshape(B, n, 3), lam.cpu().numpy().reshape(B, n, 3), flag.cpu().numpy().reshape(B, n)]
        assert same_bits(got, [want[0], want[1], want[3]]), with_cov
        if with_cov:
            assert same_bits([cov.cpu().numpy().reshape(B, n, 6)], [want[2]])
        else:
            assert (cbuf.cpu().numpy() == SENTINEL_F).all()
    assert want[3].sum() == 1 and want[3][2, n - 1] == 1


def test_return_codes():
    lib, st = L().lib(), L().current_stream()
    n = m = 40
    t = to(R.make_cloud("gauss", m, 1)[None])
    index = torch.zeros((n * 33,), dtype=torch.int32, device=dev())
    nbuf, normal = guarded(n * 3, torch.float64, SENTINEL_F)
    lbuf, lam = guarded(n * 3, torch.float64, SENTINEL_F)
    fbuf, flag = guarded(n, torch.int32, SENTINEL_I)

    def rc(B=1, n=n, m=m, c=t.data_ptr(), i=index.data_ptr(), k=4, nrm=normal.data_ptr(), lm=lam.data_ptr(), fl=flag.data_ptr()):
        return lib.dpf_normals(B, n, m, c, m * 3, 3, 1, i, k, None, 0, nrm, lm, None, fl, st)

    assert rc(B=0) == 0                                                                     # nothing to do, nothing launched
    for bad in (dict(B=-1), dict(n=0), dict(m=0), dict(k=2), dict(k=0), dict(k=-1), dict(c=None), dict(i=None), dict(nrm=None),
                dict(lm=None), dict(fl=None)):
        assert rc(**bad) == -1, bad
    assert rc(k=33) == -2 and rc(k=1000) == -2
    torch.cuda.synchronize()
    assert all((b.cpu().numpy() == s).all() for b, s in ((nbuf, SENTINEL_F), (lbuf, SENTINEL_F), (fbuf, SENTINEL_I)))
    assert rc(k=3) == 0 and rc(k=32) == 0 and rc(m=2, k=3) == 0                              # (k above m: a list may repeat a point)
    torch.cuda.synchronize()
    assert (flag.cpu().numpy() == 0).all()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def test_estimate_normals_and_surface_variation():
    from dpf_nets_amd.metrics import estimate_normals, normals_from_index, surface_variation
    from dpf_nets_amd.metrics.knn import knn_index
    n, k = 300, 10
    clouds = to(batch(n, 110))
    index = knn_index(clouds, clouds, k, False)[1]
    assert (index[:, :, 0] == torch.arange(n, device=dev())[None]).all()                    # the point itself is its first neighbour
    normal, lam, flag = normals_from_index(clouds, index)
    assert normal.dtype == torch.float64 and lam.dtype == torch.float64 and flag.dtype == torch.int32 and flag.shape == (3, n)
    n64, l64 = estimate_normals(clouds, k, double=True)
    assert torch.equal(n64, normal) and torch.equal(l64, lam) and not n64.requires_grad
    n32, l32 = estimate_normals(clouds.requires_grad_(True), k)
    assert n32.dtype == torch.float32 and n32.shape == (3, n, 3) and l32.dtype == torch.float64 and torch.equal(l32, lam)
    assert not n32.requires_grad and not l32.requires_grad
    assert ((n32.double() - normal).abs() <= 2.0 ** -24).all()
    clouds = clouds.detach()
    ncf, lcf = estimate_normals(clouds.transpose(1, 2).contiguous(), k, channels_first=True, double=True)
    assert torch.equal(ncf, normal) and torch.equal(lcf, lam)
    w = torch.tensor([0.0, 0.0, 50.0], device=dev())
    nv, _ = estimate_normals(clouds[:1], k, viewpoint=w, double=True)
    assert torch.equal(nv, normals_from_index(clouds[:1], index[:1], w)[0])
    centroid = R.covariance(clouds[0].cpu().numpy()[index[0].cpu().numpy()])[0]             # every normal faces the viewpoint from its centroid
    assert ((nv[0].cpu().numpy() * (w.cpu().numpy().astype(np.float64) - centroid)).sum(-1) >= 0).all()
    sv = surface_variation(lam)
    assert sv.dtype == torch.float64 and sv.shape == (3, n) and ((sv >= 0) & (sv <= 1.0 / 3.0 + 1e-12)).all()
    assert np.array_equal(sv.cpu().numpy(), R.surface_variation(lam.cpu().numpy()))
    flat = to(plane(2, 0.5, n, 111)[None])
    assert (surface_variation(estimate_normals(flat, k)[1]) == 0.0).all()                   # a plane: exactly 0
    same = to(R.make_cloud("same", n, 112)[None])
    assert (surface_variation(estimate_normals(same, k)[1]) == 0.0).all()                   # a zero sum: 0, not NaN
    with pytest.raises(RuntimeError):
        estimate_normals(clouds.cpu(), k)
    with pytest.raises(RuntimeError):
        estimate_normals(clouds.double(), k)
    for bad_k in (2, 33, n + 1):
        with pytest.raises(ValueError):
            estimate_normals(clouds, bad_k)
    with pytest.raises(ValueError):
        estimate_normals(clouds[:, :20], 21)
    with pytest.raises(ValueError):
        normals_from_index(clouds, index[:, :, :2])
    bad = clouds.clone()
    bad[1, 7, 0] = float("nan")
    with pytest.raises(ValueError, match=r"point \(1, 0\).*%d points flagged" % n):          # dpf_knn refuses the slot: every point of it
        estimate_normals(bad, k)


def test_normal_consistency():
    from dpf_nets_amd.metrics import estimate_normals, normal_consistency
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    n, m, k = 257, 300, 8
    a, b = to(batch(n, 120)), to(batch(m, 121))
    ab, ba = normal_consistency(a, b, k)
    assert ab.shape == (3,) and ba.shape == (3,) and ab.dtype == torch.float64 and ba.dtype == torch.float64
    na, nb = (estimate_normals(x, k, double=True)[0].cpu().numpy() for x in (a, b))
    _, i1, _, i2 = (t.cpu().numpy() for t in BK.NNDistance(a, b))
    for s in range(3):
        want_ab = np.abs((na[s] * nb[s][i1[s]]).sum(-1)).mean()
        want_ba = np.abs((nb[s] * na[s][i2[s]]).sum(-1)).mean()
        print("slot %d: a->b %.6f (error %.2e), b->a %.6f (error %.2e), tolerance %.2e"
              % (s, want_ab, abs(float(ab[s]) - want_ab), want_ba, abs(float(ba[s]) - want_ba), max(n, m) * EPS))
        assert abs(float(ab[s]) - want_ab) <= n * EPS and abs(float(ba[s]) - want_ba) <= m * EPS
        assert 0.0 < want_ab < 1.0
    given = normal_consistency(a, b, k, normals_a=to(na), normals_b=to(nb))                  # the caller's normals: the same numbers
    assert torch.equal(given[0], ab) and torch.equal(given[1], ba)
    swapped = normal_consistency(a, b, k, normals_a=to(-na))                                # unoriented
    assert torch.equal(swapped[0], ab) and torch.equal(swapped[1], ba)
    self_ab, self_ba = normal_consistency(a, a, k)
    assert ((self_ab - 1.0).abs() <= 2.0 ** -40).all() and ((self_ba - 1.0).abs() <= 2.0 ** -40).all()
    low, high, wall = to(plane(2, 0.5, n, 122)[None]), to(plane(2, 1.5, m, 123)[None]), to(plane(0, 0.5, m, 124)[None])
    par = normal_consistency(low, high, k)
    assert float(par[0]) == 1.0 and float(par[1]) == 1.0                                    # two parallel planes
    perp = normal_consistency(low, wall, k)
    assert float(perp[0]) == 0.0 and float(perp[1]) == 0.0                                  # two perpendicular planes
