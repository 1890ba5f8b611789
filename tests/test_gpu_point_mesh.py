"""dpf_point_mesh_distance / dpf_point_mesh_distance_grad (csrc/point_mesh.hip) through dpf_nets_amd.metrics, against the
float64 oracle of tests/point_mesh_ref.py, under form 1 (every workgroup walks all faces), form 2 (faces split over workgroups,
64-bit atomic minimum, finishing launch) and form 0 (csrc/dispatch.h decides).

Tolerance.  R = the largest absolute coordinate among a case's points and vertices; atol = K * 2^-23 * R^2 on squared distances
and K * 2^-23 * R on positions, K = 4 * K_MEASURED.  K_MEASURED = 1.37 is the worst |d2_32 - d2_64| / (2^-23 R^2) of the
contract's numpy float32 restatement against the oracle over every case used here (measured 1.369 at spread300/far;
tests/test_point_mesh_ref_cpu.py measures it without a GPU and never against the kernel), so K = 5.48.

Sizes: N in {1, 63, 64, 65, 129} (a lane, a wave less one, a wave, a wave and one, two waves and one); meshes of 1, 7, 12, 47
and 300 faces and soups of tile - 1, tile, tile + 1 and 2 * tile + 3 faces (tile = dpf_point_mesh_tile() = 256).  With one
workgroup of points, form 2 deals the 2 * tile + 3 faces to three workgroups (dispatch::pm_form, tests/test_point_mesh_dispatch_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_cases as MC                                                                     # noqa: E402
import point_mesh_ref as PR                                                                 # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 0)
CASES = PR.cases()
MESHES = PR.meshes()
_ORACLE = {}


def dev():
    return torch.device("cuda", 0)


def oracle(key):
    """computed once per case and shared"""
    if key not in _ORACLE:
        _, name, pts = next(c for c in CASES if c[0] == key)
        _ORACLE[key] = PR.oracle(*MESHES[name], pts)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def PM():
    from dpf_nets_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def DS():
    from dpf_nets_amd import datasets
    return datasets


@pytest.fixture(scope="module")
def store(DS):
    M = len(PR.ORDER)
    return DS.MeshStore(*MC.pack([MESHES[n] for n in PR.ORDER]), orig_c=np.tile(MC.ORIG_C, (M, 1)), orig_s=np.full(M, MC.ORIG_S), device=dev())


def run(PM, store, pts, idx, form, **kw):
    """pts (B, N, 3) numpy -> dist, face, closest as numpy"""
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev())
    out = PM.point_mesh_distance(p, store, idx, return_closest=True, form=form, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_tile_constant():
    from dpf_nets_amd._lib import lib
    assert lib().dpf_point_mesh_tile() == PR.TILE
    assert lib().dpf_point_mesh_workspace_bytes(3, 5) == 3 * 5 * 8 and lib().dpf_point_mesh_workspace_bytes(0, 5) == 0


# ---- values ----------------------------------------------------------------------------------------------------------------
def check_values(key, name, pts, got):
    v, f = MESHES[name]
    dist, face, closest = (g[0] for g in got)
    dmin, D, _ = oracle(key)
    R = PR.radius(v, pts)
    atol, ptol = PR.K * PR.EPS * R * R, PR.K * PR.EPS * R
    i = np.arange(len(pts))
    err = np.abs(dist.astype(np.float64) - dmin).max()
    assert face.min() >= 0 and face.max() < len(f), key
    far = (D[i, face] - dmin).max()
    on = np.sqrt(np.diagonal(PR.oracle(v, f[face], closest.astype(np.float64))[1]).max())
    own = np.abs(((pts.astype(np.float64) - closest) ** 2).sum(1) - dist).max()
    print("%s: |dist - oracle| %.3g, reported face - minimum %.3g, |p - closest|^2 - dist %.3g (atol %.3g); closest off its face %.3g (%.3g)"
          % (key, err, far, own, atol, on, ptol))
    assert np.isfinite(dist).all() and np.isfinite(closest).all(), key
    assert err <= atol, key
    assert far <= atol, key
    assert on <= ptol, key
    assert own <= atol, key


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key,name,pts", CASES, ids=[c[0] for c in CASES])
def test_values_against_the_oracle(PM, store, key, name, pts, form):
    """every mesh and size, Gaussian / on-vertex / edge-midpoint / centroid / far points, degenerate faces included (seven, degen)"""
    check_values(key, name, pts, run(PM, store, pts[None], [PR.ORDER.index(name)], form))


# ---- cross-form, batching, run to run ----------------------------------------------------------------------------------------
def test_forms_batches_and_runs_agree_bit_for_bit(PM, store):
    n = 129
    names = ["2tp3", "seven", "tp1", "2tp3", "spread300"]
    clouds = np.stack([PR.query_points(*MESHES[m], n, 800 + i) for i, m in enumerate(names)])
    idx = [PR.ORDER.index(m) for m in names]
    alone = {b: run(PM, store, clouds[b:b + 1], idx[b:b + 1], 1) for b in range(5)}
    for form in FORMS:
        batch = run(PM, store, clouds, idx, form)
        assert same(batch, run(PM, store, clouds, idx, form)), "two runs differ (form %d)" % form
        for b in range(5):
            assert same([x[b] for x in batch], [x[0] for x in alone[b]]), "slot %d differs from the cloud alone (form %d)" % (b, form)
            assert same([x[0] for x in run(PM, store, clouds[b:b + 1], idx[b:b + 1], form)], [x[0] for x in alone[b]]), (b, form)
    # the same cloud as slot 0, as slot B - 1 and against a repeated mesh
    order = [3, 1, 2, 4, 0]
    moved = run(PM, store, clouds[order], [idx[b] for b in order], 2)
    for at, b in enumerate(order):
        assert same([x[at] for x in moved], [x[0] for x in alone[b]]), (at, b)
    twice = run(PM, store, np.stack([clouds[0]] * 5), [idx[0]] * 5, 0)
    for b in range(5):
        assert same([x[b] for x in twice], [x[0] for x in alone[0]]), b


# ---- past the slots of one launch ----------------------------------------------------------------------------------------------
EDGE_SLOTS = (0, 32767, 32768)


@pytest.mark.parametrize("form", (1, 2))
def test_slots_past_one_launch(PM, DS, form):
    """B = 32 769 slots of one point each, all naming the one-triangle mesh: one more than a launch holds along y
    (dispatch::MAX_SLOTS = 32 768), so the last slot is served by a second launch.  The last slot of the first launch, the first
    of the second and slot 0 equal, bit for bit, a call with that point alone.  The limit along x (2^22 workgroups) would need
    about 10^9 items: tests/test_chunk_dispatch_cpu.py crosses it on the host with small limits instead."""
    one = DS.MeshStore(*MC.pack([MESHES["one"]]), device=dev())
    B = EDGE_SLOTS[-1] + 1
    pts = np.random.RandomState(41).standard_normal((B, 1, 3)).astype(np.float32)
    got = run(PM, one, pts, [0] * B, form)
    assert np.isfinite(got[0]).all() and (got[1] == 0).all()
    for b in EDGE_SLOTS:
        assert same([x[b] for x in got], [x[0] for x in run(PM, one, pts[b:b + 1], [0], form)]), (b, form)


# ---- ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_ties_report_the_lowest_face(PM, store, form):
    """A closed cube, points on its axes and diagonals.  Phrased on distances: the reported face is the lowest among those the
    restatement finds tied, or the kernel's distance is strictly below the restatement's for every lower-indexed face."""
    v, f = MESHES["cube"]
    pts = PR.cube_points()
    dist, face, _ = (g[0] for g in run(PM, store, pts[None], [PR.ORDER.index("cube")], form))
    d32, k32, _, D = PR.restate32(v, f, pts)
    lowest = ok = 0
    for i in range(len(pts)):
        tied = np.flatnonzero(D[i] == d32[i])
        if face[i] == tied[0]:
            lowest += 1
        else:
            assert (dist[i] < D[i, :face[i]]).all(), (i, face[i], tied, dist[i], D[i])
            ok += 1
    print("form %d: %d points on the restatement's lowest tied face, %d strictly nearer than every lower face" % (form, lowest, ok))
    assert lowest >= len(pts) // 2


# ---- bad input ---------------------------------------------------------------------------------------------------------------
def all_bad(got, sel):
    dist, face, closest = got
    return np.isnan(dist[sel]).all() and (face[sel] == -1).all() and np.isnan(closest[sel]).all()


@pytest.mark.parametrize("form", FORMS)
def test_bad_slots_and_points_are_nan_and_leave_their_neighbours_alone(PM, DS, store, form):
    n = 65
    names = ["seven", "tp1", "cube"]
    clouds = np.stack([PR.query_points(*MESHES[m], n, 900 + i) for i, m in enumerate(names)])
    idx = [PR.ORDER.index(m) for m in names]
    clean = run(PM, store, clouds, idx, form)
    for bad in (-1, len(PR.ORDER)):
        got = run(PM, store, clouds, [idx[0], bad, idx[2]], form)
        assert all_bad(got, 1)
        assert same([x[[0, 2]] for x in got], [x[[0, 2]] for x in clean])
    dirty = clouds.copy()
    dirty[0, 3, 1], dirty[1, 0, 0], dirty[1, 64, 2], dirty[2, 17] = np.nan, np.inf, -np.inf, np.nan
    got = run(PM, store, dirty, idx, form)
    hit = np.zeros((3, n), bool)
    hit[0, 3] = hit[1, 0] = hit[1, 64] = hit[2, 17] = True
    assert all_bad(got, hit)
    assert same([x[~hit] for x in got], [x[~hit] for x in clean])
    # a store that holds a flagged mesh (a face index outside its vertices)
    v, f = MC.soup(50, 106)
    broken = f.copy()
    broken[7, 1] = len(v)
    loose = DS.MeshStore(*MC.pack([MESHES["seven"], (v, broken), MESHES["cube"]]), device=dev(), strict=False)
    assert loose.bad == {1: DS.sampling.BAD_INDEX}
    got = run(PM, loose, clouds, [0, 1, 2], form)
    assert all_bad(got, 1)
    assert same([x[[0, 2]] for x in got], [x[[0, 2]] for x in clean])


# ---- round trip with the sampler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_sampled_points_lie_on_their_faces(PM, DS, store, form):
    names = ["2tp3", "spread300", "seven"]
    idx = [PR.ORDER.index(m) for m in names]
    n = 129
    plain = DS.sample_clouds(store, idx, n, seed=5, step=3, return_faces=True)
    src = plain["faces"].cpu().numpy()
    for tname in (None, "original", "scaled"):
        tf = None if tname is None else DS.CloudTransform(**MC.TRANSFORMS[tname])
        out = plain if tf is None else DS.sample_clouds(store, idx, n, seed=5, step=3, transform=tf)
        pts = out["cloud"].transpose(1, 2).contiguous()
        dist, face = PM.point_mesh_distance(pts, store, idx, transform=tf, form=form)
        dist, face = dist.cpu().numpy(), face.cpu().numpy()
        mesh_frame = plain["cloud"].transpose(1, 2).cpu().numpy()
        os_ = float(MC.ORIG_S) if tf is not None and tf.rescale else 1.0
        sc = float(tf.scale_value) if tf is not None and tf.scale else 1.0
        factor = (os_ / sc) ** 2                                   # dist' = dist * (orig_s / scale)^2
        for b, m in enumerate(names):
            v, f = MESHES[m]
            R = PR.radius(v, mesh_frame[b])
            atol = PR.K * PR.EPS * R * R
            print("%s %s: max dist %.3g (atol %.3g x %.3g)" % (tname, m, dist[b].max(), atol, factor))
            assert (dist[b] <= atol * factor).all(), (tname, m)
            p64 = mesh_frame[b].astype(np.float64)
            to_reported = np.diagonal(PR.oracle(v, f[face[b]], p64)[1])
            to_sampled = np.diagonal(PR.oracle(v, f[src[b]], p64)[1])
            assert (to_reported <= to_sampled + atol).all(), (tname, m)
    for bad in (dict(cloud_noise=True, cloud_noise_scale=0.01), MC.TRANSFORMS["centered"]):
        with pytest.raises(RuntimeError):
            PM.point_mesh_distance(pts, store, idx, transform=DS.CloudTransform(**bad))


def test_surface_accuracy(PM, store):
    key, name, pts = next(c for c in CASES if c[0] == "2tp3/129/b")
    p = torch.from_numpy(np.stack([pts, pts + np.float32(0.05)])).to(dev())
    idx = [PR.ORDER.index(name)] * 2
    dist, _ = PM.point_mesh_distance(p, store, idx)
    acc, pct = PM.surface_accuracy(p, store, idx, threshold=0.01)
    assert torch.equal(acc, dist.mean(1)) and torch.equal(PM.surface_accuracy(p, store, idx), acc)
    assert torch.equal(pct, 100.0 * (dist < 0.01).float().mean(1)) and acc.shape == (2,) and pct.shape == (2,)


# ---- autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_gradient_with_respect_to_the_points(PM, store, form):
    names = ["2tp3", "seven"]
    n = 65
    clouds = np.stack([PR.query_points(*MESHES[m], n, 950 + i) for i, m in enumerate(names)])
    clouds[1, 5] = np.nan                                           # dist NaN: gradient 0
    on_vertex = [1, 6, 11]                                          # query_points puts vertices there: on the surface exactly
    idx = [PR.ORDER.index(m) for m in names]
    g = np.random.RandomState(7).standard_normal((2, n)).astype(np.float32)
    g[0, 9] = g[1, 30] = 0.0
    p = torch.from_numpy(clouds).to(dev()).requires_grad_(True)
    dist, face, closest = PM.point_mesh_distance(p, store, idx, return_closest=True, form=form)
    assert dist.grad_fn is not None and face.grad_fn is None and not face.requires_grad and not closest.requires_grad
    (grad,) = torch.autograd.grad(dist, p, torch.from_numpy(g).to(dev()), retain_graph=True)
    (again,) = torch.autograd.grad(dist, p, torch.from_numpy(g).to(dev()))
    assert torch.equal(grad, again), "two backward runs differ"
    grad, face, dist = grad.cpu().numpy(), face.cpu().numpy(), dist.detach().cpu().numpy()
    assert np.isfinite(grad).all()
    for b, m in enumerate(names):
        v, f = MESHES[m]
        keep = np.isfinite(clouds[b]).all(1)
        R = PR.radius(v, clouds[b][keep])
        _, _, C = PR.oracle(v, f, clouds[b][keep])
        c64 = C[np.arange(keep.sum()), face[b][keep]]              # the oracle's closest point on the reported face
        want = 2.0 * g[b][keep, None] * (clouds[b][keep].astype(np.float64) - c64)
        tol = 2.0 * PR.K * PR.EPS * R * np.abs(g).max()
        err = np.abs(grad[b][keep] - want).max()
        print("form %d %s: gradient error %.3g (tol %.3g)" % (form, m, err, tol))
        assert err <= tol, m
        assert (grad[b][on_vertex] == 0).all() and (dist[b][on_vertex] == 0).all(), m
        assert (grad[b][dist[b] == 0] == 0).all(), m
    assert (grad[0, 9] == 0).all() and (grad[1, 30] == 0).all() and (grad[1, 5] == 0).all() and np.isnan(dist[1, 5])
    # without a gradient to compute there is no node and no backward launch
    q = torch.from_numpy(clouds).to(dev())
    d2, f2 = PM.point_mesh_distance(q, store, idx, form=form)
    assert d2.grad_fn is None and not d2.requires_grad
    assert np.array_equal(bits(d2.cpu().numpy()), bits(dist))
    loss = PM.surface_accuracy(p, store, [idx[0]] * 2).sum()
    loss.backward()
    assert p.grad is not None and torch.isfinite(p.grad[0]).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_batches(PM, store):
    good = torch.zeros((2, 5, 3), dtype=torch.float32, device=dev())
    bad = [(good.cpu(), [0, 1]), (good.double(), [0, 1]), (good.half(), [0, 1]), (good[0], [0]), (good.reshape(2, 15), [0, 1]),
           (torch.zeros((2, 5, 4), device=dev()), [0, 1]), (good, [0]), (good, [0, 1, 2]), (good, torch.tensor([0, 1, 2])),
           (good.transpose(0, 1), [0] * 5), (good, [0.5, 1.0])]
    for pts, idx in bad:
        with pytest.raises(RuntimeError):
            PM.point_mesh_distance(pts, store, idx)
    with pytest.raises(RuntimeError):
        PM.point_mesh_distance(good, object(), [0, 1])
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            PM.point_mesh_distance(good.to("cuda:1"), store, [0, 1])
    for B, N in ((0, 5), (2, 0), (0, 0)):
        for form in FORMS:
            dist, face, closest = PM.point_mesh_distance(torch.zeros((B, N, 3), device=dev()), store, [0] * B, return_closest=True, form=form)
            assert dist.shape == (B, N) and face.shape == (B, N) and closest.shape == (B, N, 3)
            assert dist.dtype == torch.float32 and face.dtype == torch.int32
    d, f = PM.point_mesh_distance(good, store, torch.tensor([0, 1], device=dev()))          # a device tensor of indices is fine
    assert d.shape == (2, 5) and torch.isfinite(d).all()
