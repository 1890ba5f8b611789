"""dpf_mesh_point_distance / dpf_mesh_point_distance_grad (csrc/mesh_point.hip) through dpf_nets_amd.metrics, against the float64
column oracle of tests/mesh_point_ref.py, under form 1 (every workgroup walks all points) and form 2 (point tiles split over
workgroups, 64-bit atomic minimum, finishing launch).

Tolerance.  R = the largest absolute coordinate among a case's finite points and vertices; atol = K_COLS * 2^-23 * R^2 on squared
distances and K_COLS * 2^-23 * R on positions, K_COLS = 4 * K_MEASURED_COLS.  K_MEASURED_COLS = 3.17 is the worst column-wise
|d2_32 - d2_64| / (2^-23 R^2) of the contract's numpy float32 restatement against the oracle over every case used here (measured
3.162 at tm1/1; tests/test_mesh_point_ref_cpu.py measures it without a GPU and never against the kernel), so K_COLS = 12.68.

Sizes: the cases of tests/test_gpu_point_mesh.py (N in {1, 63, 64, 65, 129}; meshes of 1, 7, 12, 47 and 300 faces and soups of
255, 256, 257 and 515 faces: a workgroup of faces less one, one, one and a lane, two and three lanes) and clouds of 255, 256, 257
and 513 points, which cross the 256-point LDS tile; with one workgroup of faces form 2 deals the 513 points to three workgroups
(dispatch::mp_form, tests/test_mesh_point_dispatch_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_cases as MC                                                                     # noqa: E402
import mesh_point_ref as MR                                                                 # noqa: E402
import point_mesh_ref as PR                                                                 # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = (1, 2)
CASES = MR.cases()
MESHES = PR.meshes()
_ORACLE = {}


def dev():
    return torch.device("cuda", 0)


def oracle(key):
    """computed once per case and shared"""
    if key not in _ORACLE:
        _, name, pts = next(c for c in CASES if c[0] == key)
        _ORACLE[key] = MR.oracle_cols(*MESHES[name], pts)
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


def tensor(pts):
    return torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).to(dev())


def run(PM, store, pts, idx, form, **kw):
    """pts (B, N, 3) numpy -> dist, point, closest, area as numpy"""
    out = PM.mesh_point_distance(tensor(pts), store, idx, return_closest=True, return_area=True, form=form, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def slot(names):
    return [PR.ORDER.index(m) for m in names]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def all_bad(got, sel):
    dist, point, closest, area = got
    return bool(np.isnan(dist[sel]).all() and (point[sel] == -1).all() and np.isnan(closest[sel]).all() and (bits(area[sel]) == 0).all())


def test_tile_constant():
    from dpf_nets_amd._lib import lib
    assert lib().dpf_mesh_point_tile() == MR.TILE
    assert lib().dpf_mesh_point_workspace_bytes(3, 5) == 3 * 5 * 8 and lib().dpf_mesh_point_workspace_bytes(0, 5) == 0


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key,name,pts", CASES, ids=[c[0] for c in CASES])
def test_values_against_the_oracle(PM, store, key, name, pts, form):
    v, f = MESHES[name]
    dist, point, closest, area = (g[0] for g in run(PM, store, pts[None], slot([name]), form))
    assert dist.shape == (len(f),)
    dcol, D, _, rows = oracle(key)
    R = PR.radius(v, pts[rows])
    atol, ptol = MR.K_COLS * MR.EPS * R * R, MR.K_COLS * MR.EPS * R
    j = np.arange(len(f))
    assert np.isfinite(dist).all() and np.isfinite(closest).all(), key
    assert np.isin(point, rows).all(), key
    err = np.abs(dist.astype(np.float64) - dcol).max()
    far = (D[np.searchsorted(rows, point), j] - dcol).max()
    own = np.abs(((pts[point].astype(np.float64) - closest) ** 2).sum(1) - dist).max()
    on = np.sqrt(np.diagonal(PR.oracle(v, f, closest.astype(np.float64))[1]).max())
    print("%s form %d: |dist - oracle| %.3g, reported point - minimum %.3g, |p - closest|^2 - dist %.3g (atol %.3g); closest off its face %.3g (%.3g)"
          % (key, form, err, far, own, atol, on, ptol))
    assert err <= atol, key
    assert far <= atol, key
    assert own <= atol, key
    assert on <= ptol, key


# ---- 2. cross-form, batching, run to run -----------------------------------------------------------------------------------------
def test_forms_batches_and_runs_agree_bit_for_bit(PM, store):
    n = 513
    names = ["2tp3", "seven", "tp1", "2tp3", "spread300"]
    F = [len(MESHES[m][1]) for m in names]
    W = max(F)
    clouds = np.stack([PR.query_points(*MESHES[m], n, 800 + i) for i, m in enumerate(names)])
    idx = slot(names)
    alone = {b: run(PM, store, clouds[b:b + 1], idx[b:b + 1], 1) for b in range(5)}        # (W = F_b: no padding)
    for b in range(5):
        assert alone[b][0].shape == (1, F[b])

    def check(batch, at, b, what):
        assert same([x[at][:F[b]] for x in batch], [x[0] for x in alone[b]]), what
        assert all_bad([x[at] for x in batch], np.arange(W) >= F[b]), what

    for form in FORMS + (0,):
        batch = run(PM, store, clouds, idx, form)
        assert batch[0].shape == (5, W) and batch[2].shape == (5, W, 3)
        assert same(batch, run(PM, store, clouds, idx, form)), "two runs differ (form %d)" % form
        for b in range(5):
            check(batch, b, b, "slot %d differs from the cloud alone (form %d)" % (b, form))
            assert same(run(PM, store, clouds[b:b + 1], idx[b:b + 1], form), alone[b]), (b, form)
    order = [3, 1, 2, 4, 0]                                          # every cloud in another slot, the first one last
    moved = run(PM, store, clouds[order], [idx[b] for b in order], 2)
    for at, b in enumerate(order):
        check(moved, at, b, (at, b))
    twice = run(PM, store, np.stack([clouds[1]] * 5), [idx[1]] * 5, 0)   # (W = 7 here)
    for b in range(5):
        assert same([x[b] for x in twice], [x[0] for x in alone[1]]), b


# ---- 2b. past the slots of one launch ------------------------------------------------------------------------------------------------
EDGE_SLOTS = (0, 32767, 32768)


def test_slots_past_one_launch(PM, DS):
    """B = 32 769 slots of one point each, all naming the one-triangle mesh: one more than a launch holds along y
    (dispatch::MAX_SLOTS = 32 768), so the last slot is served by a second launch -- of the search in both forms and of the
    backward.  The last slot of the first launch, the first of the second and slot 0 equal, bit for bit, a call with that point
    alone.  The limit along x (2^22 workgroups) would need about 10^9 items: tests/test_chunk_dispatch_cpu.py crosses it on the
    host with small limits instead."""
    one = DS.MeshStore(*MC.pack([MESHES["one"]]), device=dev())
    B = EDGE_SLOTS[-1] + 1
    pts = np.random.RandomState(43).standard_normal((B, 1, 3)).astype(np.float32)
    for form in FORMS:
        got = run(PM, one, pts, [0] * B, form)
        assert got[0].shape == (B, 1) and np.isfinite(got[0]).all() and (got[1] == 0).all()
        for b in EDGE_SLOTS:
            assert same([x[b] for x in got], [x[0] for x in run(PM, one, pts[b:b + 1], [0], form)]), (b, form)
    g = np.random.RandomState(44).standard_normal((B, 1)).astype(np.float32)

    def grad(sel):
        p = tensor(pts[sel]).requires_grad_(True)
        dist, _ = PM.mesh_point_distance(p, one, [0] * len(pts[sel]))
        return torch.autograd.grad(dist, p, tensor(g[sel]))[0].cpu().numpy()
    whole = grad(slice(None))
    assert np.isfinite(whole).all() and (whole != 0).any(axis=(1, 2)).all()
    for b in EDGE_SLOTS:
        assert np.array_equal(bits(whole[b]), bits(grad(slice(b, b + 1))[0])), b


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_ties_report_the_lowest_point(PM, store, form):
    """The repeated point: whatever face it is nearest to names index 3, never 70 or 300.  The cube: phrased on distances -- the
    reported point is the lowest among those the restatement finds tied, or the kernel's distance is strictly below the
    restatement's for every lower-indexed point."""
    pts = MR.repeated_cloud()
    dist, point, _, _ = (g[0] for g in run(PM, store, pts[None], slot([MR.REPEAT_MESH]), form))
    assert (point == MR.REPEAT_AT[0]).all(), point                  # (the other points are a hundred extents away)
    v, f = MESHES["cube"]
    pts = PR.cube_points()
    dist, point, _, _ = (g[0] for g in run(PM, store, pts[None], slot(["cube"]), form))
    d32, k32, _, D, rows = MR.restate32_cols(v, f, pts)
    lowest = 0
    for j in range(len(f)):
        tied = np.flatnonzero(D[:, j] == d32[j])
        if point[j] == tied[0]:
            lowest += 1
        else:
            assert (dist[j] < D[:point[j], j]).all(), (j, point[j], tied, dist[j])
        assert not (pts[:point[j]] == pts[point[j]]).all(1).any()
    print("form %d: %d of %d faces on the restatement's lowest tied point" % (form, lowest, len(f)))
    assert lowest >= len(f) // 2


# ---- 4. one arithmetic in both directions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,pts", CASES, ids=[c[0] for c in CASES])
def test_both_directions_share_one_arithmetic(PM, store, key, name, pts):
    """exact, no tolerance: both are minima of one matrix of fp32 pair distances"""
    pts = pts.copy()
    if len(pts) > 4:
        pts[2] = np.nan                                              # (a skipped point is in neither minimum)
    keep = np.isfinite(pts).all(1)
    d_pm, face_pm = (x[0].cpu().numpy() for x in PM.point_mesh_distance(tensor(pts[None]), store, slot([name])))
    for form in FORMS:
        dist, point, _, _ = (g[0] for g in run(PM, store, pts[None], slot([name]), form))
        assert keep[point].all()
        assert (dist[face_pm[keep]] <= d_pm[keep]).all(), (key, form)
        assert (d_pm[point] <= dist).all(), (key, form)
        assert bits(dist.min()) == bits(d_pm[keep].min()), (key, form)


# ---- 5. padding and bad slots --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_padding_bad_slots_and_bad_points(PM, DS, store, form):
    n = 65
    names = ["seven", "tp1", "cube"]
    F = [len(MESHES[m][1]) for m in names]
    W = max(F)
    clouds = np.stack([PR.query_points(*MESHES[m], n, 900 + i) for i, m in enumerate(names)])
    idx = slot(names)
    clean = run(PM, store, clouds, idx, form)
    pad = np.arange(W)[None] >= np.array(F)[:, None]
    assert all_bad(clean, pad) and np.isfinite(clean[0][~pad]).all() and (clean[1][~pad] >= 0).all()
    for bad in (-1, len(PR.ORDER)):
        got = run(PM, store, clouds, [idx[0], bad, idx[2]], form)     # (the width is that of the meshes the host knows: 12)
        assert got[0].shape == (3, max(F[0], F[2])) and all_bad(got, 1)
        for b in (0, 2):
            assert same([x[b][:F[b]] for x in got], [x[b][:F[b]] for x in clean]), (bad, b)
            assert all_bad([x[b] for x in got], np.arange(got[0].shape[1]) >= F[b]), (bad, b)
    blank = clouds.copy()
    blank[1] = np.nan                                                # no finite point in slot 1
    blank[1, 7] = (np.inf, 0.0, 0.0)
    got = run(PM, store, blank, idx, form)
    assert all_bad(got, 1)
    assert same([x[[0, 2]] for x in got], [x[[0, 2]] for x in clean])
    got = run(PM, store, clouds[:, :0], idx, form)                   # N = 0
    assert got[0].shape == (3, W) and all_bad(got, slice(None))
    # a store that holds a flagged mesh (a face index outside its vertices)
    v, f = MC.soup(50, 106)
    broken = f.copy()
    broken[7, 1] = len(v)
    loose = DS.MeshStore(*MC.pack([MESHES["seven"], (v, broken), MESHES["cube"]]), device=dev(), strict=False)
    assert loose.bad == {1: DS.sampling.BAD_INDEX}
    got = run(PM, loose, clouds, [0, 1, 2], form)
    assert got[0].shape == (3, 50) and all_bad(got, 1)
    assert same([x[0][:F[0]] for x in got], [x[0][:F[0]] for x in clean]) and same([x[2][:F[2]] for x in got], [x[2][:F[2]] for x in clean])
    # some points NaN / Inf: the same cloud without them
    for b, name in enumerate(names):
        dirty = clouds[b].copy()
        dirty[3, 1], dirty[0, 0], dirty[64, 2], dirty[17] = np.nan, np.inf, -np.inf, np.nan
        keep = np.flatnonzero(np.isfinite(dirty).all(1))
        a = [g[0] for g in run(PM, store, dirty[None], [idx[b]], form)]
        c = [g[0] for g in run(PM, store, dirty[keep][None], [idx[b]], form)]
        assert same([a[0], a[2], a[3]], [c[0], c[2], c[3]]) and np.array_equal(a[1], keep[c[1]]), name


# ---- 6. area ---------------------------------------------------------------------------------------------------------------------
def test_area_is_the_samplers_bit_for_bit(PM, store):
    names = list(PR.ORDER)
    W = max(len(MESHES[m][1]) for m in names)
    pts = np.zeros((len(names), 1, 3), np.float32)
    for form in FORMS:
        area = run(PM, store, pts, slot(names), form)[3]
        for b, m in enumerate(names):
            v, f = MESHES[m]
            want = MC.areas(v.astype(np.float32), f).astype(np.float32)
            assert np.array_equal(bits(area[b, :len(f)]), bits(want)), m
            assert (bits(area[b, len(f):]) == 0).all(), m
    v, f = MESHES["seven"]
    assert (MC.areas(v, f)[[0, 1, 6]] == 0).all() and (area[names.index("seven"), [0, 1, 6]] == 0).all()
    assert area.shape == (len(names), W)


# ---- 7. autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_gradient_with_respect_to_the_points(PM, store, form):
    names = ["2tp3", "seven"]
    n = 257
    F = [len(MESHES[m][1]) for m in names]
    W = max(F)
    clouds = np.stack([PR.query_points(*MESHES[m], n, 950 + i) for i, m in enumerate(names)])
    clouds[1, 5] = np.nan                                           # a skipped point: no face names it
    idx = slot(names)
    g = np.random.RandomState(7).standard_normal((2, W)).astype(np.float32)
    g[0, 9] = g[1, 3] = 0.0
    gt = torch.from_numpy(g).to(dev())
    p = tensor(clouds).requires_grad_(True)
    dist, point, closest, area = PM.mesh_point_distance(p, store, idx, return_closest=True, return_area=True, form=form)
    assert dist.grad_fn is not None and point.grad_fn is None
    assert not point.requires_grad and not closest.requires_grad and not area.requires_grad
    (grad,) = torch.autograd.grad(dist, p, gt, retain_graph=True)
    (again,) = torch.autograd.grad(dist, p, gt)
    assert torch.equal(grad, again), "two backward runs differ"
    grad, point, dist = grad.cpu().numpy(), point.cpu().numpy(), dist.detach().cpu().numpy()
    assert np.isfinite(grad).all()                                  # (the padded columns' NaN closest points and their g add nothing)
    for b, m in enumerate(names):
        v, f = MESHES[m]
        keep = np.isfinite(clouds[b]).all(1)
        R = PR.radius(v, clouds[b][keep])
        assert (point[b, F[b]:] == -1).all() and (point[b, :F[b]] >= 0).all()
        want, credit = MR.grad64(v, f, np.where(keep[:, None], clouds[b], 0.0), point[b, :F[b]], g[b, :F[b]])
        tol = 2.0 * MR.K_COLS * MR.EPS * R * np.abs(g).max() * credit
        err = np.abs(grad[b] - want).max(1)
        print("form %d %s: worst gradient error / tolerance %.3g over %d credited points" % (form, m, (err[credit > 0] / tol[credit > 0]).max(),
                                                                                              (credit > 0).sum()))
        assert (err <= tol).all(), m
        assert (grad[b][credit == 0] == 0).all() and (credit == 0).any(), m
    assert (grad[1, 5] == 0).all()
    # without a gradient to compute there is no node and no backward launch
    q = tensor(clouds)
    d2, p2 = PM.mesh_point_distance(q, store, idx, form=form)
    assert d2.grad_fn is None and not d2.requires_grad
    assert np.array_equal(bits(d2.cpu().numpy()), bits(dist))
    p.grad = None
    PM.surface_completeness(p, store, idx).sum().backward()
    assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any())
    p.grad = None
    PM.surface_chamfer(p, store, [idx[0]] * 2).sum().backward()
    assert torch.isfinite(p.grad[0]).all()


# ---- 8. surface_completeness / surface_chamfer -----------------------------------------------------------------------------------------
def test_surface_completeness_and_chamfer(PM, store):
    """against numpy float64 on the device's own dist and area.  Tolerance of the float32 weighted mean over F faces: the weights'
    sum carries (F - 1) roundings, the division and the product one each, the final sum (F - 1): (2 F + 2) * 2^-24 relative."""
    names = ["2tp3", "seven", "spread300", "cube"]
    n = 129
    clouds = np.stack([PR.query_points(*MESHES[m], n, 1300 + i) for i, m in enumerate(names)])
    idx = slot(names)
    idx[3] = -1                                                     # a bad slot
    p = tensor(clouds)
    dist, point, area = (x.cpu().numpy() for x in PM.mesh_point_distance(p, store, idx, return_area=True))
    thr = float(np.median(dist[0]))
    for weights in ("area", "uniform"):
        mean = PM.surface_completeness(p, store, idx, weights=weights)
        mean_t, pct = PM.surface_completeness(p, store, idx, threshold=thr, weights=weights)
        assert mean.shape == (4,) and pct.shape == (4,) and torch.equal(mean[:3], mean_t[:3])
        mean, pct = mean.cpu().numpy(), pct.cpu().numpy()
        assert np.isnan(mean[3]) and np.isnan(pct[3])
        for b, m in enumerate(names[:3]):
            F = len(MESHES[m][1])
            want, want_pct = MR.completeness64(dist[b], area[b], F, weights, thr)
            rel = (2 * F + 2) * 2.0 ** -24
            print("%s %s: completeness %.6g (float64 %.6g), %.4g %% below %.3g (%.4g)" % (weights, m, mean[b], want, pct[b], thr, want_pct))
            assert abs(mean[b] - want) <= rel * want and abs(pct[b] - want_pct) <= rel * 100.0, (weights, m)
    with pytest.raises(RuntimeError):
        PM.surface_completeness(p, store, idx, weights="faces")
    both = PM.surface_chamfer(p, store, idx)
    assert both.shape == (4,) and torch.equal(both[:3], (PM.surface_accuracy(p, store, idx) + PM.surface_completeness(p, store, idx))[:3])
    assert torch.isnan(both[3])


def test_completeness_of_transformed_clouds(PM, DS, store):
    """Clouds sampled with a transform that can be undone give the completeness of the untransformed clouds times
    (orig_s / scale)^2.  Tolerance per face, in the mesh frame: two kernel evaluations (2 atol) at points that differ by the
    float32 round trip, delta = 8 roundings (four steps out, four back) of 2^-24 relative to the largest coordinate met on the
    way: |d dist| <= 2 sqrt(dist) delta + delta^2; a weighted mean moves by no more than its terms, plus its own summation error."""
    names = ["2tp3", "spread300", "seven"]
    idx = slot(names)
    n = 129
    plain = DS.sample_clouds(store, idx, n, seed=5, step=3)["cloud"].transpose(1, 2).contiguous()
    base = PM.surface_completeness(plain, store, idx).cpu().numpy().astype(np.float64)
    dmax = PM.mesh_point_distance(plain, store, idx)[0].cpu().numpy()
    for tname in ("original", "scaled"):
        tf = DS.CloudTransform(**MC.TRANSFORMS[tname])
        pts = DS.sample_clouds(store, idx, n, seed=5, step=3, transform=tf)["cloud"].transpose(1, 2).contiguous()
        got = PM.surface_completeness(pts, store, idx, transform=tf).cpu().numpy()
        os_ = float(MC.ORIG_S) if tf.rescale else 1.0
        sc = float(tf.scale_value) if tf.scale else 1.0
        factor = (os_ / sc) ** 2
        for b, m in enumerate(names):
            v, f = MESHES[m]
            R = PR.radius(v, plain[b].cpu().numpy())
            big = max(R, float(pts[b].abs().max())) * max(1.0, os_, sc) + float(np.abs(MC.ORIG_C).max()) + max(MC.SHIFT)
            delta = 8 * 2.0 ** -24 * big
            tol = 2 * MR.K_COLS * MR.EPS * R * R + 2 * np.sqrt(np.nanmax(dmax[b])) * delta + delta * delta
            tol += (2 * len(f) + 2) * 2.0 ** -24 * 2 * base[b]
            print("%s %s: completeness %.6g against %.6g x %.4g (tol %.3g)" % (tname, m, got[b], base[b], factor, tol * factor))
            assert abs(got[b] - base[b] * factor) <= tol * factor, (tname, m)
    for bad in (dict(cloud_noise=True, cloud_noise_scale=0.01), MC.TRANSFORMS["centered"]):
        with pytest.raises(RuntimeError):
            PM.mesh_point_distance(plain, store, idx, transform=DS.CloudTransform(**bad))
        with pytest.raises(RuntimeError):
            PM.surface_completeness(plain, store, idx, transform=DS.CloudTransform(**bad))


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_batches(PM, store):
    good = torch.zeros((2, 5, 3), dtype=torch.float32, device=dev())
    bad = [(good.cpu(), [0, 1]), (good.double(), [0, 1]), (good.half(), [0, 1]), (good[0], [0]), (good.reshape(2, 15), [0, 1]),
           (torch.zeros((2, 5, 4), device=dev()), [0, 1]), (good, [0]), (good, [0, 1, 2]), (good, torch.tensor([0, 1, 2])),
           (good.transpose(0, 1), [0] * 5), (good, [0.5, 1.0])]
    for pts, idx in bad:
        with pytest.raises(RuntimeError):
            PM.mesh_point_distance(pts, store, idx)
    with pytest.raises(RuntimeError):
        PM.mesh_point_distance(good, object(), [0, 1])
    for form in (-1, 3, "1"):
        with pytest.raises(RuntimeError):
            PM.mesh_point_distance(good, store, [0, 1], form=form)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            PM.mesh_point_distance(good.to("cuda:1"), store, [0, 1])
    W = len(MESHES[PR.ORDER[1]][1])
    for B, N in ((0, 5), (2, 0), (0, 0)):
        for form in FORMS + (0,):
            dist, point, closest, area = PM.mesh_point_distance(torch.zeros((B, N, 3), device=dev()), store, [1] * B, return_closest=True,
                                                                return_area=True, form=form)
            if B:
                assert dist.shape == (B, W) and point.shape == (B, W) and closest.shape == (B, W, 3) and area.shape == (B, W)
                assert torch.isnan(dist).all() and bool((point == -1).all()) and bool((area == 0).all())
            else:
                assert dist.shape[0] == 0 and point.shape[0] == 0 and closest.shape[0] == 0 and closest.shape[2] == 3 and area.shape[0] == 0
            assert dist.dtype == torch.float32 and point.dtype == torch.int32
    d, k = PM.mesh_point_distance(good, store, torch.tensor([0, 1], device=dev()))          # a device tensor of indices is fine
    assert d.shape == (2, int(store.face_counts.max())) and bool((k[0, :1] == 0).all())
