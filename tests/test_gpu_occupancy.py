"""dpf_occupancy_grid (csrc/occupancy.hip) through its callers: entropy_of_occupancy_grid / jsd_between_point_cloud_sets
(metrics/evaluation_metrics.py) against the reference's own results (tests/golden/occupancy_jsd.npz), the nearest-centre
contract at its edges against a float64 brute force written here, and get_voxel_occ_dist / JSD (networks/utils.py) on CUDA
tensors against the vectors of tests/golden/eval_metrics.npz.

The contract (include/dpf_hip.h): the cell of a point is the argmin over the kept centres of (dx*dx + dy*dy) + dz*dz in double,
the fp32 inputs widened, the LOWEST kept index on an exact tie.  Counts are integers: every comparison below is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SLICE = 4096            # points of a cloud per workgroup (csrc/occupancy.hip OCC_SLICE): a longer cloud is split
MAX_WGS = 32768         # workgroups per launch (OCC_MAX_WGS): more clouds than this are chunked by the entry point


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "occupancy_jsd.npz"))


@pytest.fixture(scope="module")
def vox():
    return np.load(os.path.join(HERE, "golden", "eval_metrics.npz"))


@pytest.fixture(scope="module")
def EM():
    from dpf_nets_amd.metrics import evaluation_metrics
    return evaluation_metrics


@pytest.fixture(scope="module")
def OC():
    from dpf_nets_amd.metrics import occupancy
    return occupancy


def dev():
    return torch.device("cuda", 0)


def golden_counters(gold, tag, res, sph):
    key = "%s/%d/%d" % (tag, res, sph)
    out = np.zeros(len(gold["grid/%d/%d" % (res, sph)].reshape(-1, 3)))
    out[gold["counters_idx/" + key]] = gold["counters_val/" + key]
    return out


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's own results
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sample", "ref"])
@pytest.mark.parametrize("res", [8, 28])
@pytest.mark.parametrize("sph", [False, True])
def test_counters_and_entropy_vs_reference_golden(gold, EM, tag, res, sph):
    clouds = gold["clouds/" + tag]
    ent, counters = EM.entropy_of_occupancy_grid(clouds, res, sph)
    want = golden_counters(gold, tag, res, sph)
    assert counters.dtype == np.float64 and counters.shape == want.shape
    assert np.array_equal(counters, want)                                     # no point is exempt (the inputs have no ties)
    want_ent = float(gold["entropy/%s/%d/%d" % (tag, res, sph)])
    print("entropy", ent, "reference", want_ent, "diff", abs(ent - want_ent))
    assert abs(ent - want_ent) <= len(want) * 2.0 ** -52 * want_ent + 1e-15      # a reordered sum of <= n_cells doubles
    ent_t, counters_t = EM.entropy_of_occupancy_grid(torch.from_numpy(clouds).to(dev()), res, sph)
    assert ent_t == ent and np.array_equal(counters_t, counters)              # numpy array and CUDA tensor: the same call


@pytest.mark.parametrize("res", [8, 28])
def test_jsd_vs_reference_golden(gold, EM, res):
    s, r = gold["clouds/sample"], gold["clouds/ref"]
    got = EM.jsd_between_point_cloud_sets(s, r, res)
    print("jsd", got, "reference", float(gold["jsd/%d" % res]))
    assert abs(got - float(gold["jsd/%d" % res])) <= 1e-12
    assert EM.jsd_between_point_cloud_sets(torch.from_numpy(s).to(dev()), torch.from_numpy(r).to(dev()), res) == got


# ---------------------------------------------------------------------------------------------------------------
# 2. the contract at its edges, against a float64 brute force
# ---------------------------------------------------------------------------------------------------------------
def brute(clouds, grid):
    """(counts, clouds_touching) by the contract's expression in float64; np.argmin takes the lowest index of a tie"""
    g = grid.reshape(-1, 3).astype(np.float64)
    S, n = clouds.shape[:2]
    p = clouds.reshape(-1, 3).astype(np.float64)
    best = np.empty(len(p), np.int64)
    step = max(1, (1 << 22) // len(g))
    for lo in range(0, len(p), step):
        d = p[lo:lo + step, None, :] - g[None, :, :]
        best[lo:lo + step] = np.argmin((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
    counts = np.bincount(best, minlength=len(g))
    touching = np.zeros(len(g), np.int64)
    for s in range(S):
        touching[np.unique(best[s * n:(s + 1) * n])] += 1
    return counts, touching


def special_points(OC, res, sph):
    """centres, midpoints between neighbouring kept cells (exact ties where the grid is dyadic), the origin, |x| = 3, the
    clipped cells nearest to the sphere (a point there rounds to a cell that is not kept), and points so far out along one axis
    that the other axes' terms vanish in the rounded sum: every cell of a row ties, and the lowest index must win"""
    full = OC.unit_cube_grid(res, False)[0].reshape(-1, 3)
    kept = OC.unit_cube_grid(res, sph)[0].reshape(-1, 3)
    rng = np.random.RandomState(res * 2 + sph)
    pts = [kept[rng.randint(0, len(kept), 12)]]                                           # exactly on centres
    a = kept[rng.randint(0, len(kept), 40)]
    for axis in range(3):                                                                 # midpoints along one axis, two, three
        step = np.zeros(3, np.float32)
        step[:axis + 1] = np.float32(1.0 / (res - 1))
        pts.append((a.astype(np.float64) + 0.5 * step.astype(np.float64)).astype(np.float32))
    pts.append(np.zeros((1, 3), np.float32))
    pts.append(np.array([[3, 0, 0], [-3, 3, 3], [0, -3, 0], [3, 3, -3], [0.1, 0.2, 3], [-3, -3, -3]], np.float32))
    norms = np.linalg.norm(full, axis=1)
    outside = full[np.argsort(np.where(norms > 0.5, norms, np.inf))[:16]]                 # first cells outside the fp32 clip
    pts.append(outside)
    pts.append((outside * np.float32(1.001)).astype(np.float32))
    pts.append(np.array([[0.3, 1e9, 0.1], [1e9, 0.2, -0.1], [-0.2, 0.1, -1e9], [1e30, -1e30, 0.0]], np.float32))
    return np.concatenate(pts, axis=0)


def edge_clouds(OC, res, sph, S, n, seed):
    rng = np.random.RandomState(seed)
    c = (rng.randn(S, n, 3) * 0.3).astype(np.float32)
    sp = special_points(OC, res, sph)
    flat = c.reshape(-1, 3)
    take = min(len(flat), len(sp))
    flat[rng.permutation(len(flat))[:take]] = sp[rng.permutation(len(sp))[:take]]
    return c


EDGE_CASES = [  # (res, in_sphere, S, n)
    (8, True, 3, 1), (8, True, 3, 63), (8, True, 3, 65), (8, True, 3, 300), (8, True, 1, 300), (8, False, 3, 300),
    (33, True, 2, 300), (33, False, 2, 300), (28, True, 2, 300),
    (8, True, 3, SLICE + 4),                         # a cloud split over two workgroups
    (8, True, MAX_WGS + 5, 2),                       # more clouds than one launch takes
]


@pytest.mark.parametrize("res,sph,S,n", EDGE_CASES)
def test_nearest_centre_contract_vs_float64_brute_force(OC, res, sph, S, n):
    clouds = edge_clouds(OC, res, sph, S, n, seed=res + S + n)
    want_c, want_t = brute(clouds, OC.unit_cube_grid(res, sph)[0])
    got_c, got_t = OC.nearest_grid_counts(clouds, res, sph)
    assert got_c.sum() == S * n
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_t, want_t)


def test_exact_midpoints_go_to_the_lowest_kept_index(OC):
    """res = 33: the centres are multiples of 1/32, so the midpoint of two neighbours is an exact tie in double"""
    res = 33
    kept = OC.unit_cube_grid(res, True)[0]
    pts = special_points(OC, res, True)[12:12 + 120]                          # the three families of midpoints
    d = pts[:, None, :].astype(np.float64) - kept[None].astype(np.float64)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum() >= 60     # the ties are there
    clouds = pts.reshape(1, -1, 3)
    want_c, want_t = brute(clouds, kept)
    got_c, got_t = OC.nearest_grid_counts(clouds, res, True)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_t, want_t)


@pytest.mark.parametrize("S,n", [(5, 300), (3, SLICE + 4)])
def test_one_cell_from_every_cloud(OC, S, n):
    res = 8
    kept = OC.unit_cube_grid(res, True)[0]
    cell = 77
    clouds = np.broadcast_to(kept[cell], (S, n, 3)).copy()
    counts, touching = OC.nearest_grid_counts(torch.from_numpy(clouds).to(dev()), res, True)
    want = np.zeros(len(kept), np.int64)
    want[cell] = S * n
    assert np.array_equal(counts, want)
    want[cell] = S
    assert np.array_equal(touching, want)
    one_c, one_t = OC.nearest_grid_counts(clouds[:1], res, True)
    assert one_c[cell] == n and one_c.sum() == n and one_t[cell] == 1 and one_t.sum() == 1


def test_resolution_above_the_cap_raises(EM, OC):
    cap = OC.max_resolution()
    assert cap >= 64
    clouds = np.zeros((1, 4, 3), np.float32)
    with pytest.raises(ValueError):
        EM.entropy_of_occupancy_grid(clouds, cap + 1, True)
    from dpf_nets_amd.networks import utils as U
    with pytest.raises(ValueError):
        U.get_voxel_occ_dist(torch.from_numpy(clouds).to(dev()), res=cap + 1)
    ent, counters = EM.entropy_of_occupancy_grid(clouds, cap, False)          # the cap itself works: every point at the origin
    assert counters.sum() == 4 and counters.max() == 4


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_point_raises_in_nearest_mode(EM, bad):
    clouds = (np.random.RandomState(3).randn(2, 70, 3) * 0.2).astype(np.float32)
    clouds[1, 69, 1] = bad
    with pytest.raises(ValueError):
        EM.entropy_of_occupancy_grid(clouds, 8, True)
    with pytest.raises(ValueError):
        EM.entropy_of_occupancy_grid(torch.from_numpy(clouds).to(dev()), 8, False)


def test_two_consecutive_calls_agree(EM, gold):
    x = torch.from_numpy(gold["clouds/sample"]).to(dev())
    a = EM.entropy_of_occupancy_grid(x, 28, True)
    other = EM.entropy_of_occupancy_grid(torch.from_numpy(gold["clouds/ref"]).to(dev()), 28, True)
    b = EM.entropy_of_occupancy_grid(x, 28, True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], other[1])
    assert a[1].sum() == x.shape[0] * x.shape[1]                             # zeroed per call: nothing accumulates


# ---------------------------------------------------------------------------------------------------------------
# 3. cube bins
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["v1", "v2"])
def test_voxel_occupancy_and_jsd_of_cuda_tensors_vs_reference_golden(vox, tag, capsys):
    from dpf_nets_amd.networks import utils as U
    c1, c2 = vox[tag + "/c1"], vox[tag + "/c2"]
    t1, t2 = torch.from_numpy(c1).to(dev()), torch.from_numpy(c2).to(dev())
    occ = U.get_voxel_occ_dist(t1, warning=False)
    assert occ.dtype == np.float64 and occ.shape == (28, 28, 28)
    assert np.array_equal(occ, vox[tag + "/occ1"])                            # faces, edges and the NaN point included
    assert np.array_equal(U.get_voxel_occ_dist(t1, warning=False), occ)       # and again: the counters start from zero
    got = U.JSD(t1, t2, warning=False)
    print("JSD", got, "reference", float(vox[tag + "/jsd"]))
    assert abs(got - float(vox[tag + "/jsd"])) <= 1e-12
    assert U.JSD(t1, t1, warning=False) == pytest.approx(0.0, abs=1e-12)
    capsys.readouterr()
    U.get_voxel_occ_dist(t1, clouds_flag="gen")
    on_device = capsys.readouterr().out
    U.get_voxel_occ_dist(c1, clouds_flag="gen")
    assert on_device == capsys.readouterr().out and "NaN values" in on_device and "out of cube bounds" in on_device


@pytest.mark.parametrize("res,S,n", [(7, 2, SLICE + 4), (2, 2, 65), (64, 1, 300), (5, MAX_WGS + 3, 1)])
def test_cube_bins_agree_with_the_host_path(res, S, n):
    from dpf_nets_amd.networks import utils as U
    c = (np.random.RandomState(res + n).randn(S, n, 3) * 0.3).astype(np.float32)
    edges = (-0.5 + np.arange(res + 1) * (1. / res)).astype(np.float32)
    c.reshape(-1)[:res + 1] = edges[:c.size]                                  # on the edges (after the fp32 rounding), and +-0.5
    c[-1, -1] = [np.inf, 0.0, -np.inf]
    want = U.get_voxel_occ_dist(c, res=res, warning=False)
    got = U.get_voxel_occ_dist(torch.from_numpy(c).to(dev()), res=res, warning=False)
    assert np.array_equal(got, want)
