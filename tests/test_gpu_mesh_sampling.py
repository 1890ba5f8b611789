"""dpf_mesh_cdf_build / dpf_mesh_variates / dpf_mesh_sample (csrc/mesh_sample.hip) through dpf_nets_amd.datasets, against the
reference's own sample_cloud and cloud transformations (tests/golden/mesh_sampling.npz, tools/gen_golden_mesh_sampling.py).

The contract (include/dpf_hip.h).  Face choice: the kernel's edges are exact ratios of running sums of UNROUNDED fp32 areas;
the reference's come from fp32-ROUNDED probabilities, so a reference edge equals the exact-ratio edge times (1 + a) / (1 + b)
with |a|, |b| <= 2^-24 and lies within 2^-23 of it (edges are <= 1; the double sums add nothing visible at that scale).  A
reported face k is accepted iff edge_ref[k - 1] - 2^-23 <= u < edge_ref[k] + 2^-23 -- exact equality with the reference's face
away from an edge, and the generator has checked that at most 2 % of a case's samples are near one.  No sample is exempt.
Points: bitwise the golden where the face is the reference's, bitwise the fp32 formula on the reported face otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_cases as MC                                                                     # noqa: E402

pytestmark = pytest.mark.gpu

T = MC.T                 # faces per scan tile of the cumulative distribution (csrc/mesh_sample.hip MS_TILE)
ORDER = sorted(MC.MESHES)


def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "mesh_sampling.npz"))


@pytest.fixture(scope="module")
def DS():
    from dpf_nets_amd import datasets
    return datasets


@pytest.fixture(scope="module")
def meshes(gold):
    out = {}
    for name in ORDER:
        out[name] = (gold["vertices/" + name], gold["faces/" + name]) if name in MC.STORED else MC.MESHES[name]()
        assert MC.checksum(*out[name]) == int(gold["crc/" + name])
    return out


def make_store(DS, meshes, names, **kw):
    M = len(names)
    return DS.MeshStore(*MC.pack([meshes[n] for n in names]), orig_c=np.tile(MC.ORIG_C, (M, 1)), orig_s=np.full(M, MC.ORIG_S), device=dev(), **kw)


@pytest.fixture(scope="module")
def store(DS, meshes):
    return make_store(DS, meshes, ORDER)


def bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def run_case(DS, store, gold, mesh, n, ev, seed, transform=None):
    key = MC.case_key(mesh, n, ev, seed)
    S = 2 * n if ev else n
    var = tuple(gold[k + "/" + key].reshape(1, S) for k in ("u", "s1", "s2"))
    out = DS.sample_clouds(store, [ORDER.index(mesh)], n, return_eval_cloud=ev, variates=var, transform=transform, return_faces=True)
    return key, var, out


def check_faces(u, k, edges, area):
    """test 1 of the module docstring, for every sample; returns which faces are the reference's own"""
    assert k.min() >= 0 and k.max() < len(edges)
    lower = np.where(k > 0, edges[np.maximum(k - 1, 0)], 0.0)
    ok = (lower - MC.EDGE_TOL <= u) & (u < edges[k] + MC.EDGE_TOL)
    assert ok.all(), "faces outside the reference's interval: samples %s" % np.flatnonzero(~ok)[:8]
    assert (area[k] > 0).all(), "a zero-area face was chosen"
    return k == edges.searchsorted(u, side="right")


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2. faces and points against the reference's outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,n,ev,seed,forced", MC.CASES, ids=[MC.case_key(*c[:4]) for c in MC.CASES])
def test_faces_and_points_vs_reference_golden(DS, store, gold, meshes, mesh, n, ev, seed, forced):
    key, (u, s1, s2), out = run_case(DS, store, gold, mesh, n, ev, seed)
    v, f = meshes[mesh]
    S = u.shape[1]
    assert set(out) == {"cloud", "faces", "orig_c", "orig_s"} | ({"eval_cloud"} if ev else set())
    assert out["cloud"].shape == (1, 3, n) and out["cloud"].dtype == torch.float32 and out["cloud"].is_cuda
    assert out["faces"].shape == (1, S) and out["orig_c"].shape == (1, 3) and out["orig_s"].shape == (1,)
    k = out["faces"].cpu().numpy()[0].astype(np.int64)
    own = check_faces(u[0], k, gold["edges/" + mesh], MC.areas(v, f))
    assert np.array_equal(gold["face/" + key][own], k[own])
    print("%s: %d of %d samples on the reference's own face" % (key, int(own.sum()), S))
    assert own.mean() >= 0.98
    if forced:
        assert u[0, 0] == 0.0 and u[0, 1] == MC.U_MAX and own[0] and own[1]
    formula = MC.points(v, f, k, s1[0], s2[0])                               # (S, 3): the fp32 formula on the REPORTED face
    parts = (("cloud", slice(0, None, 2)), ("eval_cloud", slice(1, None, 2))) if ev else (("cloud", slice(None)),)
    for name, sel in parts:
        got, want = bits(out[name])[0], bits(gold[name + "/" + key])
        assert got.shape == want.shape == (3, n)
        o = own[sel]
        assert np.array_equal(got[:, o], want[:, o]), name                   # the reference's point, bit for bit
        assert np.array_equal(got[:, ~o], bits(formula[sel].T)[:, ~o]), name


def test_batch_with_a_repeated_mesh_explicit(DS, store, gold):
    """(B, 3, N) layout with B = 3: slots 0 and 2 name the same mesh with the same variates, slot 1 another mesh"""
    a, b = ("2tp3", 65, True, 2121), ("spread300", 65, True, 2021)
    ka, kb = MC.case_key(*a), MC.case_key(*b)
    var = tuple(np.stack([gold[k + "/" + ka], gold[k + "/" + kb], gold[k + "/" + ka]]) for k in ("u", "s1", "s2"))
    idx = [ORDER.index("2tp3"), ORDER.index("spread300"), ORDER.index("2tp3")]
    out = DS.sample_clouds(store, idx, 65, return_eval_cloud=True, variates=var, return_faces=True)
    faces = out["faces"].cpu().numpy()
    for slot, key in enumerate((ka, kb, ka)):
        own = faces[slot] == gold["face/" + key]
        assert own.mean() >= 0.98
        for name, sel in (("cloud", slice(0, None, 2)), ("eval_cloud", slice(1, None, 2))):
            assert np.array_equal(bits(out[name])[slot][:, own[sel]], bits(gold[name + "/" + key])[:, own[sel]])
    assert np.array_equal(bits(out["cloud"])[0], bits(out["cloud"])[2])
    # CUDA tensors as variates: the same call
    again = DS.sample_clouds(store, np.array(idx), 65, return_eval_cloud=True, variates=tuple(torch.from_numpy(x).to(dev()) for x in var))
    assert np.array_equal(bits(again["cloud"]), bits(out["cloud"])) and np.array_equal(bits(again["eval_cloud"]), bits(out["eval_cloud"]))


# ---------------------------------------------------------------------------------------------------------------
# 3. transforms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["original", "scaled"])
@pytest.mark.parametrize("case", MC.TRANSFORM_CASES, ids=[MC.case_key(*c) for c in MC.TRANSFORM_CASES])
def test_fused_transforms_vs_reference_golden(DS, store, gold, tag, case):
    mesh, n, ev, seed = case
    key, _, out = run_case(DS, store, gold, mesh, n, ev, seed, DS.CloudTransform(**MC.TRANSFORMS[tag]))
    own = out["faces"].cpu().numpy()[0] == gold["face/" + key]
    assert own.mean() >= 0.98
    for name, sel in ((("cloud", slice(0, None, 2)), ("eval_cloud", slice(1, None, 2))) if ev else (("cloud", slice(None)),)):
        o = own[sel]
        assert np.array_equal(bits(out[name])[0][:, o], bits(gold["%s/%s/%s" % (name, tag, key)])[:, o]), name


@pytest.mark.parametrize("case", MC.TRANSFORM_CASES, ids=[MC.case_key(*c) for c in MC.TRANSFORM_CASES])
def test_centring_vs_reference_golden(DS, store, gold, case):
    """both sides subtract an fp32 tree sum of n <= 2^16 terms divided by n: ~log2(n) * 2^-24 relative error each"""
    mesh, n, ev, seed = case
    key, _, out = run_case(DS, store, gold, mesh, n, ev, seed, DS.CloudTransform(**MC.TRANSFORMS["centered"]))
    assert (out["faces"].cpu().numpy()[0] == gold["face/" + key]).all()      # (else the means would differ by a whole point)
    for name in ("cloud", "eval_cloud") if ev else ("cloud",):
        want = gold["%s/centered/%s" % (name, key)]
        scaled = gold["%s/scaled/%s" % (name, key)]                          # the coordinates before the mean is taken
        err = np.abs(out[name].cpu().numpy()[0] - want).max()
        print(name, key, "centring error", err, "bound", 2.0 ** -20 * np.abs(scaled).max())
        assert err <= 2.0 ** -20 * np.abs(scaled).max()


def test_noise_scale_and_mean(DS, store):
    """fixed seed: the added noise is what separates the two calls.  Bounds for THIS draw of 2 * 3 * 2048 normals: none beyond
    6 sigma, the sample deviation within 5 % of sigma, and the mean over a cloud's 2048 points moved by less than 6 sigma / sqrt(2048)."""
    sigma, n, idx = 0.002, 2048, [ORDER.index("big")]
    base = DS.sample_clouds(store, idx, n, return_eval_cloud=True, seed=5, step=1)
    torch.manual_seed(1234)
    noisy = DS.sample_clouds(store, idx, n, return_eval_cloud=True, seed=5, step=1,
                             transform=DS.CloudTransform(cloud_noise=True, cloud_noise_scale=sigma))
    for name in ("cloud", "eval_cloud"):
        d = (noisy[name].double() - base[name].double()).cpu().numpy()[0]
        print(name, "noise std", d.std(), "max", np.abs(d).max(), "mean shift", np.abs(d.mean(axis=1)).max())
        assert np.abs(d).max() <= 6 * sigma and np.abs(d).max() > 0
        assert 0.95 * sigma <= d.std() <= 1.05 * sigma
        assert np.abs(d.mean(axis=1)).max() <= 6 * sigma / np.sqrt(n)


# ---------------------------------------------------------------------------------------------------------------
# 4. the drawn path
# ---------------------------------------------------------------------------------------------------------------
def test_drawn_equals_explicit_host_variates(DS, store):
    idx = [ORDER.index(m) for m in ("2tp3", "big", "2tp3", "one")]
    for n, ev in ((65, True), (64, False), (1, False)):
        S = 2 * n if ev else n
        drawn = DS.sample_clouds(store, idx, n, return_eval_cloud=ev, seed=77, step=3, return_faces=True)
        again = DS.sample_clouds(store, idx, n, return_eval_cloud=ev, seed=77, step=3, return_faces=True)
        expl = DS.sample_clouds(store, idx, n, return_eval_cloud=ev, variates=DS.host_variates(77, 3, len(idx), S), return_faces=True)
        for name in drawn:
            assert torch.equal(drawn[name], again[name]), name
            assert torch.equal(drawn[name], expl[name]), name
        if n > 1:
            assert not torch.equal(drawn["cloud"][0], drawn["cloud"][2])         # one mesh in two slots: two streams
            for other in (dict(seed=77, step=4), dict(seed=78, step=3)):
                assert not torch.equal(DS.sample_clouds(store, idx, n, return_eval_cloud=ev, **other)["cloud"], drawn["cloud"])


def test_drawn_faces_follow_the_areas(DS, store, meshes):
    """50 faces, 65 536 samples, fixed seed: every face with at least 1 % of the area within six binomial standard deviations"""
    v, f = meshes["fifty"]
    S = 65536
    out = DS.sample_clouds(store, [ORDER.index("fifty")], S, seed=2024, step=0, return_faces=True)
    k = out["faces"].cpu().numpy()[0]
    assert k.min() >= 0 and k.max() < len(f)
    a = MC.areas(v, f).astype(np.float64)
    p = a / a.sum()
    count = np.bincount(k, minlength=len(f))
    z = (count - S * p) / np.sqrt(S * p * (1 - p))
    big = p >= 0.01
    print("faces with >= 1 %% of the area: %d, largest |z| %.2f" % (big.sum(), np.abs(z[big]).max()))
    assert big.sum() >= 10 and (np.abs(z[big]) <= 6).all()
    pts = out["cloud"].cpu().numpy()[0]
    assert np.isfinite(pts).all() and np.abs(pts).max() <= 0.5


def test_slots_past_one_launch(DS):
    """B = 32 769 slots of one sample each, all naming the one-triangle mesh: one more than a launch of the sampler holds along y
    (dispatch::MAX_SLOTS = 32 768), so the last slot is served by a second launch.  The last slot of the first launch, the first
    of the second and slot 0 equal, bit for bit, a call with those variates alone.  The limit along x (2^22 workgroups) would
    need about 10^9 items: tests/test_chunk_dispatch_cpu.py crosses it on the host with small limits instead."""
    one = DS.MeshStore(*MC.pack([MC.one_face()]), device=dev())
    B = 32769
    var = DS.host_variates(11, 2, B, 1)
    got = DS.sample_clouds(one, [0] * B, 1, variates=var, return_faces=True)
    assert got["cloud"].shape == (B, 3, 1) and torch.isfinite(got["cloud"]).all() and bool((got["faces"] == 0).all())
    for b in (0, 32767, 32768):
        alone = DS.sample_clouds(one, [0], 1, variates=tuple(x[b:b + 1] for x in var), return_faces=True)
        for name in ("cloud", "faces"):
            assert torch.equal(got[name][b], alone[name][0]), (name, b)
        assert np.array_equal(bits(got["cloud"][b]), bits(alone["cloud"][0])), b


# ---------------------------------------------------------------------------------------------------------------
# 5. the distribution of a mesh depends on that mesh only
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["2tp3", "big", "seven"])
def test_independent_of_packing(DS, store, meshes, mesh):
    v, f = meshes[mesh]
    n = 64
    var = DS.host_variates(9, 0, 1, 2 * n)
    want_cdf = MC.tiled_edges(v, f)
    results = []
    for names, at in (([mesh, "one", "t"], 0), (["tp1", "one", mesh, "seven"], 2), ([mesh], 0), (ORDER, ORDER.index(mesh))):
        st = store if names is ORDER else make_store(DS, meshes, names)
        lo = int(st.face_bounds[at])
        cdf = st.cdf[lo:lo + len(f)].cpu().numpy()
        assert np.array_equal(bits(cdf), bits(want_cdf))                     # the contract's sums, bit for bit
        out = DS.sample_clouds(st, [at], n, return_eval_cloud=True, variates=var, return_faces=True)
        results.append(out)
    assert (np.diff(want_cdf) >= 0).all() and want_cdf[-1] == 1.0
    for out in results[1:]:
        for name in ("cloud", "eval_cloud", "faces"):
            assert torch.equal(out[name], results[0][name]), name


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals: validation comes first, on the host
# ---------------------------------------------------------------------------------------------------------------
def bad_meshes(meshes):
    v, f = meshes["tp1"]
    bad_index = (v, f.copy())
    bad_index[1][T, 2] = len(v)                                              # one past the mesh's last vertex, in the second tile
    nan_vertex = (v.copy(), f)
    nan_vertex[0][int(f[3, 1]), 0] = np.nan
    flat = (v, np.repeat(f[:, :1], 3, axis=1))                               # every face a repeated vertex: total area zero
    return bad_index, nan_vertex, flat


def test_bad_meshes_raise_at_construction(DS, meshes):
    bad_index, nan_vertex, flat = bad_meshes(meshes)
    good = meshes["seven"]
    for mesh, err in ((bad_index, IndexError), (nan_vertex, ValueError), (flat, ValueError)):
        with pytest.raises(err, match="mesh 1"):
            DS.MeshStore(*MC.pack([good, mesh, good]), device=dev())


def test_non_strict_store_refuses_only_the_bad_meshes(DS, meshes):
    bad_index, nan_vertex, flat = bad_meshes(meshes)
    names = ["2tp3", "seven", "spread300"]
    st = DS.MeshStore(*MC.pack([meshes["2tp3"], bad_index, meshes["seven"], nan_vertex, flat, meshes["spread300"]]), device=dev(), strict=False)
    assert st.bad == {1: 1, 3: 2, 4: 4}
    for m, err in ((1, IndexError), (3, ValueError), (4, ValueError)):
        with pytest.raises(err):
            DS.sample_clouds(st, [0, m, 2], 16)
    clean = DS.MeshStore(*MC.pack([meshes[n] for n in names]), device=dev())
    var = DS.host_variates(1, 2, 3, 64)
    got = DS.sample_clouds(st, [0, 2, 5], 32, return_eval_cloud=True, variates=var, return_faces=True)
    want = DS.sample_clouds(clean, [0, 1, 2], 32, return_eval_cloud=True, variates=var, return_faces=True)
    for name in ("cloud", "eval_cloud", "faces"):
        assert torch.equal(got[name], want[name]), name
    assert torch.isfinite(got["cloud"]).all()


def test_argument_refusals(DS, store):
    u, s1, s2 = DS.host_variates(0, 0, 1, 8)
    with pytest.raises(IndexError, match="outside the store"):
        DS.sample_clouds(store, [len(ORDER)], 8)
    with pytest.raises(IndexError):
        DS.sample_clouds(store, [-1], 8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        DS.sample_clouds(store, [0], 8, variates=(torch.from_numpy(u), torch.from_numpy(s1), torch.from_numpy(s2)))
    with pytest.raises(RuntimeError, match="host integers"):
        DS.sample_clouds(store, torch.zeros(1, dtype=torch.int64, device=dev()), 8)
    with pytest.raises(TypeError, match="float64"):
        DS.sample_clouds(store, [0], 8, variates=(u.astype(np.float32), s1, s2))
    with pytest.raises(TypeError, match="float32"):
        DS.sample_clouds(store, [0], 8, variates=(u, s1.astype(np.float64), s2))
    with pytest.raises(TypeError):
        DS.sample_clouds(store, [0.5], 8)
    with pytest.raises(ValueError):
        DS.sample_clouds(store, [0], 8, variates=(u[:, :4], s1, s2))
    with pytest.raises(ValueError):
        DS.sample_clouds(store, [0], 0)
    with pytest.raises(RuntimeError, match="GPU"):
        DS.MeshStore(*MC.pack([MC.one_face()]), device="cpu")
    bare = DS.MeshStore(*MC.pack([MC.one_face()]), device=dev())
    with pytest.raises(ValueError, match="orig_s"):
        DS.sample_clouds(bare, [0], 8, transform=DS.CloudTransform(cloud_rescale2orig=True))
    assert set(DS.sample_clouds(bare, [0], 8)) == {"cloud"}
