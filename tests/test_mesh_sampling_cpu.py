"""The host side of the mesh sampler (dpf_nets_amd/datasets/sampling.py) and the conditions its golden fixture rests on
(tests/golden/mesh_sampling.npz, tools/gen_golden_mesh_sampling.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_cases as MC                                                                     # noqa: E402

from dpf_nets_amd import datasets as DS                                                     # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "mesh_sampling.npz"))


def test_host_variates_pinned():
    u, s1, s2 = DS.host_variates(3, 5, 2, 4)
    assert u.dtype == np.float64 and s1.dtype == np.float32 and s2.dtype == np.float32 and u.shape == s1.shape == s2.shape == (2, 4)
    assert [float(x).hex() for x in u[0, :2]] == ["0x1.30e2e0be96ffcp-2", "0x1.aeffa09093d0cp-1"]
    # the construction, restated with Python integers: mix(mix(seed) ^ step) -> mix(. ^ slot) -> mix(. ^ (4 * i + stream))
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    base = mix(mix(3) ^ 5)
    for b in range(2):
        for i in range(4):
            d = [(mix(mix(base ^ b) ^ (4 * i + k)) >> 11) * 2.0 ** -53 for k in range(3)]
            assert u[b, i] == d[0] and s1[b, i] == np.float32(d[1]) and s2[b, i] == np.float32(d[2])


def test_host_variates_properties():
    u, s1, s2 = DS.host_variates(2 ** 64 + 7, 11, 3, 4096)              # (the seed is taken modulo 2^64)
    u7 = DS.host_variates(7, 11, 3, 4096)[0]
    assert np.array_equal(u, u7)
    assert u.min() >= 0.0 and u.max() < 1.0 and s1.min() >= 0.0 and s1.max() <= 1.0
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))       # 53-bit uniforms
    assert 0.45 < u.mean() < 0.55 and 0.45 < s1.mean() < 0.55 and 0.45 < s2.mean() < 0.55
    for other in (DS.host_variates(7, 12, 3, 4096), DS.host_variates(8, 11, 3, 4096)):
        assert not np.array_equal(other[0], u)
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(s1, s2)
    a = DS.host_variates(7, 11, 2, 100)
    assert np.array_equal(a[0], u[:2, :100])                            # a prefix in both directions: keyed by (slot, sample)
    with pytest.raises(ValueError):
        DS.host_variates(0, 0, 0, 4)


def test_store_refuses_bad_packing_before_touching_the_device():
    v, vb, f, fb = MC.pack([MC.one_face(), MC.seven_faces()])
    assert vb.tolist() == [0, 3, 10] and fb.tolist() == [0, 1, 8]
    bad = [
        (dict(vertices=v[:, :2]), ValueError), (dict(vertices=v.astype(np.int32)), ValueError), (dict(faces=f.astype(np.float32)), ValueError),
        (dict(vertex_bounds=vb[:2]), ValueError), (dict(vertex_bounds=np.array([1, 3, 10])), ValueError),
        (dict(face_bounds=np.array([0, 9, 8])), ValueError), (dict(face_bounds=np.array([0, 0, 8])), ValueError),
        (dict(face_bounds=fb.astype(np.float64)), ValueError), (dict(face_bounds=np.array([0, 1, 7])), ValueError),
        (dict(faces=f.astype(np.int64) - 1), IndexError),
    ]
    for change, err in bad:
        kw = dict(vertices=v, vertex_bounds=vb, faces=f, face_bounds=fb)
        kw.update(change)
        with pytest.raises(err, match="MeshStore"):
            DS.MeshStore(**kw)
    import torch
    with pytest.raises(TypeError, match="numpy"):
        DS.MeshStore(torch.from_numpy(v), vb, f, fb)
    with pytest.raises(TypeError, match="MeshStore"):
        DS.sample_clouds(object(), [0], 8)


def test_cloud_transform_reads_the_reference_keys():
    t = DS.CloudTransform(**MC.TRANSFORMS["original"])
    assert t.order() == ["rescale2orig", "recenter2orig", "translate"]
    mask, shift, scale = t.fused()
    assert mask == 7 and shift.dtype == np.float32 and np.array_equal(shift, np.array(MC.SHIFT, np.float32)) and scale == np.float32(1.0)
    t = DS.CloudTransform(cloud_rescale2orig=False, cloud_recenter2orig=False, cloud_translate=False, cloud_translate_shift=[1, 2, 3],
                          cloud_scale=True, cloud_scale_scale=2.0, cloud_noise=False, cloud_noise_scale=0.002, cloud_center=False,
                          batch_size=64)                                 # a whole config: inactive values and other keys are ignored
    assert t.order() == ["scale"] and t.fused()[0] == 8 and t.fused()[2] == np.float32(2.0) and not t.fused()[1].any()
    t = DS.CloudTransform(cloud_recenter2orig=True, cloud_noise=True, cloud_noise_scale=0.5, cloud_center=True)
    assert t.order() == ["recenter2orig", "noise", "center"] and t.fused()[0] == 2 and t.noise_scale == np.float32(0.5)
    assert DS.CloudTransform().order() == [] and DS.CloudTransform().fused()[0] == 0
    with pytest.raises(ValueError):
        DS.CloudTransform(cloud_translate=True, cloud_translate_shift=[1.0, 2.0])
    with pytest.raises(KeyError):
        DS.CloudTransform(cloud_scale=True)                              # the reference's kwargs.get would divide by None


def test_cloud_transform_tail_order_on_host_tensors():
    """noise first, then centring, cloud before eval_cloud -- the reference's order; checked on CPU tensors"""
    import torch
    x = torch.arange(24, dtype=torch.float32).reshape(1, 3, 8)
    sample = {"cloud": x.clone(), "eval_cloud": 2 * x.clone(), "orig_s": torch.ones(1)}
    g = torch.Generator().manual_seed(3)
    DS.CloudTransform(cloud_noise=True, cloud_noise_scale=0.25, cloud_center=True).tail(sample, generator=g)
    g = torch.Generator().manual_seed(3)
    n1 = torch.randn(x.shape, generator=g) * 0.25
    n2 = torch.randn(x.shape, generator=g) * 0.25
    for got, want in ((sample["cloud"], x + n1), (sample["eval_cloud"], 2 * x + n2)):
        assert torch.equal(got, want - want.mean(dim=2, keepdim=True))
    assert torch.equal(sample["orig_s"], torch.ones(1))


def test_fixture_meshes_and_cap(gold):
    for name, make in MC.MESHES.items():
        v, f = make()
        assert MC.checksum(v, f) == int(gold["crc/" + name]), name
        assert np.array_equal(MC.reference_edges(v, f), gold["edges/" + name]), name
        if name in MC.STORED:
            assert np.array_equal(v, gold["vertices/" + name]) and np.array_equal(f, gold["faces/" + name])
    a = MC.areas(*MC.seven_faces())
    assert (a[[0, 1, 6]] == 0).all() and (a[2:6] > 0).all()
    a = MC.areas(*MC.spread())
    assert len(a) == 300 and a.max() / a.min() >= 1e8
    assert [len(MC.MESHES[m]()[1]) for m in ("one", "tm1", "t", "tp1", "2tp3", "big")] == [1, MC.T - 1, MC.T, MC.T + 1, 2 * MC.T + 3, 20000]
    for mesh, n, ev, seed, forced in MC.CASES:
        key = MC.case_key(mesh, n, ev, seed)
        assert MC.near_edge(gold["u/" + key], gold["edges/" + mesh]).mean() <= 0.02, key
    for mesh, n, ev, seed in MC.TRANSFORM_CASES:
        assert not MC.near_edge(gold["u/" + MC.case_key(mesh, n, ev, seed)], gold["edges/" + mesh]).any()


def test_restated_cdf_reproduces_the_stored_reference_clouds(gold):
    sizes = set()
    for mesh, n, ev, seed, forced in MC.CASES:
        key = MC.case_key(mesh, n, ev, seed)
        v, f = MC.MESHES[mesh]()
        S = 2 * n if ev else n
        u, s1, s2 = MC.draw(seed, S, forced)
        assert np.array_equal(u, gold["u/" + key]) and np.array_equal(s1.reshape(-1), gold["s1/" + key])
        assert np.array_equal(s2.reshape(-1), gold["s2/" + key])
        k, pts = MC.restate(v, f, u, s1, s2, gold["edges/" + mesh])
        assert np.array_equal(k, gold["face/" + key])
        for name, want in MC.split(pts, ev).items():
            assert np.ascontiguousarray(want).tobytes() == gold[name + "/" + key].tobytes(), (key, name)
        assert ("eval_cloud/" + key in gold.files) == ev
        sizes.add((n, ev))
    assert {(n, e) for n in (1, 63, 64, 65, 2048) for e in (False, True)} <= sizes


def test_tiled_edges_stay_within_the_tolerance_of_the_reference_edges(gold):
    """the argument of the GPU test's acceptance rule, on the contract's own numpy restatement"""
    for name in MC.MESHES:
        mine, ref = MC.tiled_edges(*MC.MESHES[name]()), gold["edges/" + name]
        assert (np.diff(mine) >= 0).all() and mine[-1] == 1.0
        assert np.abs(mine - ref).max() <= MC.EDGE_TOL, name
