"""The matrix-core Chamfer filter evaluates its survivors once per PASS of 64 candidate tiles: the pass's first chunk of 32 tiles
waits, is pruned against the pass's final threshold and shares one work list with the second chunk (csrc/chamfer_mfma.hip,
DESIGN 4.4).  Shapes and clouds that sit on that logic's edges -- chunk and pass boundaries, the neighbour in the waiting chunk, in
the last one, alternating; exact ties and near-ties across the chunks; passes whose pruned list still overflows; a running minimum
carried into a second pass; non-finite input in either chunk.  Every case: the filter (forced as tests/test_gpu_chamfer.py forces
it) and the VALU scan against the CPU oracle bit for bit, both directions, and the single-launch Chamfer + CD entry
(dpf_nndistance_cd through ChamferEvaluator) against the sum of the oracle's distances."""
import numpy as np
import pytest
import torch

from oracle import structural as S
from oracle.gen_golden import chamfer_inputs

pytestmark = pytest.mark.gpu

CHUNK = 32 * 32                 # candidates of a sweep chunk
CD_RTOL = 2e-6                  # the tolerance of the existing CD tests (test_nonfinite_input_through_the_cd_and_pairwise_entry_points)


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    return BK


def _run(BK, a, b, impl):
    old = BK.NN_IMPL
    BK.NN_IMPL = impl
    try:
        out = BK.NNDistance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    finally:
        BK.NN_IMPL = old
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_same(got, ref, tag):
    """bit for bit where the reference is a number, NaN where it is NaN (a NaN's payload differs between x86 and gfx950)"""
    for g, r, name in zip(got, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, name)
        if g.dtype == np.float32:
            rn = np.isnan(r)
            assert np.array_equal(np.isnan(g), rn), (tag, name, int((np.isnan(g) != rn).sum()))
            assert np.array_equal(g.view(np.uint32)[~rn], r.view(np.uint32)[~rn]), (tag, name, int((g[~rn] != r[~rn]).sum()))
        else:
            assert np.array_equal(g, r), (tag, name, int((g != r).sum()), np.argwhere(g != r)[:4].tolist())


def _check(a, b, tag, pairwise=False):
    """filter = scan = oracle on (a, b) in both directions; the CD entry's distances, indices and per-cloud CD; optionally the
    pairwise entry (the 8- and 16-wave forms of the same kernel at these sizes).  Returns the oracle's result."""
    BK = _gpu()
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        ref = S.nndistance(a, b)
        ref_cd = ref[0].mean(1, dtype=np.float64) + ref[2].mean(1, dtype=np.float64)
    _assert_same(_run(BK, a, b, "mfma"), ref, (tag, "mfma"))
    _assert_same(_run(BK, a, b, "brute"), ref, (tag, "brute"))
    from dpf_nets_amd.networks.utils import ChamferEvaluator, pairwise_CD
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ev = ChamferEvaluator()
    for _ in range(2):                                              # the second call finds the workspace's tickets reset
        out = ev(ta, tb)
        torch.cuda.synchronize()
        _assert_same([t.cpu().numpy() for t in out[:4]], ref, (tag, "cd entry"))
        cd = out[4].cpu().numpy()
        bad = ~np.isfinite(ref_cd)
        assert np.array_equal(~np.isfinite(cd), bad), (tag, "cd entry")
        np.testing.assert_allclose(cd[~bad], ref_cd[~bad], rtol=CD_RTOL, err_msg=str(tag))
    if pairwise:
        mat = pairwise_CD(ta, tb).cpu().numpy()
        for i in range(a.shape[0]):
            for j in range(b.shape[0]):
                want = ref_cd[i]
                if i != j:
                    r = S.nndistance(a[i:i + 1], b[j:j + 1])
                    want = r[0].mean(dtype=np.float64) + r[2].mean(dtype=np.float64)
                assert abs(mat[i, j] - want) <= CD_RTOL * abs(want), (tag, "pairwise", i, j)
    return ref


# ---- chunk boundaries: one chunk (nothing waits), a full chunk + a ragged chunk of one tile, a ragged tile inside the ragged chunk,
# two full chunks, and one tile past the pass (64 tiles: the waiting chunk is evaluated before the fragments are rebuilt)
BOUNDARY_SHAPES = [(2, 96, 1024), (1, 96, 1056), (2, 96, 1040), (2, 96, 2048), (1, 2048, 96), (2, 96, 2080), (1, 2080, 1040),
                   (2, 1056, 2048)]


@pytest.mark.parametrize("shape", BOUNDARY_SHAPES)
def test_chunk_boundaries(shape):
    B, n, m = shape
    a, b = chamfer_inputs(5100 + n + m, B, n, m)
    _check(a, b, shape, pairwise=(n >= 1040 or m == 2080))


# ---- where the neighbour lies
def _placed(seed, B, n, placement):
    """n queries, 2 048 candidates: a near half (the queries are slightly moved copies of n of its points, so each query's
    neighbour is known) and a half shifted far away; the candidate order puts every query's neighbour into chunk 0, into chunk 1,
    or into chunk (query index mod 2).  Returns a, b and the chunk each query's neighbour must lie in."""
    rng = np.random.default_rng(seed)
    near = (rng.random((B, CHUNK, 3), dtype=np.float32) - 0.5)
    far = (rng.random((B, CHUNK, 3), dtype=np.float32) - 0.5)
    far[..., 0] += np.float32(3.0)
    a = near[:, :n] + (rng.random((B, n, 3), dtype=np.float32) - 0.5) * np.float32(1e-3)
    if placement == "chunk0":
        b, want = np.concatenate([near, far], 1), np.zeros(n, int)
    elif placement == "chunk1":
        b, want = np.concatenate([far, near], 1), np.ones(n, int)
    else:
        # near point k (the neighbour of query k for k < n) goes to chunk k mod 2; both chunks are half near, half far
        b = np.empty((B, 2 * CHUNK, 3), np.float32)
        b[:, 0:CHUNK:2] = near[:, 0::2]; b[:, 1:CHUNK:2] = far[:, 0::2]
        b[:, CHUNK + 1::2] = near[:, 1::2]; b[:, CHUNK::2] = far[:, 1::2]
        want = np.arange(n) % 2
    return np.ascontiguousarray(a), b, want


@pytest.mark.parametrize("placement", ["chunk0", "chunk1", "alternating"])
@pytest.mark.parametrize("n", [160, CHUNK])
def test_neighbour_in_the_waiting_chunk_or_the_last(placement, n):
    a, b, want = _placed(5200 + n, 2, n, placement)
    ref = _check(a, b, (placement, n), pairwise=(placement == "alternating"))
    assert np.array_equal(ref[1] // CHUNK, np.broadcast_to(want, ref[1].shape)), "the clouds do not place the neighbours as meant"


# ---- ties across the chunks
@pytest.mark.parametrize("order", ["copy_in_chunk1", "copy_in_chunk0_reversed", "some"])
def test_exact_duplicates_in_both_chunks_lowest_index_wins(order):
    B, n = 2, 200
    a, b = chamfer_inputs(5300 + len(order), B, n, 2 * CHUNK)
    if order == "copy_in_chunk1":
        b[:, CHUNK:] = b[:, :CHUNK]                             # candidate k and its copy k + 1 024
    elif order == "copy_in_chunk0_reversed":
        b[:, :CHUNK] = b[:, :CHUNK - 1:-1]                      # candidate k is a copy of 2 047 - k: other tile, other row
    else:
        b[:, CHUNK + 300:CHUNK + 420] = b[:, 40:160]            # a hundred and twenty of them, tiles not aligned
        b[:, 700:760] = b[:, 2 * CHUNK - 60:]
    a[:, ::3] = b[:, 5:5 + len(a[0, ::3])]                      # queries ON duplicated candidates: distance 0 twice
    ref = _check(a, b, order, pairwise=(order == "some"))
    if order != "some":
        assert (ref[1] < CHUNK).all()                           # every candidate has its copy: the lower one is in chunk 0


def _adversarial(kind, a, b):
    """the distributions of tests/test_gpu_chamfer.py's generator (near-ties within the filter's tolerance, massive exact ties)"""
    a, b = a.copy(), b.copy()
    m = b.shape[1]
    if kind == "same_x":
        a[..., 0] = 0.125; b[..., 0] = 0.125
    elif kind == "two_planes":
        a[..., 0] = np.where(a[..., 0] > 0, 0.25, -0.25); b[..., 0] = np.where(b[..., 0] > 0, 0.25, -0.25)
        b[:, m // 2:m // 2 + 100] = b[:, 100:200]
    elif kind == "line":
        a[..., 1:] = 0; b[..., 1:] = 0
    elif kind == "clustered":
        a = (np.round(a * 4) / 4 + a * 0.01).astype(np.float32); b = (np.round(b * 4) / 4 + b * 0.01).astype(np.float32)
    elif kind == "surface":
        a[..., 2] = np.sin(a[..., 0] * 9) * 0.1; b[..., 2] = np.sin(b[..., 0] * 9) * 0.1
    elif kind == "far_offset":
        a += np.float32(37.0); b += np.float32(37.0)
    elif kind == "all_equal":
        b[:] = b[:, :1]
    elif kind == "big_coords":
        a *= np.float32(1000.0); b *= np.float32(1000.0)
    elif kind == "tiny_coords":
        a *= np.float32(1e-6); b *= np.float32(1e-6)
    elif kind == "lattice":
        a = (np.round(a * 8) / 8).astype(np.float32); b = (np.round(b * 8) / 8).astype(np.float32)
    return a, b


@pytest.mark.parametrize("kind", ["same_x", "two_planes", "line", "clustered", "surface", "far_offset", "big_coords", "tiny_coords"])
def test_near_ties_across_the_chunks(kind):
    B, n, m = 2, 160, 2080
    a, b = chamfer_inputs(5400 + len(kind), B, n, m)
    a, b = _adversarial(kind, a, b)
    _check(a, b, kind)


# ---- a pass whose pruned list is still longer than the list's capacity: the per-lane loop, over both chunks' masks
@pytest.mark.parametrize("kind", ["lattice", "all_equal"])
@pytest.mark.parametrize("shape", [(2, 96, 2048), (1, 2048, 2080)])
def test_overflow_of_the_pass_list(kind, shape):
    B, n, m = shape
    a, b = chamfer_inputs(5500 + n + len(kind), B, n, m)
    a, b = _adversarial(kind, a, b)
    _check(a, b, (kind, shape))


# ---- a second pass: the running minimum is carried, the lists and the waiting chunk are not
@pytest.mark.parametrize("kind", ["uniform", "neighbours_in_pass0", "neighbours_in_pass1"])
def test_second_pass_carries_the_running_minimum(kind):
    B, n = 4, 2500
    a, b = chamfer_inputs(5600, B, n, n)
    if kind != "uniform":
        sl = slice(2 * CHUNK, None) if kind == "neighbours_in_pass0" else slice(0, 2 * CHUNK)
        b[:, sl, 0] += np.float32(3.0)                          # that pass's candidates are far from every query
    ref = _check(a, b, kind, pairwise=(kind == "uniform"))
    if kind != "uniform":
        assert ((ref[1] >= 2 * CHUNK) == (kind == "neighbours_in_pass1")).all()


# ---- non-finite input: the workgroups of that cloud take the reference's scan, the other cloud's the filter
@pytest.mark.parametrize("where", ["chunk0", "chunk1"])
def test_nan_and_inf_in_either_chunk(where):
    B, n, m = 2, 96, 2048
    a, b = chamfer_inputs(5700, B, n, m)
    k = 300 if where == "chunk0" else CHUNK + 500
    b[0, k, 1] = np.float32(np.nan)
    b[1, k + 77, 0] = np.float32(np.inf)
    _check(a, b, where)
    a2, b2 = chamfer_inputs(5701, B, n, m)
    b2[1, k, 2] = np.float32(np.nan)                            # cloud 0 stays finite beside it
    _check(a2, b2, where + "/one cloud")


def test_cd_entry_at_the_smallest_batch_the_filter_serves():
    """B <= 2 goes to the LDS-staged scan behind dpf_nndistance_cd; eight clouds of 2 048 are the smallest batch of this size its
    dispatch gives to the filter (16-wave workgroups, partial sums and tickets): the far half is chunk 1 in the even clouds and
    chunk 0 in the odd ones."""
    B, n = 8, 2 * CHUNK
    a, b = chamfer_inputs(5800, B, n, n)
    b[0::2, CHUNK:, 0] += np.float32(3.0)
    b[1::2, :CHUNK, 0] += np.float32(3.0)
    ref = _check(a, b, "cd, B = 8")
    assert (ref[1][0::2] < CHUNK).all() and (ref[1][1::2] >= CHUNK).all()
