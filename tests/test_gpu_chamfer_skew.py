"""The 16-wave form of the matrix-core Chamfer filter schedules its waves by progress (r11; csrc/chamfer_mfma.hip):
a wave's issue priority falls from the first chunk's sweep to the second's to the evaluation, so the waves of a SIMD no longer run
in launch order.  Scheduling must not reach the bits: every case here holds the filter (forced, as tests/test_gpu_chamfer.py
forces it), and the single-launch Chamfer + CD entry (dpf_nndistance_cd through ChamferEvaluator: 16-wave workgroups, partial
sums, tickets), to the CPU oracle bit for bit in d1, i1, d2, i2.  The oracle has no fp32 per-cloud CD: the CD is held to the sum of
the oracle's distances at the tolerance of the existing CD tests, and bit for bit to ITSELF over repeated calls (its additions have
a fixed order, so any bit that moved between two calls would be scheduling reaching a result).
Cases: chunk and pass boundaries at B = 2 and B = 32, unequal sizes, every neighbour in one chunk / alternating, duplicates at the
same offset of both chunks, clouds that leave the upper or the lower eight waves of a workgroup without a query, an odd batch, an
overflowing work list, NaN / +Inf in one chunk only, and ten repeats of the headline shape."""
import numpy as np
import pytest
import torch

from oracle import structural as S
from oracle.gen_golden import chamfer_inputs

pytestmark = pytest.mark.gpu

CHUNK = 32 * 32                 # candidates of a sweep chunk
CD_RTOL = 2e-6                  # the tolerance of the existing CD tests
# the 16-wave form serves a launch of >= 128 workgroups of 512 queries (dispatch.h nnm_qw): 22 clouds of <= 1 024 x 2 048 points
# are 132; the batches below are the smallest that reach it at their sizes (B = 2 runs the 4-wave form, which r11 leaves alone)
B16 = 22


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    return BK


def _forced(BK, a, b):
    old = BK.NN_IMPL
    BK.NN_IMPL = "mfma"
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


def _check(a, b, tag, calls=2):
    """forced filter = oracle; the CD entry's distances and indices = oracle, its CD within CD_RTOL of the oracle's sums and the
    same bits on every call (the later calls find the workspace's tickets reset).  Returns the oracle's result."""
    BK = _gpu()
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    with np.errstate(all="ignore"):
        ref = S.nndistance(a, b)
        ref_cd = ref[0].mean(1, dtype=np.float64) + ref[2].mean(1, dtype=np.float64)
    _assert_same(_forced(BK, a, b), ref, (tag, "mfma"))
    from dpf_nets_amd.networks.utils import ChamferEvaluator
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ev = ChamferEvaluator()
    first = None
    for k in range(calls):
        out = ev(ta, tb)
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in out[:4]]
        cd = out[4].cpu().numpy()
        if first is None:
            _assert_same(got, ref, (tag, "cd entry"))
            bad = ~np.isfinite(ref_cd)
            assert np.array_equal(~np.isfinite(cd), bad), (tag, "cd entry")
            np.testing.assert_allclose(cd[~bad], ref_cd[~bad], rtol=CD_RTOL, err_msg=str(tag))
            first = got + [cd]
        else:
            for g, f in zip(got + [cd], first):
                assert g.tobytes() == f.tobytes(), (tag, "call", k, "differs from call 0")
    return ref


# ---- chunk and pass boundaries: one chunk, a ragged chunk 1 of one tile, two full chunks, a ragged tile in a second pass
@pytest.mark.parametrize("n", [1024, 1056, 2048, 2080])
@pytest.mark.parametrize("B", [2, 32])
def test_small_and_ragged_chunks(B, n):
    a, b = chamfer_inputs(6100 + n + B, B, n, n)
    _check(a, b, (B, n))


@pytest.mark.parametrize("shape", [(2, 2048, 1024), (2, 1024, 2048), (22, 2048, 1024), (22, 1024, 2048), (22, 1056, 2080)])
def test_unequal_sizes(shape):
    B, n, m = shape
    a, b = chamfer_inputs(6200 + n + m + B, B, n, m)
    _check(a, b, shape)


def _placed(seed, B, n, placement):
    """n queries, 2 048 candidates: a near half (the queries are slightly moved copies of n of its points) and a half shifted far
    away; every query's neighbour lies in chunk 0, in chunk 1, or in chunk (query index mod 2)"""
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
        b = np.empty((B, 2 * CHUNK, 3), np.float32)
        b[:, 0:CHUNK:2] = near[:, 0::2]; b[:, 1:CHUNK:2] = far[:, 0::2]
        b[:, CHUNK + 1::2] = near[:, 1::2]; b[:, CHUNK::2] = far[:, 1::2]
        want = np.arange(n) % 2
    return np.ascontiguousarray(a), b, want


@pytest.mark.parametrize("placement", ["chunk0", "chunk1", "alternating"])
def test_every_neighbour_in_one_chunk(placement):
    a, b, want = _placed(6300, B16, CHUNK, placement)
    ref = _check(a, b, placement)
    assert np.array_equal(ref[1] // CHUNK, np.broadcast_to(want, ref[1].shape)), "the clouds do not place the neighbours as meant"


def test_duplicates_at_the_same_offset_of_both_chunks():
    B, n = B16, 600
    a, b = chamfer_inputs(6400, B, n, 2 * CHUNK)
    b[:, CHUNK:] = b[:, :CHUNK]                                 # candidate k and its copy k + 1 024: same tile row, other chunk
    a[:, ::3] = b[:, 5:5 + len(a[0, ::3])]                      # queries ON duplicated candidates: distance 0 twice
    ref = _check(a, b, "duplicates")
    assert (ref[1] < CHUNK).all()                               # the lower copy is in chunk 0, whichever wave finds it first


# ---- a workgroup is 16 waves x 32 queries: 200 queries leave waves 7 .. 15 without one, 512 + 200 fill the first workgroup and
# leave the second's upper waves empty; 256 + 8 puts eight queries into the first wave of the upper eight; an odd batch
@pytest.mark.parametrize("shape", [(26, 200, 2048), (22, 712, 2048), (26, 264, 2048), (33, 1024, 2048), (27, 256, 2048)])
def test_empty_halves_and_odd_batches(shape):
    B, n, m = shape
    a, b = chamfer_inputs(6500 + n + B, B, n, m)
    _check(a, b, shape)


@pytest.mark.parametrize("kind", ["lattice", "all_equal"])
def test_list_overflow(kind):
    B, n, m = B16, 600, 2048
    a, b = chamfer_inputs(6600 + len(kind), B, n, m)
    if kind == "lattice":
        a = (np.round(a * 8) / 8).astype(np.float32); b = (np.round(b * 8) / 8).astype(np.float32)
    else:
        b[:] = b[:, :1]
    _check(a, b, kind)


@pytest.mark.parametrize("where", ["chunk0", "chunk1"])
def test_non_finite_candidates_in_one_chunk(where):
    B, n, m = B16, 600, 2048
    a, b = chamfer_inputs(6700, B, n, m)
    k = 300 if where == "chunk0" else CHUNK + 500
    b[0, k, 1] = np.float32(np.nan)
    b[1, k + 77, 0] = np.float32(np.inf)                        # the other clouds stay finite beside them: the filter serves those
    _check(a, b, where)


def test_headline_shape_ten_times_identical_bits():
    a, b = chamfer_inputs(6800, 32, 2048, 2048)
    _check(a, b, "headline x 10", calls=10)
