"""The matrix-core Chamfer filter (csrc/chamfer_mfma.hip, nnm_kernel) at the smallest shapes that reach each of its paths:
the one-pass / full-chunk sweep and its ragged neighbours, a second pass, fewer waves than a workgroup has, the mu sample
larger than the cloud, a poisoned R2 (the reference-scan fallback), a near-tie chunk beside the wave-wide work list, an
offset cloud, and the CD entry point with a reused workspace.  Forced with impl = "mfma" as tests/test_gpu_chamfer.py does;
the yardstick is the C oracle, bit for bit."""
import numpy as np
import pytest
import torch

from oracle import structural as S
from oracle.gen_golden import chamfer_inputs

pytestmark = pytest.mark.gpu


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    return BK


def _filter(BK, a, b):
    old = BK.NN_IMPL
    BK.NN_IMPL = "mfma"
    try:
        out = BK.NNDistance(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    finally:
        BK.NN_IMPL = old
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _assert_same(got, ref, tag):
    """bit for bit where the oracle has numbers, NaN where it has NaN, indices equal"""
    for g, r, name in zip(got, ref, ("dist1", "idx1", "dist2", "idx2")):
        assert g.dtype == r.dtype and g.shape == r.shape, (tag, name)
        if g.dtype == np.float32:
            nan = np.isnan(r)
            assert np.array_equal(np.isnan(g), nan), (tag, name, "NaN pattern")
            assert np.array_equal(g.view(np.uint32)[~nan], r.view(np.uint32)[~nan]), (tag, name, int((g != r).sum()))
        else:
            assert np.array_equal(g, r), (tag, name, int((g != r).sum()))


def _qw(B, n, m):
    """waves per workgroup that launch_nnm (csrc/chamfer_mfma.hip) picks for a forced-filter call: 16 where that leaves at
    least 128 workgroups, else 8 where that does, else 4.  Restated here so that every case SAYS which instantiation it is
    after and fails if its shape stops selecting it."""
    def wgs(qw):
        per = qw * 32
        return B * ((n + per - 1) // per + (m + per - 1) // per)
    return 16 if wgs(16) >= 128 else (8 if wgs(8) >= 128 else 4)


# (B, n, m, instantiation).  The shapes the paths need, at B = 2 (the 4-wave workgroup serves them) and at the batch that makes
# the dispatch take the 16-wave workgroup -- the one the headline runs: fast path on | just off: ragged last tile | ragged last
# chunk | second pass of one tile with one live row | unequal and tiny | exactly the mu sample | mu sample larger than the cloud |
# half a workgroup of queries.  n = 96 and n = 512 at B = 32 are the 8-wave instantiation.
SHAPES = [(2, 1024, 1024, 4), (2, 1024, 1023, 4), (2, 1056, 1024, 4), (1, 64, 2049, 4), (2, 33, 95, 4), (2, 1, 64, 4), (2, 40, 17, 4),
          (2, 96, 1024, 4), (2, 512, 1024, 4),
          (32, 1024, 1024, 16), (32, 1024, 1023, 16), (32, 1056, 1024, 16), (32, 64, 2049, 16), (64, 33, 95, 16), (64, 1, 64, 16),
          (64, 40, 17, 16), (48, 512, 1024, 16),
          (32, 96, 1024, 8), (32, 512, 1024, 8)]


@pytest.mark.parametrize("shape", SHAPES)
def test_filter_paths_bit_exact_vs_oracle(shape):
    BK = _gpu()
    B, n, m, qw = shape
    assert _qw(B, n, m) == qw
    a, b = chamfer_inputs(3100 + n + m, B, n, m)
    _assert_same(_filter(BK, a, b), S.nndistance(a, b), shape)


@pytest.mark.parametrize("B", [2, 32])
@pytest.mark.parametrize("where", ["nan_first", "nan_64", "nan_last", "inf_query"])
def test_filter_poisoned_r2_takes_the_reference_scan(where, B):
    """One non-finite coordinate poisons R2 -- through the fragment build's own read of the candidates -- and the workgroup
    must return the reference loop's result (B = 2: 4-wave workgroups; B = 32: 16-wave, the other clouds keep the filter)."""
    BK = _gpu()
    assert _qw(B, 1024, 1024) == (16 if B == 32 else 4)
    a, b = chamfer_inputs(3200, B, 1024, 1024)
    if where == "inf_query":
        a[0, 5, 1] = np.inf
    else:
        b[0, {"nan_first": 0, "nan_64": 64, "nan_last": 1023}[where], 2] = np.nan
    with np.errstate(all="ignore"):
        ref = S.nndistance(a, b)
    _assert_same(_filter(BK, a, b), ref, (where, B))


@pytest.mark.parametrize("B,m", [(2, 1024), (32, 1024), (32, 2048)])
def test_filter_near_tie_chunk_beside_the_work_list(B, m):
    """300 copies of one point among the first 1 024 candidates, and 64 queries for which every copy is a near tie: their
    waves have more items in that chunk than the wave-wide work list takes (the per-lane loop) while the other waves go
    through the list.  m = 2 048 adds a second chunk without copies: the SAME wave then runs the per-lane loop and the list
    one after the other.  B = 32: 16-wave workgroups."""
    BK = _gpu()
    assert _qw(B, 1024, m) == (16 if B == 32 else 4)
    a, b = chamfer_inputs(3300 + m, B, 1024, m)
    b[:, 100:400] = b[:, 50:51]
    a[:, :64] = b[:, 50:51] + np.float32(1e-4) * a[:, :64]
    _assert_same(_filter(BK, a, b), S.nndistance(a, b), ("near-tie", B, m))


@pytest.mark.parametrize("B", [2, 32])
def test_filter_offset_cloud(B):
    """every coordinate + 1 000: tau must scale with the extent of the data (the centring), the bits stay the oracle's"""
    BK = _gpu()
    assert _qw(B, 1024, 1024) == (16 if B == 32 else 4)
    a, b = chamfer_inputs(3400, B, 1024, 1024)
    a += np.float32(1000.0)
    b += np.float32(1000.0)
    _assert_same(_filter(BK, a, b), S.nndistance(a, b), ("offset", B))


def test_filter_cd_entry_point_with_a_reused_workspace():
    """dpf_nndistance_cd where the filter serves it, three calls on one CDWorkspace: the oracle's distances and indices, cd =
    chamfer_per_cloud of them at the existing CD test's tolerance, identical results, tickets left at zero"""
    BK = _gpu()
    from dpf_nets_amd.networks.utils import chamfer_per_cloud
    B, n, m = 32, 2048, 2048
    a, b = chamfer_inputs(3500, B, n, m)
    ref = S.nndistance(a, b)
    ref_cd = chamfer_per_cloud(torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[2]).cuda())
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = BK.CDWorkspace(B, n, m, ta.device)
    outs = [BK.NNDistanceCD(ta, tb, ws) for _ in range(3)]
    torch.cuda.synchronize()
    _assert_same([x.cpu().numpy() for x in outs[0][:4]], ref, "cd")
    assert torch.allclose(outs[0][4].double(), ref_cd.double(), rtol=2e-6, atol=0)
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert torch.equal(x, y)
    assert int(ws.tickets().abs().sum()) == 0 and not ws.dirty


def test_library_runs_with_the_profile_switch_off():
    """The shipped library has no phase stamps: the profile build's setter is absent, and the filter runs."""
    BK = _gpu()
    from dpf_nets_amd._lib import lib
    assert not hasattr(lib(), "dpf_debug_set_nnm_prof")
    a, b = chamfer_inputs(3600, 1, 64, 64)
    _assert_same(_filter(BK, a, b), S.nndistance(a, b), "profile-off")
