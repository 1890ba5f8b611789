"""pairwise_EMD (networks.utils; dpf_pairwise_emd) and compute_all_metrics on the GPU: the (N1, N2) approx-EMD matrix against
the CPU oracle and against match_cost pair by pair, its independence of how the matrix is cut into launches, the per-pair
choice of kernel family, its memory (no matching anywhere), the generation metrics end to end, input errors, and two ranks; and
at ragged, unequal and extreme sizes, bit for bit against the batched entry."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import structural as S
from tests.emd_cases import assert_cost_in_contract, emd_clouds, matrix_path as _matrix_path, oracle_pair_costs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _U():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.networks import utils
    return utils


def _clouds(seed, k, n, lo=0.04, hi=0.4):
    """k Gaussian clouds of n points with per-cloud axis scales in [lo, hi): distinct shapes, inside the matrix-core range"""
    rng = np.random.default_rng(seed)
    sc = rng.uniform(lo, hi, size=(k, 1, 3))
    return (rng.standard_normal((k, n, 3)) * sc).astype(np.float32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _per_pair(U, c1, c2):
    """emd_approx of every pair as its own B = 1 call (match_cost)"""
    out = torch.empty((c1.shape[0], c2.shape[0]), dtype=torch.float32, device=c1.device)
    with torch.no_grad():
        for i in range(c1.shape[0]):
            for j in range(c2.shape[0]):
                out[i, j] = U.emd_approx(c1[i:i + 1], c2[j:j + 1])[0]
    return out


def test_pairwise_emd_vs_cpu_oracle():
    """5 x 7 matrix of 256-point clouds against oracle.structural approxmatch + matchcost of every pair, at the approx-EMD cost
    contract (rtol 1e-4).  The conditioning rule of the approx-EMD tests: the auction divides by (1e-9 + a sum of weights), and
    on clouds where a point's neighbours have all been consumed every fp32 evaluation returns its own rounding noise amplified;
    where the oracle itself is further than 1e-5 from the float64 auction, an entry may be 1e-4 + 4 x that distance off."""
    U = _U()
    n = 256
    a, b = _clouds(31, 5, n), _clouds(32, 7, n)
    got = U.pairwise_EMD(_cuda(a), _cuda(b)).cpu().numpy()
    assert got.shape == (5, 7) and np.isfinite(got).all()
    pa = np.repeat(a, 7, axis=0)                                     # pair i 7 + j = (a[i], b[j])
    pb = np.tile(b, (5, 1, 1))
    rmatch, _ = S.approxmatch(pa, pb)
    rcost = (S.matchcost(pa, pb, rmatch) / np.float32(n)).reshape(5, 7)
    for i in range(5):
        for j in range(7):
            assert_cost_in_contract(got[i, j], rcost[i, j], a[i], b[j], (i, j), div=n)


def test_pairwise_emd_vs_match_cost_2048():
    """12 x 12 matrix of 2 048-point clouds against emd_approx of every pair as a B = 1 call: rtol 1e-4, every entry finite."""
    U = _U()
    c1, c2 = _cuda(_clouds(41, 12, 2048)), _cuda(_clouds(42, 12, 2048))
    got = U.pairwise_EMD(c1, c2)
    want = _per_pair(U, c1, c2)
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, want, rtol=1e-4, atol=0)


def test_pairwise_emd_chunk_independence():
    """The whole matrix, chunkings that split rows mid-way and columns, and a sub-block agree BIT FOR BIT on shared entries
    (the slice counts depend on (n, m) alone); two calls agree bit for bit."""
    U = _U()
    c1, c2 = _cuda(_clouds(51, 7, 1024)), _cuda(_clouds(52, 8, 1024))
    whole = U.pairwise_EMD(c1, c2)
    assert torch.equal(whole, U.pairwise_EMD(c1, c2))
    for bs in (16, 24, 5, 1):                 # rows of 2 (7 = 2 + 2 + 2 + 1), rows of 3, columns of 5 + 3, single pairs
        assert torch.equal(U.pairwise_EMD(c1, c2, bs=bs), whole), bs
    sub = U.pairwise_EMD(c1[2:5], c2[3:])
    assert torch.equal(sub, whole[2:5, 3:])


def _family_case(U, n):
    c1 = _cuda(_clouds(61, 4, n))
    base2 = _clouds(62, 5, n)
    scaled = base2[1] * np.float32(60.0)                              # out of the matrix-core range
    nan = base2[2].copy()
    nan[17, 1] = np.nan
    c2 = _cuda(base2)
    c2x = _cuda(np.concatenate([base2[:3], scaled[None], base2[3:], nan[None]], axis=0))    # extra clouds at columns 3 and 6
    keep = [0, 1, 2, 4, 5]
    base = U.pairwise_EMD(c1, c2)
    got = U.pairwise_EMD(c1, c2x)
    assert torch.equal(got[:, keep], base), "an out-of-range / NaN cloud changed other entries"
    sc = _per_pair(U, c1, c2x[3:4])
    assert torch.isfinite(got[:, 3]).all()
    torch.testing.assert_close(got[:, 3:4], sc, rtol=1e-4, atol=0)
    nn = _per_pair(U, c1, c2x[6:7])
    assert torch.equal(torch.isnan(got[:, 6:7]), torch.isnan(nn)), (got[:, 6], nn[:, 0])
    # the same clouds as cloud 1: their rows
    got_t = U.pairwise_EMD(c2x, c1)
    base_t = U.pairwise_EMD(c2, c1)
    assert torch.equal(got_t[keep], base_t)
    assert torch.equal(torch.isnan(got_t[6:7]), torch.isnan(_per_pair(U, c2x[6:7], c1)))


@pytest.mark.parametrize("n", [100, 512, 2048, 2500])
def test_pairwise_emd_family_is_per_pair(n):
    """A cloud scaled by 60 (packed-VALU family) and a cloud with a NaN point beside ordinary ones: every entry not involving
    them is bit-identical to the matrix without them; the scaled cloud's entries are within 1e-4 of match_cost for the pair;
    the NaN cloud's entries are NaN exactly where match_cost's are.  Again with the matrix-core path switched off.  Both
    families then share launches: at 2 048 points their own cost-partial strides would differ (128 and 64 per pair), so this
    size also holds the common per-pair stride of the partials to account; 100 and 2 500 points are ragged (padded tiles, a
    partial last wave)."""
    U = _U()
    _family_case(U, n)
    with _matrix_path(False):
        _family_case(U, n)


# ---- ragged, unequal and extreme sizes -----------------------------------------------------------------------------------
# The matrices above are all n == m at multiples of the 128-point wave.  Below: the sizes with padded tiles and partial waves,
# tiny clouds, n != m through the C ABI (the Python wrapper refuses it), the launch limit of rows * n2 <= 65535 pairs, and both
# kernel families in one launch of more than 64 pairs.  The oracle side of every test runs one pair per host thread
# (emd_cases.oracle_emd).

def _lib():
    from dpf_nets_amd._lib import lib, check, current_stream
    return lib(), check, current_stream


def _pairwise_raw(c1, c2):
    """dpf_pairwise_emd over (c1 (rows, n, 3), c2 (n2, m, 3)) in ONE launch -> (rows, n2) costs, not divided by n"""
    L, check, stream = _lib()
    (rows, n), (n2, m) = c1.shape[:2], c2.shape[:2]
    nbytes = L.dpf_pairwise_emd_workspace_bytes(rows, n2, n, m)
    assert nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    out = torch.empty((rows, n2), dtype=torch.float32, device="cuda")
    check(L.dpf_pairwise_emd(rows, n2, n, m, c1.data_ptr(), c2.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, stream()),
          "pairwise_emd")
    torch.cuda.synchronize()
    return out


def _batched64_raw(c1, c2):
    """Every pair (c1[i], c2[j]) of the matrix through dpf_approxmatch_cost_ws at b = 64 -- the batch the pairwise entry picks its
    slice counts for -- copied into contiguous batches (pair i n2 + j at batch index i n2 + j, the batch filled up to 64 by
    repeating the pairs cyclically) -> (rows, n2) costs, not divided by n"""
    L, check, stream = _lib()
    (rows, n), (n2, m) = c1.shape[:2], c2.shape[:2]
    P, B = rows * n2, 64
    assert P <= B
    pair = torch.arange(B, device="cuda") % P
    xa, xb = c1[pair // n2].contiguous(), c2[pair % n2].contiguous()
    match = torch.empty((B, m, n), dtype=torch.float32, device="cuda")
    temp = torch.empty((B, 2 * (n + m)), dtype=torch.float32, device="cuda")
    cost = torch.empty((B,), dtype=torch.float32, device="cuda")
    nbytes = L.dpf_approxmatch_workspace_bytes(B, n, m)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    check(L.dpf_approxmatch_cost_ws(B, n, m, xa.data_ptr(), xb.data_ptr(), match.data_ptr(), temp.data_ptr(), cost.data_ptr(),
                                    ws.data_ptr(), nbytes, stream()), "approxmatch_cost_ws")
    torch.cuda.synchronize()
    return cost[:P].view(rows, n2).clone()


def _assert_matrix_vs_oracle(got, want, a, b, tag, div):
    """every entry of got (rows, n2) against the oracle's costs want (rows, n2), both divided by div, at the contract"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert np.isfinite(got).all(), tag
    for i in range(got.shape[0]):
        for j in range(got.shape[1]):
            assert_cost_in_contract(got[i, j], want[i, j], a[i], b[j], tag + (i, j), div=div)


# (N1, N2, n, kind): every kind of emd_fuzz_case at least twice; N1 = 1 and N2 = 1 both present
SWEEP = [(1, 5, 1, "uniform"), (4, 1, 1, "grid"), (3, 4, 3, "gauss"), (2, 3, 3, "dup"), (5, 2, 31, "jitter"), (2, 5, 31, "line"),
         (3, 3, 33, "clustered"), (4, 3, 33, "plane"), (3, 4, 100, "offset"), (5, 3, 100, "grid"), (2, 4, 127, "uniform"),
         (4, 2, 127, "gauss"), (3, 3, 129, "jitter"), (2, 3, 129, "dup"), (3, 2, 300, "line"), (2, 2, 300, "clustered"),
         (2, 3, 777, "plane"), (3, 2, 777, "offset"), (2, 2, 1500, "gauss"), (1, 2, 2500, "jitter"), (2, 1, 2500, "uniform")]


@functools.lru_cache(maxsize=None)
def _sweep_cases():
    """the clouds of SWEEP (seeded) and the oracle's costs of every pair, computed once for both runs of the sweep"""
    rng = np.random.default_rng(4242)
    clouds = [emd_clouds(rng, kind, N1, n, N2, n) for (N1, N2, n, kind) in SWEEP]
    pairs = [(k, i, j) for k, (N1, N2, _, _) in enumerate(SWEEP) for i in range(N1) for j in range(N2)]
    costs = [np.zeros((N1, N2), np.float32) for (N1, N2, _, _) in SWEEP]
    want = oracle_pair_costs([(clouds[k][0][i], clouds[k][1][j]) for k, i, j in pairs])
    for (k, i, j), w in zip(pairs, want):
        costs[k][i, j] = w
    return clouds, costs


@pytest.mark.parametrize("matrix", [True, False], ids=["matrix_core", "packed_valu"])
def test_pairwise_emd_ragged_sweep_vs_oracle(matrix):
    """pairwise_EMD at ragged point counts (1, 3, 31, 33, 100, 127, 129, 300, 777, 1 500, 2 500: padded tiles, partial waves, tiny
    clouds), N1 and N2 from 1 to 5, every cloud kind of emd_fuzz_case twice or more: every entry against S.approxmatch +
    S.matchcost of its pair divided by n, at rtol 1e-4 under the conditioning rule -- with the matrix-core path on, and off."""
    U = _U()
    clouds, costs = _sweep_cases()
    with _matrix_path(matrix):
        for (N1, N2, n, kind), (a, b), want in zip(SWEEP, clouds, costs):
            got = U.pairwise_EMD(_cuda(a), _cuda(b))
            assert got.shape == (N1, N2)
            _assert_matrix_vs_oracle(got, want / np.float32(n), a, b, (kind, N1, N2, n, matrix), div=n)


@pytest.mark.parametrize("matrix", [True, False], ids=["matrix_core", "packed_valu"])
@pytest.mark.parametrize("n,kind", [(33, "grid"), (129, "jitter"), (777, "offset")])
def test_pairwise_emd_bits_equal_the_64_cloud_batch(n, kind, matrix):
    """An entry of dpf_pairwise_emd has the SAME BITS as dpf_approxmatch_cost_ws at b = 64 on the same pair: the pairwise entry's
    slice counts are those of a 64-cloud batch, and everything else a pair computes (its centroid, grid exponent and range
    check in emd_mfma_prep_kernel, its passes, its cost partials) reads only its own two clouds.  That holds where the batch's
    one verdict is the pair's own: with the matrix-core path on, on clouds all in range; with it off, on any clouds (one of
    them scaled by 60 here).  8 x 8 matrices at ragged sizes, raw costs of the C ABI (before the division by n): pins the
    PairMap indexing, the per-pair verdicts and the cost stride the two families share."""
    _U()
    rng = np.random.default_rng(n)
    a, b = emd_clouds(rng, kind, 8, n, 8, n)
    if not matrix:
        a[5] *= np.float32(60.0)
    c1, c2 = _cuda(a), _cuda(b)
    with _matrix_path(matrix):
        got = _pairwise_raw(c1, c2)
        want = _batched64_raw(c1, c2)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), (got - want).abs().max()


NM_CASES = [(3, 4, 300, 129, "uniform"), (2, 3, 96, 1024, "gauss"), (2, 2, 1500, 1024, "clustered")]


@functools.lru_cache(maxsize=None)
def _nm_case(k):
    N1, N2, n, m, kind = NM_CASES[k]
    a, b = emd_clouds(np.random.default_rng(900 + k), kind, N1, n, N2, m)
    want = oracle_pair_costs([(a[i], b[j]) for i in range(N1) for j in range(N2)]).reshape(N1, N2)
    return a, b, want


@pytest.mark.parametrize("matrix", [True, False], ids=["matrix_core", "packed_valu"])
@pytest.mark.parametrize("k", range(len(NM_CASES)), ids=["%dx%d_%d_%d" % c[:4] for c in NM_CASES])
def test_pairwise_emd_n_ne_m_through_the_c_abi(k, matrix):
    """n != m, which the Python wrapper refuses, through dpf_pairwise_emd itself: (N1, N2, n, m) = (3, 4, 300, 129) and
    (2, 2, 1 500, 1 024) take multiR = n / m > 1 by integer division (2 and 1: the second ratio does not divide), (2, 3, 96,
    1 024) multiL = 10; the cost partials' stride follows n, not m.  Every entry against the oracle of its pair (rtol 1e-4
    under the conditioning rule) and bit for bit against the 64-pair batched call -- with the matrix-core path on, and off."""
    _U()
    a, b, want = _nm_case(k)
    c1, c2 = _cuda(a), _cuda(b)
    with _matrix_path(matrix):
        got = _pairwise_raw(c1, c2)
        batched = _batched64_raw(c1, c2)
    _assert_matrix_vs_oracle(got, want, a, b, NM_CASES[k] + (matrix,), div=1.0)
    assert torch.equal(got, batched), (got - batched).abs().max()


def test_pairwise_emd_at_the_launch_limit():
    """rows * n2 = 255 x 257 = 65 535 pairs of 32-point clouds in ONE call (grid y at its limit; a workspace of about 3.8 GB, as
    dpf_pairwise_emd_workspace_bytes reports), the last column scaled by 60 (the packed-VALU family beside the matrix-core one).
    Every entry is finite and has the same bits as the same row computed as a launch of its own.  The first and last row and
    column and 300 seeded entries against the oracle: with the matrix-core path off at the contract (rtol 1e-4 under the
    conditioning rule; measured over all 65 535 pairs: worst 8.8e-5), with it on within 1e-3.  (Measured with it on: 27 of the
    65 535 pairs of these 32-point clouds leave 1e-4, worst 6.5e-4 on inputs the fp32 oracle resolves to 1e-8 -- the same bits
    as dpf_approxmatch_cost_ws gives the pair alone, so it is the matrix-core family's accuracy on small clouds and not the
    pairwise entry's indexing.)  One pair more (256 x 256) is DPF_ENOSUP, and its workspace query 0."""
    _U()
    L, check, stream = _lib()
    R, C, n = 255, 257, 32
    a, b = _clouds(91, R, n), _clouds(92, C, n)
    b[-1] *= np.float32(60.0)
    c1, c2 = _cuda(a), _cuda(b)
    rng = np.random.default_rng(93)
    sel = {(0, j) for j in range(C)} | {(R - 1, j) for j in range(C)} | {(i, 0) for i in range(R)} | {(i, C - 1) for i in range(R)}
    sel |= {(int(i), int(j)) for i, j in zip(rng.integers(0, R, 300), rng.integers(0, C, 300))}
    sel = sorted(sel)
    want = oracle_pair_costs([(a[i], b[j]) for i, j in sel])
    for matrix in (True, False):
        with _matrix_path(matrix):
            got = _pairwise_raw(c1, c2)
            torch.cuda.empty_cache()
            assert got.shape == (R, C) and torch.isfinite(got).all(), matrix
            for i in range(R):
                assert torch.equal(_pairwise_raw(c1[i:i + 1], c2)[0], got[i]), (matrix, i)
        got = got.cpu().numpy()
        for (i, j), w in zip(sel, want):
            if matrix:
                assert abs(float(got[i, j]) - float(w)) <= 1e-3 * abs(float(w)), (i, j, float(got[i, j]), float(w))
            else:
                assert_cost_in_contract(got[i, j], w, a[i], b[j], (i, j))
    # one pair over the limit: refused before anything is read or launched
    assert L.dpf_pairwise_emd_workspace_bytes(256, 256, n, n) == 0
    t = torch.zeros((16,), dtype=torch.float32, device="cuda")
    assert L.dpf_pairwise_emd(256, 256, n, n, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 1 << 40, stream()) == -2


def test_pairwise_emd_mixed_families_in_a_launch_over_64_pairs():
    """A 12 x 14 matrix of 300-point clouds in ONE launch (168 pairs): clouds2 holds an out-of-range cloud (scaled by 60, column 3)
    and a cloud with a NaN point (column 10), so every row has a pair of each family, on both sides of pair index 64.  Every
    other entry is bit-identical to the 12 x 12 matrix without those two clouds; the scaled cloud's entries are within 1e-4 of the
    oracle; the NaN cloud's entries are NaN exactly where match_cost's are."""
    U = _U()
    n = 300
    a, base2 = _clouds(101, 12, n), _clouds(102, 12, n)
    scaled = base2[1] * np.float32(60.0)
    nan = base2[2].copy()
    nan[17, 1] = np.nan
    x2 = np.concatenate([base2[:3], scaled[None], base2[3:9], nan[None], base2[9:]], axis=0)
    keep = [j for j in range(14) if j not in (3, 10)]
    c1 = _cuda(a)
    base = U.pairwise_EMD(c1, _cuda(base2))
    got = U.pairwise_EMD(c1, _cuda(x2))
    assert got.shape == (12, 14)
    assert torch.equal(got[:, keep], base), "an out-of-range / NaN cloud changed other entries"
    want = oracle_pair_costs([(a[i], scaled) for i in range(12)])
    for i in range(12):
        assert abs(float(got[i, 3]) - float(want[i]) / n) <= 1e-4 * abs(float(want[i]) / n), (i, float(got[i, 3]), float(want[i]) / n)
    nn = _per_pair(U, c1, _cuda(nan[None]))
    assert torch.equal(torch.isnan(got[:, 10:11]), torch.isnan(nn)), (got[:, 10], nn[:, 0])


def test_pairwise_emd_memory_has_no_matching():
    """At (N1, N2, n) = (2, 8, 4 096) the call's peak allocation rise is at most the reported workspace plus the output -- and
    below one pair's matching (4 n m bytes)."""
    U = _U()
    from dpf_nets_amd._lib import lib
    n = 4096
    c1, c2 = _cuda(_clouds(71, 2, n)), _cuda(_clouds(72, 8, n))
    U.pairwise_EMD(c1, c2)                                           # (library loaded, kernels resident)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = U.pairwise_EMD(c1, c2)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    r512 = lambda v: (v + 511) // 512 * 512                           # noqa: E731 (the caching allocator's rounding)
    ws = lib().dpf_pairwise_emd_workspace_bytes(2, 8, n, n)
    assert rise <= r512(ws) + r512(out.numel() * 4), (rise, ws)
    assert rise < 4 * n * n, rise


def test_compute_all_metrics_end_to_end():
    """compute_all_metrics on 12 generated vs 10 reference clouds of 512 points against knn / lgan_mmd_cov over the matrices of
    _pairwise_EMD_CD_ (the reference-shaped path) in the reference's orientation.  The shapes are well separated (nearest
    neighbours 2-5 % apart in the float64 auction), so MMD agrees to 1e-4 and COV / 1-NN accuracy exactly."""
    U = _U()
    from dpf_nets_amd.metrics import evaluation_metrics as E
    smp, ref = _cuda(_clouds(2, 12, 512)), _cuda(_clouds(1002, 10, 512))
    with torch.no_grad():
        got = E.compute_all_metrics(smp, ref, 8)
        rs_cd, rs_emd = E._pairwise_EMD_CD_(ref, smp, 8)
        rr_cd, rr_emd = E._pairwise_EMD_CD_(ref, ref, 8)
        ss_cd, ss_emd = E._pairwise_EMD_CD_(smp, smp, 8)
    want = {}
    for metric, (rr, rs, ss) in (("CD", (rr_cd, rs_cd, ss_cd)), ("EMD", (rr_emd, rs_emd, ss_emd))):
        want.update({"%s-%s" % (k, metric): v for k, v in E.lgan_mmd_cov(rs.t()).items()})
        want.update({"1-NN-%s-%s" % (metric, k): v for k, v in E.knn(rr, rs, ss, 1).items() if "acc" in k})
    assert set(got) == set(want) and len(got) == 12
    for k, v in got.items():
        if "mmd" in k:
            assert abs(float(v) - float(want[k])) <= 1e-4 * abs(float(want[k])), (k, float(v), float(want[k]))
        else:
            assert float(v) == float(want[k]), (k, float(v), float(want[k]))


def test_pairwise_emd_input_errors():
    U = _U()
    a = _cuda(_clouds(81, 2, 64))
    with pytest.raises(RuntimeError):
        U.pairwise_EMD(a.cpu(), a.cpu())
    with pytest.raises(RuntimeError):
        U.pairwise_EMD(a.double(), a.double())
    with pytest.raises(AssertionError):
        U.pairwise_EMD(a, _cuda(_clouds(82, 2, 96)))
    with pytest.raises(RuntimeError):
        U.pairwise_EMD(a.clone().requires_grad_(True), a)
    with pytest.raises(RuntimeError):                                # not point-major (x, y, z)
        U.pairwise_EMD(a[..., :2].contiguous(), a[..., :2].contiguous())
    with pytest.raises(RuntimeError):
        U.pairwise_EMD(a.reshape(2, -1), a.reshape(2, -1))


def test_pairwise_emd_two_ranks_sharing_one_gpu_over_gloo():
    """pairwise_EMD(..., shard_rows=True) over two ranks (two processes sharing cuda:0, gloo) equals the single-process matrix
    bit for bit (tests/dist_worker_pairwise_emd.py)."""
    _U()
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "tests", "dist_worker_pairwise_emd.py")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "PAIRWISE_EMD_OK world=2" in r.stdout
