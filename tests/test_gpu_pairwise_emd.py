"""pairwise_EMD (networks.utils; dpf_pairwise_emd) and compute_all_metrics on the GPU: the (N1, N2) approx-EMD matrix against
the CPU oracle and against match_cost pair by pair, its independence of how the matrix is cut into launches, the per-pair
choice of kernel family, its memory (no matching anywhere), the generation metrics end to end, input errors, and two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import structural as S

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


class _matrix_path:
    """dpf_emd_set_matrix_path(on) for the duration of a block (restored in finally)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from dpf_nets_amd._lib import lib
        self.prev = lib().dpf_emd_set_matrix_path(1 if self.on else 0)

    def __exit__(self, *exc):
        from dpf_nets_amd._lib import lib
        lib().dpf_emd_set_matrix_path(self.prev)


def _auction64(a1, b1):
    """The approx-EMD auction (approxmatch.cu:3-182) + matchcost in float64, whole passes as matrix expressions: exact arithmetic
    for practical purposes, the measure of how well conditioned an input is for the fp32 oracle."""
    n, m = len(a1), len(b1)
    d2 = ((b1[:, None, :].astype(np.float64) - a1[None, :, :].astype(np.float64)) ** 2).sum(2)
    remL = np.full(n, 1.0 if n >= m else float(m // n))
    remR = np.full(m, float(n // m) if n >= m else 1.0)
    match = np.zeros((m, n))
    for j in range(7, -2, -1):
        e = np.exp(-(4.0 ** j) * d2)
        ratioL = remL / (1e-9 + remR @ e)
        sumr = (e @ ratioL) * remR
        ratioR = np.minimum(remR / (sumr + 1e-9), 1.0) * remR
        remR = np.maximum(0.0, remR - sumr)
        w = e * ratioR[:, None] * ratioL[None, :]
        match += w
        remL = np.maximum(0.0, remL - w.sum(0))
    return float((match * np.sqrt(d2)).sum())


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
    err = np.abs(got - rcost) / np.maximum(np.abs(rcost), 1e-6)
    for i, j in zip(*np.nonzero(err > 1e-4)):
        cond = abs(float(rcost[i, j]) * n - _auction64(a[i], b[j])) / max(abs(float(rcost[i, j]) * n), 1e-6)
        assert cond > 1e-5 and err[i, j] <= 1e-4 + 4.0 * cond, (int(i), int(j), float(err[i, j]), cond)


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


@pytest.mark.parametrize("n", [512, 2048])
def test_pairwise_emd_family_is_per_pair(n):
    """A cloud scaled by 60 (packed-VALU family) and a cloud with a NaN point beside ordinary ones: every entry not involving
    them is bit-identical to the matrix without them; the scaled cloud's entries are within 1e-4 of match_cost for the pair;
    the NaN cloud's entries are NaN exactly where match_cost's are.  Again with the matrix-core path switched off.  Both
    families then share launches: at 2 048 points their own cost-partial strides would differ (128 and 64 per pair), so this
    size also holds the common per-pair stride of the partials to account."""
    U = _U()
    _family_case(U, n)
    with _matrix_path(False):
        _family_case(U, n)


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
