"""dpf_emd_exact where tests/test_gpu_emd_exact.py (sizes 1, 2, 63, 64, 65, 256, 2 048) does not go: ragged slices, the 256 -> 1 024
thread switch, the streamed kernel and the resident one at its LDS limit, grids of 1, 2 and 24 bits, the pairwise entry with
N1 != N2 and chunked rows, the gradient past one block, zero and extreme extents, max_rounds == 0.  The oracle is
tests/emd_exact_ref.py (held to scipy on all of these cases in tests/test_emd_exact_ref_cpu.py); a case's oracle is computed once.

The slices a lone or late bidder's scan is cut into, from the kernel's two lines
    while (2 * S * k <= W && n / (2 * S) >= 64) S *= 2;          len = (ceil(n / S) + 63) & ~63
with k the bidders of the round and W the waves (4 for 65 <= n <= 512, 16 above; dispatch::ee_form).  layout() below restates
them and test_the_slice_layouts_the_sizes_were_chosen_for asserts this table:
    n      W   k = 1                                     more bidders
    127    4   never sliced (n / 2 < 64)
    128    4   S 2, len 64: 64 + 64                      k = 2: the same
    129    4   S 2, len 128: 128 + ONE candidate         k = 2: the same
    191    4   S 2, len 128: 128 + 63                    k = 2: the same
    257    4   S 4, len 128: 128, 128, ONE, one EMPTY    k = 2: S 2, len 192: 192 + 65
    512    4   S 4, len 128: four full slices            k = 2: S 2, len 256
    513   16   S 8, len 128: 4 full, ONE, three EMPTY    k = 2: the same S 8; k = 3, 4: S 4, len 192: 192, 192, 129, one empty;
                                                         k = 5 .. 8: S 2, len 320: 320 + 193
    1025  16   S 16, len 128: 8 full, ONE, seven EMPTY   k = 2: S 8, len 192: 5 full, 65, two empty; k = 3, 4: S 4, len 320:
                                                         3 full + 65; k = 5 .. 8: S 2, len 576: 576 + 449
An empty slice hands the merge (u1 INF, j 0x7fffffff, price 0); `lattice` and `collapsed` have equal u across slices, so the
lowest-index rule is decided between slices of unequal length.

What the cases cost: the numpy oracle on one CPU core (seconds), and the rounds / bids the kernel then needs (every case has
bids > n: objects change hands).  B = 2 (seeds 100 n, 100 n + 1) up to 513, B = 1 at 1 025.
    n      gauss                        lattice                      collapsed
    127    0.01 s    442 /     3 146    0.01 s    232 /     2 661    0.20 s   8 643 /    80 652
    128    0.02 s    843 /     3 464    0.01 s    192 /     2 784    0.19 s   8 459 /    81 611
    129    0.01 s    622 /     3 502    0.02 s    869 /     3 591    0.19 s   8 780 /    83 210
    191    0.02 s    904 /     5 900    0.20 s  9 864 /    16 980    0.32 s  13 437 /   176 742
    257    0.03 s  1 304 /     7 206    0.03 s  1 025 /    14 366    0.47 s  17 612 /   313 676
    512    0.10 s  2 769 /    18 147    0.10 s  1 259 /    47 949    2.08 s  35 209 / 1 343 369
    513    0.10 s  2 936 /    19 051    0.19 s  6 076 /    55 531    2.11 s  35 789 / 1 349 069
    1025   0.37 s 10 221 /    51 746    1.01 s 22 278 /   217 793    15.5 s  72 652 / 5 320 652 -> replaced by `jitter`:
                                                                     0.43 s   7 381 /    63 736
(the second seed is within a factor of three of the first, `collapsed` identical.)
`jitter` (b = a[perm] + JITTER * noise) at 4 096 / 4 097 points, by amplitude -- seconds, rounds / bids; `perm` itself needs 11
rounds and 45 056 bids:
    0.02  2.6 s   1 208 /  63 301           0.05  2.7 s   5 128 /  80 190
    0.1   3.7 s  16 404 / 149 764    /  4.3 s  14 187 / 144 341
    0.2   5.4 s  34 577 / 198 642    /  4.4 s  23 246 / 166 074
    0.3   5.0 s  22 614 / 196 533    /  4.1 s  19 011 / 158 068
    0.5   4.8 s  20 648 / 196 961    /  5.0 s  22 923 / 201 847
    1.0   6.5 s  27 463 / 255 220    /  6.4 s  42 384 / 278 240
    2.0   8.3 s  35 791 / 386 883    /  8.0 s  22 820 / 361 794      <- emd_exact_ref.JITTER, the largest tried
Grids of 1, 2 and 24 bits at 65 and 257 points: under 0.6 s a pair (collapsed, 257, 24 bits: 21 441 rounds / 383 297 bids);
at 1 bit gauss 257 needs 3 738 rounds / 86 013 bids for a qcost of 0: the tie rules alone."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import emd_exact_ref as R                                                                   # noqa: E402
from emd_exact_common import U, check_pair, clouds, dev, run, same_bits                     # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
ENOSUP = -2                                                                                 # DPF_ENOSUP (include/dpf_hip.h)
RAGGED = (127, 128, 129, 191, 257, 512, 513, 1025)
_ORACLE, _DEVICE = {}, {}


def ragged_case(kind, n):
    """(kind, B) of a ragged-size case: at 1 025 points one pair, and `collapsed` (15 s on the oracle) gives way to `jitter`"""
    if n < 1025:
        return kind, 2
    return ("jitter" if kind == "collapsed" else kind), 1


def oracle(kind, n, B, bits=R.BITS):
    key = (kind, n, B, bits)
    if key not in _ORACLE:
        a, b, _ = clouds(kind, n, B)
        _ORACLE[key] = [R.solve(a[k], b[k], bits=bits) for k in range(B)]
    return _ORACLE[key]


def device(kind, n, B, bits=R.BITS):
    key = (kind, n, B, bits)
    if key not in _DEVICE:
        a, b, _ = clouds(kind, n, B)
        _DEVICE[key] = run(a, b, bits=bits)
    return _DEVICE[key]


def run_c(a, b, bits=R.BITS, max_rounds=1 << 20, form=0):
    """dpf_emd_exact itself on a numpy (B, n, 3) pair -> (rc, cost, assignment, qcost, status, inverse)"""
    from dpf_nets_amd._lib import lib, current_stream
    B, n = a.shape[0], a.shape[1]
    ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
    asg = torch.full((B, n), -7, dtype=torch.int32, device=dev())
    inv = torch.full((B, n), -7, dtype=torch.int32, device=dev())
    qcost = torch.full((B,), -7, dtype=torch.int64, device=dev())
    cost = torch.full((B,), -7.0, dtype=torch.float32, device=dev())
    status = torch.full((B,), -7, dtype=torch.int32, device=dev())
    nbytes = lib().dpf_emd_exact_workspace_bytes(B, n)
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev())
    rc = lib().dpf_emd_exact(B, n, ta.data_ptr(), n * 3, tb.data_ptr(), n * 3, bits, max_rounds, form, asg.data_ptr(), inv.data_ptr(),
                             qcost.data_ptr(), cost.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, current_stream())
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (cost, asg, qcost, status, inv))


def layout(n, k):
    """(S, [candidates per slice]) of a round with k bidders: the kernel's two lines"""
    W = 1 if n <= 64 else 4 if n <= 512 else 16
    S = 1
    while 2 * S * k <= W and n // (2 * S) >= 64:
        S *= 2
    length = (-(-n // S) + 63) & ~63
    return S, [max(0, min(n, (q + 1) * length) - q * length) for q in range(S)]


# ---- 1: ragged slices, and the thread switch at 512 / 513 -----------------------------------------------------------------------
def test_the_slice_layouts_the_sizes_were_chosen_for():
    assert layout(127, 1) == (1, [127])
    assert layout(128, 1) == layout(128, 2) == (2, [64, 64])
    assert layout(129, 1) == layout(129, 2) == (2, [128, 1])
    assert layout(191, 1) == (2, [128, 63])
    assert layout(257, 1) == (4, [128, 128, 1, 0]) and layout(257, 2) == (2, [192, 65])
    assert layout(512, 1) == (4, [128] * 4) and layout(512, 2) == (2, [256, 256])
    assert layout(513, 1) == layout(513, 2) == (8, [128] * 4 + [1, 0, 0, 0])
    assert layout(513, 3) == layout(513, 4) == (4, [192, 192, 129, 0]) and layout(513, 8) == (2, [320, 193])
    assert layout(1025, 1) == (16, [128] * 8 + [1] + [0] * 7) and layout(1025, 2) == (8, [192] * 5 + [65, 0, 0])
    assert layout(1025, 4) == (4, [320, 320, 320, 65]) and layout(1025, 8) == (2, [576, 449])


@pytest.mark.parametrize("n", RAGGED)
@pytest.mark.parametrize("kind", ("gauss", "lattice", "collapsed"))
def test_ragged_slices_against_the_oracle_in_every_form(kind, n):
    kind, B = ragged_case(kind, n)
    a, b, _ = clouds(kind, n, B)
    base = device(kind, n, B)
    cost, asg, qcost, status = base
    for k, o in enumerate(oracle(kind, n, B)):
        assert o["bids"] > n, (kind, n, k)                                                  # objects change hands: not a trivial case
        check_pair(a[k], b[k], o, cost[k], asg[k], qcost[k], status[k], (kind, n, k))
    for form in (1, 2):
        assert same_bits(run(a, b, form=form), base), (kind, n, "form", form)


# ---- 2: the streamed kernel at work, the resident one at its LDS limit ----------------------------------------------------------
@pytest.mark.parametrize("n", (4096, 4097))
def test_jitter_at_the_lds_limit_and_past_it(n):
    """4 096: the resident form's largest LDS request, and the streamed form on the same pair; 4 097: streamed by size"""
    a, b, _ = clouds("jitter", n, 1)
    o = oracle("jitter", n, 1)[0]
    assert o["bids"] > 10 * n and o["rounds"] > 1000, (o["rounds"], o["bids"])      # `perm` at these sizes: 11 rounds, 11 n bids
    base = device("jitter", n, 1)
    cost, asg, qcost, status = base
    check_pair(a[0], b[0], o, cost[0], asg[0], qcost[0], status[0], ("jitter", n))
    if n == 4096:
        assert same_bits(run(a, b, form=2), base), "streamed against resident"
        assert same_bits(run(a, b, form=1), base), "resident forced against resident by size"
    else:
        assert same_bits(run(a, b, form=2), base), "streamed forced against streamed by size"
        got = run_c(a, b, form=1)
        assert got[0] == ENOSUP, got[0]
        assert (got[4] == -7).all() and (got[2] == -7).all(), "a refused call writes nothing"
        with pytest.raises(RuntimeError, match="unsupported shape"):
            run(a, b, form=1)


# ---- 3: grids of 1, 2 and 24 bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (65, 257))
@pytest.mark.parametrize("kind", ("gauss", "lattice", "collapsed"))
@pytest.mark.parametrize("bits", (1, 2, 24))
def test_grid_bits(bits, kind, n):
    a, b, _ = clouds(kind, n, 2)
    cost, asg, qcost, status = device(kind, n, 2, bits)
    for k, o in enumerate(oracle(kind, n, 2, bits)):
        assert float(o["s"]) * 2.0 ** (R.BITS - bits) == float(oracle(kind, n, 2)[k]["s"])  # check_pair's step is this grid's
        assert o["bids"] > n
        check_pair(a[k], b[k], o, cost[k], asg[k], qcost[k], status[k], (bits, kind, n, k))


def tiny_pairs(n):
    """(B, n, 3) pairs of 2 or 3 points: random ones, and one whose four (nine) costs are all equal on a coarse grid"""
    rng = np.random.RandomState(40 + n)
    a = rng.randn(4, n, 3).astype(F32)
    b = rng.randn(4, n, 3).astype(F32)
    a[3] = 0
    a[3, :, 0] = np.arange(n)                                        # a on the x axis, b the same points one unit up: d = 1 or more,
    b[3] = a[3]                                                      # ties between the straight and the crossed matching
    b[3, :, 1] = 1
    a[2], b[2] = a[2, ::-1].copy(), a[2].copy()                      # a reversed copy: cost 0 only through the crossed matching
    return a, b


@pytest.mark.parametrize("n", (2, 3))
@pytest.mark.parametrize("bits", (1, 2))
def test_the_first_epsilon_clamped_to_one(bits, n):
    eps0 = ((n + 1) << bits) >> R.EPS0_SHIFT
    assert eps0 <= 1 and (n > 2 or eps0 == 0)                        # n == 2: the eps < 1 -> 1 branch; n == 3, 2 bits: exactly 1
    a, b = tiny_pairs(n)
    cost, asg, qcost, status = run(a, b, bits=bits)
    for k in range(a.shape[0]):
        o = R.solve(a[k], b[k], bits=bits)
        check_pair(a[k], b[k], o, cost[k], asg[k], qcost[k], status[k], (bits, n, k))


# ---- 4: the pairwise entry's orientation and its row chunks ---------------------------------------------------------------------
def pairwise_sets(n):
    c1 = np.stack([R.make_case("gauss", n, 7000 + i)[0] for i in range(3)])
    c2 = np.stack([R.make_case("gauss", n, 7100 + j)[1] for j in range(5)])
    key = ("pairwise", n)
    if key not in _ORACLE:
        _ORACLE[key] = [[R.solve(c1[i], c2[j]) for j in range(5)] for i in range(3)]
    return c1, c2, _ORACLE[key]


def pairwise_c(c1, c2, form):
    from dpf_nets_amd._lib import lib, check, current_stream
    N1, N2, n = c1.shape[0], c2.shape[0], c1.shape[1]
    t1, t2 = torch.from_numpy(c1).to(dev()), torch.from_numpy(c2).to(dev())
    qcost = torch.full((N1, N2), -7, dtype=torch.int64, device=dev())
    cost = torch.full((N1, N2), -7.0, dtype=torch.float32, device=dev())
    status = torch.full((N1, N2), -7, dtype=torch.int32, device=dev())
    nbytes = lib().dpf_emd_exact_workspace_bytes(N1 * N2, n)
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev())
    check(lib().dpf_pairwise_emd_exact(N1, N2, n, t1.data_ptr(), t2.data_ptr(), R.BITS, 1 << 20, form, qcost.data_ptr(), cost.data_ptr(),
                                       status.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "pairwise_emd_exact")
    return qcost.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("n", (65, 129))
def test_pairwise_orientation_and_row_chunks(n):
    c1, c2, o = pairwise_sets(n)
    t1, t2 = torch.from_numpy(c1).to(dev()), torch.from_numpy(c2).to(dev())
    want = np.array([[F32(o[i][j]["cost"] / F32(n)) for j in range(5)] for i in range(3)], F32)
    want_q = np.array([[o[i][j]["qcost"] for j in range(5)] for i in range(3)], np.int64)
    want_s = np.array([[o[i][j]["rounds"] for j in range(5)] for i in range(3)], np.int32)
    assert len(set(want.ravel().tolist())) == 15 and len(set(want_q.ravel().tolist())) == 15   # no two entries can change places unseen
    with torch.no_grad():
        M = U().pairwise_EMD_exact(t1, t2).cpu().numpy()
        assert M.shape == (3, 5) and same_bits((M,), (want,)), (M, want)
        assert same_bits((U().emd_exact(t1, t2[:3].contiguous()).cpu().numpy(),), (np.diagonal(want).copy(),)), "emd_exact's own division"
        # N2 > bs; one row a launch; one row and a remainder of bs; two rows and a partial last chunk; one launch
        for bs in (2, 5, 7, 10, 512):
            assert same_bits((U().pairwise_EMD_exact(t1, t2, bs=bs).cpu().numpy(),), (want,)), bs
    for form in (0, 2):
        qcost, cost, status = pairwise_c(c1, c2, form)
        assert qcost.shape == (3, 5) and same_bits((qcost, status), (want_q, want_s)), form
        assert same_bits(((cost / F32(n)).astype(F32),), (want,)), form
    # independent of the oracle: c_ij is symmetric and qcost the integer optimum, so the swapped call gives the transpose
    assert np.array_equal(pairwise_c(c2, c1, 0)[0], want_q.T)
    # one NaN in clouds2[3]: exactly column 3
    bad = c2.copy()
    bad[3, n // 2, 1] = np.nan
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            Mb = U().pairwise_EMD_exact(t1, torch.from_numpy(bad).to(dev()), bs=7).cpu().numpy()
    mine = [m for m in w if issubclass(m.category, RuntimeWarning)]
    assert len(mine) == 1 and "3 of 15 pairs" in str(mine[0].message) and "status -1" in str(mine[0].message), [str(m.message) for m in w]
    keep = [0, 1, 2, 4]
    assert np.isnan(Mb[:, 3]).all() and same_bits((Mb[:, keep],), (want[:, keep],))
    qcost, cost, status = pairwise_c(c1, bad, 0)
    assert (status[:, 3] == R.STATUS_REFUSED).all() and (qcost[:, 3] == -1).all() and np.isnan(cost[:, 3]).all()
    assert same_bits((qcost[:, keep], status[:, keep]), (want_q[:, keep], want_s[:, keep]))


# ---- 5: the gradient past one block ---------------------------------------------------------------------------------------------
def grads(a, b, g, full):
    ta = torch.from_numpy(a).to(dev()).requires_grad_(True)
    tb = torch.from_numpy(b).to(dev()).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if full:
            out, asg = U().emd_exact_full(ta, tb, normalise=False)[:2]
        else:
            out, asg = U().emd_exact(ta, tb, return_assignment=True)
    out.backward(torch.from_numpy(g).to(dev()))
    return ta.grad.cpu().numpy(), tb.grad.cpu().numpy(), asg.cpu().numpy()


@pytest.mark.parametrize("n", (257, 513))
def test_gradient_with_several_blocks_a_pair(n):
    """two and three blocks of 256 threads a pair, the last one with a single live thread"""
    a, b, _ = clouds("gauss", n, 3)
    g = np.array([0.75, -2.0, 1.0], F32)
    bad = b.copy()
    bad[1, n - 1, 0] = np.nan
    for full in (False, True):
        scale = 1.0 if full else 1.0 / n
        ga, gb, asg = grads(a, b, g, full)
        assert np.array_equal(asg, device("gauss", n, 3)[1])
        for k in range(3):
            wa, wb = R.grad64(a[k], b[k], asg[k], float(g[k]) * scale)
            tol = 8 * 2.0 ** -24 * abs(float(g[k])) * scale
            assert np.abs(ga[k] - wa).max() <= tol and np.abs(gb[k] - wb).max() <= tol, (n, full, k)
            assert np.abs(ga[k]).max() > 0.1 * abs(float(g[k])) * scale                     # (not a comparison of zeros)
        # pair 1 not solved: its gradients are exactly 0, its neighbours' keep their bits
        xa, xb, xasg = grads(a, bad, g, full)
        assert (xasg[1] == -1).all() and (xa[1] == 0).all() and (xb[1] == 0).all(), (n, full)
        assert same_bits((xa[[0, 2]], xb[[0, 2]], xasg[[0, 2]]), (ga[[0, 2]], gb[[0, 2]], asg[[0, 2]])), (n, full)


@pytest.mark.parametrize("n", (257, 513))
def test_gradient_entry_writes_its_region_and_nothing_else(n):
    from dpf_nets_amd._lib import lib, check, current_stream
    a, b, _ = clouds("gauss", n, 3)
    g = np.array([0.75, -2.0, 1.0], F32)
    ga, gb, asg = grads(a, b, g, True)
    inv = np.stack([np.argsort(asg[k]).astype(np.int32) for k in range(3)])
    ta, tb, tg = (torch.from_numpy(x).to(dev()) for x in (a, b, g))
    tasg, tinv = torch.from_numpy(asg).to(dev()), torch.from_numpy(inv).to(dev())
    pad, size, sentinel = 64, 3 * n * 3, -12345.0
    for with_b in (True, False):
        oa = torch.full((size + 2 * pad,), sentinel, dtype=torch.float32, device=dev())
        ob = torch.full((size + 2 * pad,), sentinel, dtype=torch.float32, device=dev())
        check(lib().dpf_emd_exact_grad(3, n, ta.data_ptr(), tb.data_ptr(), tasg.data_ptr(), tinv.data_ptr(), tg.data_ptr(),
                                       oa.data_ptr() + 4 * pad, ob.data_ptr() + 4 * pad if with_b else None, current_stream()),
              "emd_exact_grad")
        oa, ob = oa.cpu().numpy(), ob.cpu().numpy()
        assert (oa[:pad] == sentinel).all() and (oa[pad + size:] == sentinel).all(), with_b
        assert same_bits((oa[pad:pad + size].reshape(3, n, 3),), (ga,)), with_b
        if with_b:
            assert (ob[:pad] == sentinel).all() and (ob[pad + size:] == sentinel).all()
            assert same_bits((ob[pad:pad + size].reshape(3, n, 3),), (gb,))
        else:
            assert (ob == sentinel).all()


# ---- 6: zero and extreme extents on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 70, 300))
@pytest.mark.parametrize("kind", ("point", "point_signed"))
def test_a_pair_of_zero_extent_between_two_ordinary_pairs(kind, n):
    ga, gb, _ = clouds("gauss", n, 2)
    pa, pb, _ = R.make_case(kind, n, 100 * n)
    o = R.solve(pa, pb)
    assert o["status"] == 0 and o["s"] == 0 and o["rounds"] == 0
    a, b = np.stack([ga[0], pa, ga[1]]), np.stack([gb[0], pb, gb[1]])
    rc, cost, asg, qcost, status, inv = run_c(a, b)
    assert rc == 0
    ident = np.arange(n, dtype=np.int32)
    assert status[1] == 0 and qcost[1] == 0 and same_bits((cost[1],), (F32(0),)), (status[1], qcost[1], cost[1])
    assert np.array_equal(asg[1], ident) and np.array_equal(inv[1], ident)
    alone = device("gauss", n, 2)
    assert same_bits([t[[0, 2]] for t in (cost, asg, qcost, status)], alone), "the neighbours"
    for k, j in ((0, 0), (2, 1)):
        assert np.array_equal(inv[k][asg[k]], ident)
        check_pair(ga[j], gb[j], oracle("gauss", n, 2)[j], cost[k], asg[k], qcost[k], status[k], (kind, n, k))
    # a squared extent that underflows is refused, and the neighbours stay as they were
    tiny = F32(1e-30)
    a[1], b[1] = ga[0] * tiny, gb[0] * tiny
    assert R.solve(a[1], b[1])["status"] == R.STATUS_REFUSED
    rc, cost, asg, qcost, status, inv = run_c(a, b)
    assert rc == 0 and status[1] == R.STATUS_REFUSED and np.isnan(cost[1]) and qcost[1] == -1 and (asg[1] == -1).all() and (inv[1] == -1).all()
    assert same_bits([t[[0, 2]] for t in (cost, asg, qcost, status)], alone), "the neighbours of the refused pair"


def test_power_of_two_scaling_to_the_edges_of_float32():
    """Each gauss pair of 65 points scaled by 2^k down to the last k at which E * E is still normal and up to the last at which
    3 E * E is finite.  At the lower edge most dx * dx are subnormal (E ~ 2^-63, every |dx| < E): the grid of such a pair is NOT the
    unscaled one, and the device has to reproduce numpy's gradual underflow -- it is compared with the oracle AT THAT SCALE."""
    a, b, _ = clouds("gauss", 65, 3)
    xs, ys, want = [], [], []
    for k in range(3):
        lo, hi = R.scaling_edges(a[k], b[k])
        assert -80 < lo < -40 and 40 < hi < 80, (lo, hi)
        for e in (lo - 1, lo, hi, hi + 1):
            f = np.ldexp(F32(1), e)
            with np.errstate(over="ignore"):
                xs.append((a[k] * f).astype(F32))
                ys.append((b[k] * f).astype(F32))
            want.append(R.solve(xs[-1], ys[-1]))
        d = (xs[-3][:, None, :] - ys[-3][None, :, :]).astype(F32)
        sub = np.abs((d * d).astype(F32)) < np.finfo(F32).tiny
        print("pair", k, "edges", lo, hi, "subnormal or zero squares at the lower edge: %d of %d" % (sub.sum(), sub.size))
        assert sub.mean() > 0.5
    rc, cost, asg, qcost, status, inv = run_c(np.stack(xs), np.stack(ys))
    assert rc == 0
    for t, o in enumerate(want):
        tag = ("pair", t // 4, ("below", "lowest", "highest", "above")[t % 4])
        if t % 4 in (0, 3):
            assert o["status"] == R.STATUS_REFUSED, tag
            assert status[t] == R.STATUS_REFUSED and np.isnan(cost[t]) and qcost[t] == -1 and (asg[t] == -1).all(), tag
        else:
            assert o["status"] > 0, tag
            print(tag, "status", status[t], o["rounds"], "qcost", qcost[t], o["qcost"], "cost", cost[t], o["cost"])
            assert status[t] == o["rounds"] and np.array_equal(asg[t], o["assignment"]) and qcost[t] == o["qcost"], tag
            assert same_bits((cost[t],), (o["cost"],)), tag


# ---- 7: max_rounds == 0 ---------------------------------------------------------------------------------------------------------
def test_no_rounds_allowed():
    a, b, _ = clouds("gauss", 1, 3)
    cost, asg, qcost, status = run(a, b, max_rounds=0)
    for k in range(3):
        o = R.solve(a[k], b[k], max_rounds=0)
        assert o["status"] == 0 and status[k] == 0 and asg[k].tolist() == [0] and qcost[k] == o["qcost"], k
        assert same_bits((cost[k],), (o["cost"],)), k
    n = 70
    pa, pb, _ = R.make_case("point", n, 5)
    ga, gb, _ = R.make_case("gauss", n, 6)
    assert R.solve(pa, pb, max_rounds=0)["status"] == 0 and R.solve(ga, gb, max_rounds=0)["status"] == R.STATUS_CAP
    cost, asg, qcost, status = run(np.stack([pa, ga]), np.stack([pb, gb]), max_rounds=0)
    assert status[0] == 0 and cost[0] == 0 and qcost[0] == 0 and np.array_equal(asg[0], np.arange(n))
    assert status[1] == R.STATUS_CAP and np.isnan(cost[1]) and qcost[1] == -1 and (asg[1] == -1).all()
