"""The small kernels between the big ones and the number a user reads -- Chamfer backward, the CD / F-score reductions,
PointFlowNLL forward and backward, the weight pack of the latent prior flow -- through the C ABI, against the float64
references of tests/loss_refs.py, at sizes PAST THEIR LAUNCH CAPS and at their edges.  Every tolerance is a bound derived
from the kernel's own chain of roundings (u = 2^-24) and written next to its assertion; the one constant that rests on the
accuracy of the device expf (C_TERM) is measured, see there.

Every kernel below is launched with a capped grid and walks the rest of its work in a grid-stride loop.  "Wraps" = the loop
takes a trip more than it does at any size below the cap (a second one; a fifth for the PointFlowNLL kernels, whose grid is
sized at four elements per thread).  Whoever changes a cap resizes the test named in the last column.

| kernel (file)                                              | grid cap                      | first size that wraps            | test that crosses it |
|---|---|---|---|
| nn_grad_direct_kernel, nn_grad_scatter_kernel (chamfer.hip) | 2048 x 256 threads            | b (n + m) > 524 288              | test_chamfer_backward_vs_float64[40-8192-8192] (1.25 trips), [67-9001-7003] (2.05 trips, the cloud-1 / cloud-2 boundary at thread 603 067 = trip 1, not a multiple of 256) |
| nll_partial_kernel (nll.hip)                                | ceil(B C N / 1024) workgroups x 256, at most 256: FOUR trips per thread at every size from 769 elements on | a fifth trip: B C N > 262 144 | test_nll_forward_and_backward_vs_float64[7-3-20011-...] (7 trips), [9-3-40009-...] (17), [64-3-2048-...] (6 exactly).  Below the cap (1 .. 4 trips): [1-3-1], [4-1-300], [5-3-777], [3-5-1025] |
| nll_finish_kernel (nll.hip)                                 | one thread, serial over <= 256 partial sums | --                   | the same (256 partial sums from B C N >= 261 121 on) |
| nll_backward_kernel (nll.hip)                               | ceil(B C N / 1024) x 256, at most 1024: four trips per thread as above | a fifth trip: B C N > 1 048 576 | test_nll_forward_and_backward_vs_float64[9-3-40009-...] (1 080 243 elements: the fifth trip for 31 667 threads); test_nll_backward_optional_outputs[9-3-40009] |
| adam_kernel (adam.hip)                                      | 2048 x 256 float4             | n > 2 097 152                    | test_gpu_adam.py::test_fused_adam_step_is_bitwise_the_op_sequence[n = 2 408 261] (1.15 trips + 1 tail element), [n = 4 198 307] (two full trips, 1000 float4 of a third, 3 tail elements) |
| gprior_pack_kernel (gprior.hip)                             | 2048 x 256                    | packed floats > 524 288          | test_gprior_pack_elementwise[5-250-211] (532 970 floats: 1.02 trips), [14-512-128] (1 849 344: 3.5 trips).  Before: only through test_gpu_gprior.py::test_module_vs_oracle_and_round_trip[7-128-512-50], on the flow's outputs |
| chamfer_reduce_kernel, fscore_kernel (chamfer.hip)          | one 256-thread workgroup per cloud, strides over the row | n or m > 256 (1024 on the float4 path) | test_chamfer_reduce_vs_float64, test_fscore_reduce_vs_exact_counts (rows of 1 .. 5000) |
| enc_pack_kernel (encoder.hip)                               | 256 x 256, fixed              | the encoder's widths are compile-time constants: 172 032 fragment elements (bf16x3 / bf16x6) or 180 224 (bf16) against 65 536 threads -- EVERY call takes 2.6 - 2.75 trips; its A0 (2048) and bias (1024) loops never wrap | every encoder test, e.g. test_gpu_encoder.py::test_encoder_vs_reference_golden: a wrong second trip corrupts two thirds of the layer 1-3 weights.  No size a caller can choose changes the trip count; `int` indices reach 180 224 at most |
| et_wpack_kernel (encoder_train.hip)                         | 32 x 256 per matrix, fixed    | fixed widths again: 64 lanes x fragments = 16 384 items for the 256 x 512 matrices against 8192 threads -- two trips in EVERY call, one for the smaller matrices | every training-mode encoder test, e.g. test_gpu_encoder_train.py::test_encoder_train_vs_reference_golden.  `int` indices reach 16 384 at most |
| emd_init_kernel (emd.hip, the remainL / remainR fill)       | none: ceil((n + m) / 256) x b workgroups | never: the grid covers n + m, the loop body runs once per thread for every supported size | -- (its result is held by every approx-EMD test) |

(fscore / chamfer_reduce take b workgroups: b <= 2^31 - 1 by hipLaunch's own limit, no loop over clouds.)
"""
import math

import numpy as np
import pytest
import torch

from oracle import detrng
from tests.loss_refs import cd_ref, chamfer_grad_ref, fscore_ref, nll_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                     # unit roundoff of fp32
TINY = float(np.finfo(np.float32).tiny)            # the smallest normal
NAN = float("nan")
EINVAL = -1

# Per-term rounding constant of the PointFlowNLL kernels, in units of u: the error of  lv + d d / expf(lv)  per element and of
# the backward's elementwise outputs.  A priori: d (1 rounding), d d (1), expf (the device function; not correctly rounded),
# the division (1), the adds (2), g = gout / B (1), the products (2-3): 8-9 u if expf were within 1 ulp = 2 u.  Measured on
# the MI355X at (5, 3, 777), lv0 in [-6, 1), grad_out = 1 and -0.37 (test_nll_backward_measures_the_per_element_error prints
# it): worst |d_lv0 - ref| = 2.37 u (|g| / B)(1 + d^2 e^-lv), worst |d_s0 - ref| = 3.62 u |ref|.  C_TERM = twice the worst
# (7.25), rounded up.  (The larger cases stay below it as well: 4.60 u at (7, 3, 20011).)
C_TERM = 8.0


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd._lib import lib
    return lib()


def _stream():
    from dpf_nets_amd._lib import current_stream
    return current_stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan_like(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


# ---------------------------------------------------------------------------------------------------- Chamfer backward

def _rand_idx(seed, b, n, m):
    """(b, n) uniformly random valid indices into a cloud of m points."""
    return np.minimum((detrng.uniform(seed, b * n) * m).astype(np.int32), m - 1).reshape(b, n)


def _chamfer_inputs(seed, b, n, m, kind="random"):
    x1 = detrng.normal_f32(seed, (b, n, 3))
    x2 = detrng.normal_f32(seed + 1, (b, m, 3), 0.1, 0.8)
    gd1 = detrng.normal_f32(seed + 2, (b, n))
    gd2 = detrng.normal_f32(seed + 3, (b, m))
    if kind == "hot":                               # every query of a cloud on ONE neighbour: all atomics of a cloud on 3 addresses
        idx1 = np.full((b, n), m // 3, np.int32)
        idx2 = np.full((b, m), n - 1, np.int32)
    elif kind == "mixed":                           # half of the queries on 3 candidates, the rest anywhere
        idx1, idx2 = _rand_idx(seed + 4, b, n, m), _rand_idx(seed + 5, b, m, n)
        idx1[:, ::2] = np.array([0, m // 2, m - 1], np.int32)[_rand_idx(seed + 6, b, (n + 1) // 2, 3)]
        idx2[:, ::2] = np.array([0, n // 2, n - 1], np.int32)[_rand_idx(seed + 7, b, (m + 1) // 2, 3)]
    else:
        idx1, idx2 = _rand_idx(seed + 4, b, n, m), _rand_idx(seed + 5, b, m, n)
    return x1, x2, idx1, idx2, gd1, gd2


def _chamfer_backward(L, x1, x2, idx1, idx2, gd1, gd2):
    """dpf_nndistancegrad into NaN-filled outputs: a finite, correct result shows that the direct kernel stores (it is handed
    uninitialised memory by its callers) and that the scatter kernel adds to what the direct kernel stored, in that order."""
    b, n, _ = x1.shape
    m = x2.shape[1]
    t = [_dev(v) for v in (x1, x2, gd1, idx1, gd2, idx2)]
    g1, g2 = _nan_like(b, n, 3), _nan_like(b, m, 3)
    rc = L.dpf_nndistancegrad(b, n, t[0].data_ptr(), m, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                              t[5].data_ptr(), g1.data_ptr(), g2.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return g1.cpu().numpy(), g2.cpu().numpy()


def _assert_chamfer_grad(got, ref, tag):
    """Each term is 2 gd (a - b) in fp32: the difference and the product round (2 u |term|), the factor 2 is exact.  The k
    scattered terms and the stored direct term are added in an order the hardware chooses: k additions, each within u of the
    running sum <= sum |terms| (1 + ...).  So  |got - ref| <= (k + 3) u (|direct| + sum |scattered|)  with one u to spare, plus
    the smallest normal for sums that are exactly zero."""
    g1, g2 = got
    r1, r2, a1, a2, k1, k2 = ref
    for name, g, r, a, k in (("grad_xyz1", g1, r1, a1, k1), ("grad_xyz2", g2, r2, a2, k2)):
        assert np.isfinite(g).all(), (tag, name, "not written: %d elements" % int((~np.isfinite(g)).sum()))
        err, bound = np.abs(g - r), (k[:, :, None] + 3) * U * a + TINY
        bad = err > bound
        worst = float((err / bound).max())
        print("%s %s: worst error / bound %.3f, k up to %d" % (tag, name, worst, int(k.max())))
        assert not bad.any(), (tag, name, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)


CHAMFER_CASES = [(2, 7, 3, "random"), (3, 257, 130, "random"), (1, 1, 1, "random"), (2, 1, 5000, "random"), (2, 5000, 1, "random"),
                 (40, 8192, 8192, "random"),        # 655 360 threads' worth: between one and two trips
                 (67, 9001, 7003, "random"),        # 1 072 268: more than two; cloud 1 ends at 603 067, inside trip 1, 603 067 % 256 = 187
                 (4, 2048, 2048, "hot"), (4, 2048, 1500, "mixed")]


@pytest.mark.parametrize("b,n,m,kind", CHAMFER_CASES)
def test_chamfer_backward_vs_float64(b, n, m, kind):
    L = _gpu()
    args = _chamfer_inputs(100 + n + m, b, n, m, kind)
    got = _chamfer_backward(L, *args)
    _assert_chamfer_grad(got, chamfer_grad_ref(*args), (b, n, m, kind))


def test_chamfer_backward_on_the_searchs_own_indices():
    """The backward tied to the search: indices from NNDistance (many clustered queries share a neighbour)."""
    L = _gpu()
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    b, n, m = 3, 257, 130
    x1, x2, _, _, gd1, gd2 = _chamfer_inputs(77, b, n, m)
    x2 = (x2 * 0.05).astype(np.float32)             # a tight cloud 2: few of its points are anyone's neighbour
    _, i1, _, i2 = BK.NNDistance(_dev(x1), _dev(x2))
    idx1, idx2 = i1.cpu().numpy(), i2.cpu().numpy()
    assert idx1.dtype == np.int32 and 0 <= idx1.min() and idx1.max() < m and 0 <= idx2.min() and idx2.max() < n
    got = _chamfer_backward(L, x1, x2, idx1, idx2, gd1, gd2)
    _assert_chamfer_grad(got, chamfer_grad_ref(x1, x2, idx1, idx2, gd1, gd2), "search indices")


def test_chamfer_backward_direct_part_is_exact_and_repeatable():
    """With the other side's grad_dist all zero an output holds its direct term plus zeros: 2 gd (a - b) with the difference and
    the product rounded once each -- restated in numpy fp32 it must match exactly, and two runs bit for bit (past the cap)."""
    L = _gpu()
    b, n, m = 40, 8192, 8190
    x1, x2, idx1, idx2, gd1, gd2 = _chamfer_inputs(55, b, n, m)
    rows_n, rows_m = np.repeat(np.arange(b), n), np.repeat(np.arange(b), m)
    z1, z2 = np.zeros_like(gd1), np.zeros_like(gd2)
    a1, _ = _chamfer_backward(L, x1, x2, idx1, idx2, gd1, z2)
    b1, _ = _chamfer_backward(L, x1, x2, idx1, idx2, gd1, z2)
    assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32))
    want1 = (gd1 * np.float32(2))[:, :, None] * (x1 - x2[rows_n, idx1.ravel()].reshape(b, n, 3))
    assert want1.dtype == np.float32 and np.array_equal(a1, want1), int((a1 != want1).sum())
    _, a2 = _chamfer_backward(L, x1, x2, idx1, idx2, z1, gd2)
    _, b2 = _chamfer_backward(L, x1, x2, idx1, idx2, z1, gd2)
    assert np.array_equal(a2.view(np.uint32), b2.view(np.uint32))
    want2 = (gd2 * np.float32(2))[:, :, None] * (x2 - x1[rows_m, idx2.ravel()].reshape(b, m, 3))
    assert np.array_equal(a2, want2), int((a2 != want2).sum())


def test_chamfer_backward_argument_checks():
    L = _gpu()
    x1, x2, idx1, idx2, gd1, gd2 = _chamfer_inputs(5, 2, 7, 3)
    t = [_dev(v) for v in (x1, x2, gd1, idx1, gd2, idx2)]
    g1, g2 = _nan_like(2, 7, 3), _nan_like(2, 3, 3)
    p = [v.data_ptr() for v in t]

    def call(b, n, m, ptrs, o1=g1.data_ptr(), o2=g2.data_ptr()):
        return L.dpf_nndistancegrad(b, n, ptrs[0], m, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], o1, o2, _stream())
    assert call(0, 7, 3, p) == 0                                             # an empty batch: nothing to do, nothing touched
    assert call(0, 7, 3, [None] * 6, None, None) == 0
    assert call(2, 0, 3, p) == EINVAL and call(2, 7, 0, p) == EINVAL and call(-1, 7, 3, p) == EINVAL
    for hole in range(6):
        assert call(2, 7, 3, [None if i == hole else v for i, v in enumerate(p)]) == EINVAL
    assert call(2, 7, 3, p, None) == EINVAL and call(2, 7, 3, p, g1.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(g1).all() and torch.isnan(g2).all()


# ------------------------------------------------------------------------------------------- F-score and CD reductions

T_F = np.float32(0.001)
T_BELOW, T_ABOVE = np.nextafter(T_F, np.float32(0)), np.nextafter(T_F, np.float32(np.inf))
HITS = np.array([T_BELOW, T_F * np.float32(0.5), 0.0, TINY, -1.0], np.float32)           # strictly below the threshold
MISSES = np.array([T_F, T_ABOVE, 2 * T_F, np.inf, np.nan, 1e30], np.float32)             # the threshold itself is NOT a hit


def _fscore_rows(seed, b, n, hits):
    """(b, n) rows with exactly hits[i] entries below the threshold, at shuffled positions, hits and misses drawn from the
    values that sit right at the edge."""
    pos = np.argsort(detrng.uniform(seed, b * n).reshape(b, n), axis=1)
    rank = np.empty_like(pos)
    np.put_along_axis(rank, pos, np.broadcast_to(np.arange(n), (b, n)), axis=1)
    is_hit = rank < np.asarray(hits)[:, None]
    hv = HITS[(detrng.uniform(seed + 1, b * n) * len(HITS)).astype(np.int64).reshape(b, n)]
    mv = MISSES[(detrng.uniform(seed + 2, b * n) * len(MISSES)).astype(np.int64).reshape(b, n)]
    return np.where(is_hit, hv, mv).astype(np.float32)


def _hit_plan(seed, b, n, m):
    """Hit counts per cloud: random, with the first rows forced to the corners."""
    r = np.minimum((detrng.uniform(seed, b) * (n + 1)).astype(np.int64), n)
    p = np.minimum((detrng.uniform(seed + 1, b) * (m + 1)).astype(np.int64), m)
    corners = [(n, m), (0, m), (n, 0), (0, 0), (1, 1), (n - 1, m - 1), (n, 1), (1, m)]
    for i, (ri, pi) in enumerate(corners[:b]):
        r[i], p[i] = max(ri, 0), max(pi, 0)
    return r, p


@pytest.mark.parametrize("b,n,m", [(8, 1, 1), (1000, 255, 257), (300, 256, 1), (64, 5000, 12), (37, 2500, 2500), (1, 3, 700)])
def test_fscore_reduce_vs_exact_counts(b, n, m):
    """Hit counts are integers: one miscounted element moves F by >= 1 / 5000 relative, the float arithmetic of the kernel is
    ten roundings (five to the numerator 2 P R, four to the denominator, one division): 12 u relative against float64 from the
    exact counts, two spare.  No hit on a side: exactly 0.0, never NaN."""
    L = _gpu()
    r, p = _hit_plan(9 + n, b, n, m)
    d1, d2 = _fscore_rows(13 + n, b, n, r), _fscore_rows(17 + m, b, m, p)
    want, rr, pp = fscore_ref(d1, d2, T_F)
    assert np.array_equal(rr, r) and np.array_equal(pp, p)                   # the rows are what the plan says
    t1, t2, out = _dev(d1), _dev(d2), _nan_like(b)
    assert L.dpf_fscore_reduce(b, n, m, t1.data_ptr(), t2.data_ptr(), float(T_F), out.data_ptr(), _stream()) == 0
    got = out.cpu().numpy().astype(np.float64)
    zero = (r == 0) | (p == 0)
    assert zero.any() and (~zero).any() or b == 1
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()))), got[zero][:8]
    err = np.abs(got - want)
    assert np.all(err <= 12 * U * want), (int((err > 12 * U * want).sum()), float((err[~zero] / want[~zero]).max() / U))
    print("fscore (%d, %d, %d): worst error %.2f u" % (b, n, m, float((err[~zero] / want[~zero]).max() / U) if (~zero).any() else 0.0))


def test_fscore_reduce_at_the_threshold_and_argument_checks():
    L = _gpu()
    n, m = 300, 77
    rows1 = np.stack([np.full(n, v, np.float32) for v in (T_F, T_BELOW, T_ABOVE, np.nan, np.inf, T_BELOW)])
    rows2 = np.stack([np.full(m, v, np.float32) for v in (T_BELOW, T_BELOW, T_BELOW, T_BELOW, T_BELOW, np.nan)])
    t1, t2, out = _dev(rows1), _dev(rows2), _nan_like(6)
    assert L.dpf_fscore_reduce(6, n, m, t1.data_ptr(), t2.data_ptr(), float(T_F), out.data_ptr(), _stream()) == 0
    got = out.cpu().numpy()
    full = fscore_ref(rows1[1:2], rows2[1:2], T_F)[0][0]                     # every entry a hit on both sides: 100 (less 1e-7's share)
    assert got[0] == 0.0 and got[2] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and got[5] == 0.0, got
    assert abs(float(got[1]) - full) <= 12 * U * full and abs(full - 100.0) < 1e-6
    out.fill_(NAN)
    assert L.dpf_fscore_reduce(0, n, m, None, None, float(T_F), None, _stream()) == 0
    assert L.dpf_fscore_reduce(6, 0, m, t1.data_ptr(), t2.data_ptr(), float(T_F), out.data_ptr(), _stream()) == EINVAL
    assert L.dpf_fscore_reduce(6, n, m, None, t2.data_ptr(), float(T_F), out.data_ptr(), _stream()) == EINVAL
    assert L.dpf_fscore_reduce(6, n, m, t1.data_ptr(), t2.data_ptr(), float(T_F), None, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("b,n,m", [(33, 1024, 2048), (33, 1024, 1027), (33, 1027, 1024), (33, 1027, 2049), (5, 1, 1), (5, 1, 4), (5, 4, 1),
                                   (16, 5000, 12), (7, 4096, 8)])
def test_chamfer_reduce_vs_float64(b, n, m):
    """(n % 4, m % 4) decides between the float4 and the scalar loop for BOTH rows.  Entries span 1e-8 .. 1e2.  The add chain of
    a side: per-thread serial adds (at most ceil(n / 256) of them; the float4 path adds 3 per 1024 entries), 6 shuffle steps, 3
    adds of the wave sums, one division, the final add of the two means: (ceil(n / 256) + 10) u sum|d| / n per side."""
    L = _gpu()
    d1 = (10.0 ** detrng.uniform(200 + n, b * n, -8.0, 2.0)).astype(np.float32).reshape(b, n)
    d2 = (10.0 ** detrng.uniform(300 + m, b * m, -8.0, 2.0)).astype(np.float32).reshape(b, m)
    want, a1, a2 = cd_ref(d1, d2)
    t1, t2, out = _dev(d1), _dev(d2), _nan_like(b)
    assert L.dpf_chamfer_reduce(b, n, m, t1.data_ptr(), t2.data_ptr(), out.data_ptr(), _stream()) == 0
    got = out.cpu().numpy().astype(np.float64)
    bound = (math.ceil(n / 256) + 10) * U * a1 / n + (math.ceil(m / 256) + 10) * U * a2 / m
    err = np.abs(got - want)
    print("chamfer_reduce (%d, %d, %d): worst error / bound %.3f" % (b, n, m, float((err / bound).max())))
    assert np.all(err <= bound), (float((err / bound).max()), int(np.argmax(err / bound)))


# ------------------------------------------------------------------------------------------------------- PointFlowNLL

def _nll_operand(form, seed, B, C, N, lo, hi):
    """A (B, C, N) device view in one of the stride forms the C entry point must accept, and the same view in numpy."""
    draw = lambda shape: detrng.uniform(seed, int(np.prod(shape)), lo, hi).astype(np.float32).reshape(shape)
    if form == "1c1":                               # models.py:112-117: a (1, C, 1) tensor expanded, strides (0, 1, 0)
        base = draw((1, C, 1)); view = lambda t: t.expand(B, C, N)
    elif form == "bc1":                             # a per-cloud vector expanded, strides (C, 1, 0)
        base = draw((B, C, 1)); view = lambda t: t.expand(B, C, N)
    elif form == "dense":
        base = draw((B, C, N)); view = lambda t: t
    elif form == "bnc_t":                           # a dense (B, N, C) tensor passed transposed, strides (N C, 1, C)
        base = draw((B, N, C)); view = lambda t: t.transpose(1, 2)
    else:
        raise ValueError(form)
    dev = view(_dev(base))
    host = view(torch.from_numpy(base)).numpy()
    assert dev.shape == (B, C, N) and host.shape == (B, C, N)
    return dev, host


def _nll_case(B, C, N, mu_form, lv_form, with_sum):
    s0 = detrng.normal_f32(400 + N, (B, C, N), 0.0, 0.5)
    mu_d, mu_h = _nll_operand(mu_form, 401 + N, B, C, N, -0.5, 0.5)
    lv_d, lv_h = _nll_operand(lv_form, 402 + N, B, C, N, -6.0, 1.0)          # e^-lv from 0.37 to 403: the quadratic term matters
    sl = detrng.normal_f32(403 + N, (B, C, N), 0.0, 2.0) if with_sum else None
    return s0, mu_d, mu_h, lv_d, lv_h, sl


def _nll_forward(L, B, C, N, s0_d, mu_d, lv_d, sl_d):
    ws = _nan_like(int(L.dpf_pointflow_nll_workspace_floats()))              # the workspace may hold anything on entry
    out = _nan_like(1)
    rc = L.dpf_pointflow_nll(B, C, N, s0_d.data_ptr(), mu_d.data_ptr(), *mu_d.stride(), lv_d.data_ptr(), *lv_d.stride(),
                             sl_d.data_ptr() if sl_d is not None else None, ws.data_ptr(), out.data_ptr(), _stream())
    assert rc == 0
    return out.cpu().numpy()[0]


def _nll_backward(L, B, C, N, s0_d, mu_d, lv_d, grad_out, want=(True, True, True, True)):
    go = torch.tensor([grad_out], dtype=torch.float32, device="cuda")
    outs = [_nan_like(B, C, N) for _ in range(4)]
    ptrs = [o.data_ptr() if w else None for o, w in zip(outs, want)]
    rc = L.dpf_pointflow_nll_backward(B, C, N, s0_d.data_ptr(), mu_d.data_ptr(), *mu_d.stride(), lv_d.data_ptr(), *lv_d.stride(),
                                      go.data_ptr(), *ptrs, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _nll_backward_errors(outs, grads, s0, mu_h, lv_h, B, grad_out):
    """Per-element errors of d_s0, d_mu0, d_lv0 in units of u times their scale: |ref| for d_s0 / d_mu0 (products and one
    quotient: relative error), (|g| / B)(1 + d^2 e^-lv) for d_lv0 (a difference: both of its operands count)."""
    d = s0.astype(np.float64) - mu_h.astype(np.float64)
    scale_lv = abs(grad_out) / B * (1.0 + d * d * np.exp(-lv_h.astype(np.float64)))
    e_s0 = np.abs(outs[0] - grads[0]) / (U * np.abs(grads[0]) + TINY)
    e_mu = np.abs(outs[2] - grads[2]) / (U * np.abs(grads[2]) + TINY)
    e_lv = np.abs(outs[3] - grads[3]) / (U * scale_lv)
    return e_s0, e_mu, e_lv


NLL_CASES = [
    (1, 3, 1, "dense", "dense", True, 1.0),
    (5, 3, 777, "1c1", "bc1", True, 1.0),                                     # the model's own two forms
    (5, 3, 777, "bnc_t", "dense", False, -0.37),
    (3, 5, 1025, "bc1", "bnc_t", True, -0.37),
    (4, 1, 300, "dense", "1c1", False, 1.0),
    (7, 3, 20011, "bc1", "dense", True, 1.0),                                 # 420 231 elements: forward wraps, backward does not
    (9, 3, 40009, "bnc_t", "bc1", True, -0.37),                               # 1 080 243: past the backward's cap, partial last trip
    (64, 3, 2048, "1c1", "bc1", True, 1.0),                                   # cfg-2's own shape
]


@pytest.mark.parametrize("B,C,N,mu_form,lv_form,with_sum,grad_out", NLL_CASES)
def test_nll_forward_and_backward_vs_float64(B, C, N, mu_form, lv_form, with_sum, grad_out):
    """Forward: per-thread serial partial sums over `trips` elements, 6 shuffle steps, 3 adds of the wave sums, then nwg serial adds
    in the finish kernel, each element's term within C_TERM u of its own addends:
        |got - ref| <= 0.5 / B (trips + 10 + nwg + C_TERM) u sum|term| + u |ref|
    (the finish's fp32 constant log(2 pi) C N -- three roundings, <= 3 u of 1.84 C N, against a bound of several hundred u of
    sum|term| ~ 5 B C N / B -- and its last two operations are inside the `10`).  Backward: elementwise, C_TERM u of the scale
    of each output (_nll_backward_errors); d_sum_lv is exactly fp32(0.5 fp32(g / B))."""
    L = _gpu()
    s0, mu_d, mu_h, lv_d, lv_h, sl = _nll_case(B, C, N, mu_form, lv_form, with_sum)
    s0_d, sl_d = _dev(s0), (_dev(sl) if sl is not None else None)
    want, sum_abs, grads = nll_ref(s0, mu_h, lv_h, sl, B, grad_out)
    got = _nll_forward(L, B, C, N, s0_d, mu_d, lv_d, sl_d)
    total = B * C * N
    nwg = min((total + 1023) // 1024, 256)
    trips = math.ceil(total / (nwg * 256))
    bound = 0.5 / B * (trips + 10 + nwg + C_TERM) * U * sum_abs + U * abs(want)
    const32 = float(np.float32(1.8378770664093453) * np.float32(C) * np.float32(N))
    print("nll (%d, %d, %d): trips %d, nwg %d, got %.9g, ref %.9g, error / bound %.4f; 0.5 |fp32 constant - float64 constant| = %.3g = %.2g of the bound"
          % (B, C, N, trips, nwg, got, want, abs(float(got) - want) / bound,
             0.5 * abs(const32 - math.log(2 * math.pi) * C * N), 0.5 * abs(const32 - math.log(2 * math.pi) * C * N) / bound))
    assert np.isfinite(got) and abs(float(got) - want) <= bound, (float(got), want, bound)
    again = _nll_forward(L, B, C, N, s0_d, mu_d, lv_d, sl_d)
    assert np.array_equal(np.float32(got).view(np.uint32), np.float32(again).view(np.uint32))       # fixed-order sums
    # backward, all four outputs
    outs = _nll_backward(L, B, C, N, s0_d, mu_d, lv_d, grad_out)
    for name, o in zip(("d_s0", "d_sum_lv", "d_mu0", "d_lv0"), outs):
        assert np.isfinite(o).all(), (name, "not written: %d elements" % int((~np.isfinite(o)).sum()))
    e_s0, e_mu, e_lv = _nll_backward_errors(outs, grads, s0, mu_h, lv_h, B, grad_out)
    print("nll backward (%d, %d, %d): worst d_s0 %.2f u, d_mu0 %.2f u, d_lv0 %.2f u" % (B, C, N, e_s0.max(), e_mu.max(), e_lv.max()))
    assert e_s0.max() <= C_TERM and e_mu.max() <= C_TERM and e_lv.max() <= C_TERM, (e_s0.max(), e_mu.max(), e_lv.max())
    assert np.array_equal(outs[2], -outs[0])                                  # d_mu0 = -d_s0, the same bits
    half_g = np.float32(0.5) * (np.float32(grad_out) / np.float32(B))
    assert np.array_equal(outs[1], np.full((B, C, N), half_g, np.float32))


def test_nll_backward_measures_the_per_element_error():
    """Where C_TERM comes from: the backward's d_lv0 and d_s0 expose 1 / expf(lv) element by element.  Prints the worst error of
    both in units of u on the smallest ragged case for both values of grad_out; C_TERM must be at least twice what is seen
    here (it was chosen as that, rounded up), so a device library whose expf got worse shows up here first."""
    L = _gpu()
    worst = 0.0
    for (B, C, N, mu_form, lv_form, with_sum, _) in NLL_CASES[1:3]:
        for grad_out in (1.0, -0.37):
            s0, mu_d, mu_h, lv_d, lv_h, sl = _nll_case(B, C, N, mu_form, lv_form, with_sum)
            _, _, grads = nll_ref(s0, mu_h, lv_h, sl, B, grad_out)
            outs = _nll_backward(L, B, C, N, _dev(s0), mu_d, lv_d, grad_out)
            e_s0, _, e_lv = _nll_backward_errors(outs, grads, s0, mu_h, lv_h, B, grad_out)
            print("measured (%d, %d, %d) %s/%s grad_out %g: d_s0 %.3f u, d_lv0 %.3f u" % (B, C, N, mu_form, lv_form, grad_out, e_s0.max(), e_lv.max()))
            worst = max(worst, float(e_s0.max()), float(e_lv.max()))
    assert 2.0 * worst <= C_TERM, worst


@pytest.mark.parametrize("B,C,N", [(5, 3, 777), (9, 3, 40009)])
def test_nll_backward_optional_outputs(B, C, N):
    """Each of the four gradient outputs NULL in turn: the other three carry the bits of the all-present call, and the buffer
    that was not handed over stays untouched (NaN)."""
    L = _gpu()
    s0, mu_d, mu_h, lv_d, lv_h, _ = _nll_case(B, C, N, "bc1", "bnc_t", False)
    s0_d = _dev(s0)
    full = _nll_backward(L, B, C, N, s0_d, mu_d, lv_d, -0.37)
    assert all(np.isfinite(o).all() for o in full)
    for hole in range(4):
        part = _nll_backward(L, B, C, N, s0_d, mu_d, lv_d, -0.37, want=tuple(i != hole for i in range(4)))
        for i in range(4):
            if i == hole:
                assert np.isnan(part[i]).all()
            else:
                assert np.array_equal(part[i].view(np.uint32), full[i].view(np.uint32)), (hole, i)
    go = torch.ones(1, device="cuda")
    args = (s0_d.data_ptr(), mu_d.data_ptr(), *mu_d.stride(), lv_d.data_ptr(), *lv_d.stride())
    assert L.dpf_pointflow_nll_backward(B, C, N, *args, None, None, None, None, None, _stream()) == EINVAL      # no grad_out
    assert L.dpf_pointflow_nll_backward(0, C, N, *args, go.data_ptr(), None, None, None, None, _stream()) == EINVAL
    assert L.dpf_pointflow_nll(B, C, N, *args, None, None, go.data_ptr(), _stream()) == EINVAL                  # no workspace


# ------------------------------------------------------------------------------------- latent prior flow: weight pack

def _gprior_canon(seed, S, K, nf):
    """Per step, per net (mu then logvar), the layout comment of csrc/gprior.hip:
        W0 [nf][K] | bn.weight | bn.bias | bn.running_mean | bn.running_var | W1 [K][nf] | b1 [K]"""
    nets = []
    for i in range(2 * S):
        s = seed + 10 * i
        nets.append(dict(W0=detrng.normal_f32(s, (nf, K)), gamma=detrng.uniform_f32(s + 1, (nf,), 0.5, 1.5),
                         beta=detrng.normal_f32(s + 2, (nf,)), mean=detrng.normal_f32(s + 3, (nf,)),
                         var=detrng.uniform_f32(s + 4, (nf,), 0.1, 2.0), W1=detrng.normal_f32(s + 5, (K, nf)),
                         b1=detrng.normal_f32(s + 6, (K,))))
    flat = np.concatenate([np.concatenate([n_[k].ravel() for k in ("W0", "gamma", "beta", "mean", "var", "W1", "b1")]) for n_ in nets])
    return nets, flat.astype(np.float32)


@pytest.mark.parametrize("S,G,nf", [(5, 250, 211), (14, 512, 128), (2, 6, 5)])
def test_gprior_pack_elementwise(S, G, nf):
    """What dpf_gprior_pack wrote, element by element, against the packed layout
        W0t [K][nf] | a [nf] | c [nf] | W1t [nf][K] | b1 [K],   a = gamma / sqrt(var + eps), c = beta - mean a
    The transposes and b1 are copies: exact.  a and c are formed in double and rounded once (u each); held to 2 u relative for
    a, and for c to 2 u of |beta| + |mean a| (a difference: relative to its operands, it may cancel).  Formed in fp32 -- the
    sum, the square root and the quotient each rounding, 2.5 u at worst -- a was 2.05 u (5, 250, 211) and 2.09 u (14, 512, 128)
    off, c 2.04 u: this test is why the kernel folds in double."""
    L = _gpu()
    K, eps = G // 2, 1e-5
    nets, flat = _gprior_canon(900 + G, S, K, nf)
    assert flat.size == S * L.dpf_gprior_canon_floats(G, nf)
    total = int(L.dpf_gprior_packed_floats(S, G, nf))
    assert total == 2 * S * (2 * nf * K + 2 * nf + K)
    canon, packed = _dev(flat), _nan_like(total)
    assert L.dpf_gprior_pack(S, G, nf, eps, canon.data_ptr(), packed.data_ptr(), _stream()) == 0
    got = packed.cpu().numpy().reshape(2 * S, -1)
    assert np.isfinite(got).all(), "not written: %d elements" % int((~np.isfinite(got)).sum())
    worst_a = worst_c = 0.0
    for i, n_ in enumerate(nets):
        o = 0
        assert np.array_equal(got[i, o:o + K * nf].reshape(K, nf), n_["W0"].T), (i, "W0t"); o += K * nf
        a = n_["gamma"].astype(np.float64) / np.sqrt(n_["var"].astype(np.float64) + float(np.float32(eps)))
        ea = np.abs(got[i, o:o + nf] - a) / (U * np.abs(a)); o += nf
        c_scale = np.abs(n_["beta"].astype(np.float64)) + np.abs(n_["mean"].astype(np.float64) * a)
        ec = np.abs(got[i, o:o + nf] - (n_["beta"].astype(np.float64) - n_["mean"].astype(np.float64) * a)) / (U * c_scale); o += nf
        worst_a, worst_c = max(worst_a, float(ea.max())), max(worst_c, float(ec.max()))
        assert np.array_equal(got[i, o:o + nf * K].reshape(nf, K), n_["W1"].T), (i, "W1t"); o += nf * K
        assert np.array_equal(got[i, o:o + K], n_["b1"]), (i, "b1"); o += K
        assert o == got.shape[1]
    print("gprior_pack (%d, %d, %d): %d floats, worst a %.3f u, worst c %.3f u" % (S, G, nf, total, worst_a, worst_c))
    assert worst_a <= 2.0 and worst_c <= 2.0, (worst_a, worst_c)
