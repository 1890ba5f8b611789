"""Plain float64 references for the loss, gradient and metric kernels, written from the formulas and not by calling the
code under test.  Each returns, beside the value, the quantities a rounding-error bound needs (sums of absolute values of the
addends, their counts).  tests/test_loss_refs_cpu.py checks every one of them against torch.autograd in float64.

    chamfer_grad_ref   nndistance.cu:139-153   grad_xyz1[b,j] = 2 gd1[b,j] (x1_j - x2[idx1_j]) - sum_{l: idx2_l = j} 2 gd2[b,l] (x2_l - x1_j)
    nll_ref            losses.py:11-15         0.5 (sum_{b,c,n} [sum_lv + lv0 + (s0 - mu0)^2 / e^lv0] / B + log(2 pi) C N)
    fscore_ref         utils.py:38-42          P = 100 mean(d2 < t), R = 100 mean(d1 < t), F = 2 P R / (P + R + 1e-7)
    cd_ref             evaluating.py:112       mean(d1) + mean(d2) per cloud
"""
import math

import numpy as np


def chamfer_grad_ref(x1, x2, idx1, idx2, gd1, gd2):
    """x1 (b,n,3), x2 (b,m,3), idx1 (b,n) into x2's points, idx2 (b,m) into x1's, gd1 (b,n), gd2 (b,m).
    -> g1, g2 (float64), a1, a2 (per element: |direct term| + sum |scattered terms|), k1, k2 (per element: number of
    scattered terms; the same for the three coordinates of a point)."""
    x1, x2, gd1, gd2 = (np.asarray(v, dtype=np.float64) for v in (x1, x2, gd1, gd2))
    idx1, idx2 = np.asarray(idx1, dtype=np.int64), np.asarray(idx2, dtype=np.int64)
    b, n, _ = x1.shape
    m = x2.shape[1]
    rows_n = np.repeat(np.arange(b), n)
    rows_m = np.repeat(np.arange(b), m)
    # direct terms: one per output point
    t1 = 2.0 * gd1[:, :, None] * (x1 - x2[rows_n, idx1.ravel()].reshape(b, n, 3))      # lands in g1[b,j] and, negated, in g2[b,idx1]
    t2 = 2.0 * gd2[:, :, None] * (x2 - x1[rows_m, idx2.ravel()].reshape(b, m, 3))      # lands in g2[b,l] and, negated, in g1[b,idx2]
    g1, g2 = t1.copy(), t2.copy()
    a1, a2 = np.abs(t1), np.abs(t2)
    k1, k2 = np.zeros((b, n), np.int64), np.zeros((b, m), np.int64)
    np.add.at(g2, (rows_n, idx1.ravel()), -t1.reshape(-1, 3))
    np.add.at(a2, (rows_n, idx1.ravel()), np.abs(t1).reshape(-1, 3))
    np.add.at(k2, (rows_n, idx1.ravel()), 1)
    np.add.at(g1, (rows_m, idx2.ravel()), -t2.reshape(-1, 3))
    np.add.at(a1, (rows_m, idx2.ravel()), np.abs(t2).reshape(-1, 3))
    np.add.at(k1, (rows_m, idx2.ravel()), 1)
    return g1, g2, a1, a2, k1, k2


def nll_ref(s0, mu0, lv0, sum_lv, B, grad_out=1.0):
    """s0 (B,C,N); mu0, lv0 anything that broadcasts to it (views with any strides included); sum_lv (B,C,N) or None.
    -> value, sum over the elements of (|sum_lv| + |lv0| + (s0 - mu0)^2 e^-lv0), and for d(value * grad_out) the gradients
    (d_s0, d_sum_lv, d_mu0, d_lv0) as FULL (B,C,N) float64 arrays (not reduced over broadcast dimensions)."""
    s0 = np.asarray(s0, dtype=np.float64)
    assert s0.shape[0] == B
    _, C, N = s0.shape
    mu = np.broadcast_to(np.asarray(mu0, dtype=np.float64), s0.shape)
    lv = np.broadcast_to(np.asarray(lv0, dtype=np.float64), s0.shape)
    sl = np.zeros_like(s0) if sum_lv is None else np.asarray(sum_lv, dtype=np.float64)
    d = s0 - mu
    iv = np.exp(-lv)
    q = d * d * iv
    value = 0.5 * (math.fsum((sl + lv + q).ravel()) / B + math.log(2.0 * math.pi) * C * N)
    sum_abs = math.fsum((np.abs(sl) + np.abs(lv) + q).ravel())
    g = float(grad_out) / B
    d_s0 = g * d * iv
    grads = (d_s0, np.full_like(s0, 0.5 * g), -d_s0, 0.5 * g * (1.0 - q))
    return value, sum_abs, grads


def fscore_ref(d1, d2, threshold):
    """d1 (b,n), d2 (b,m) float32 rows, threshold a float32.  -> F (float64, b), recall counts, precision counts.
    The comparison is the strict '<' on the float32 values themselves (exact); NaN is never below."""
    d1, d2 = np.asarray(d1, dtype=np.float32), np.asarray(d2, dtype=np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        r = (d1 < t).sum(axis=1).astype(np.int64)
        p = (d2 < t).sum(axis=1).astype(np.int64)
    recall = 100.0 * r.astype(np.float64) / d1.shape[1]
    precision = 100.0 * p.astype(np.float64) / d2.shape[1]
    return 2.0 * precision * recall / (precision + recall + 1e-7), r, p


def cd_ref(d1, d2):
    """-> cd (float64, b), sum |d1| and sum |d2| per cloud."""
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    s1 = np.array([math.fsum(r) for r in d1])
    s2 = np.array([math.fsum(r) for r in d2])
    a1 = np.array([math.fsum(np.abs(r)) for r in d1])
    a2 = np.array([math.fsum(np.abs(r)) for r in d2])
    return s1 / d1.shape[1] + s2 / d2.shape[1], a1, a2
