"""The numpy restatement of dpf_dcd (include/dpf_hip.h; csrc/dcd.hip): the density-aware Chamfer distance from one nn_distance
result per cloud -- the counts, the terms in float64 with every operation rounded on its own, the 256-block pairwise tree and the
ascending block order of the sums, the loss, its halves, the gradient coefficients and refusal.

numpy's float64 scalar and array arithmetic rounds every operation on its own, so what is bit-defined in the contract (the counts,
the status, everything but exp and pow) is restated exactly; exp and pow are the host library's here and the device library's there,
neither correctly rounded, which is what DCD_BOUND is for.

DCD_BOUND, relative to max(1, frac1, frac2), for finite distances >= 0 (u = 2^-53, one rounding of a float64 operation; M = max(1, frac)):
  * exp: ROCm's device library documents 1 ULP for the float64 exp (HIP's table of double-precision mathematical functions), the host
    library stays under 1 ULP too: the two e differ by at most 2 ULP = 4 u relative, and e <= 1.                               4 u
  * pow (only where n_lambda is neither 0 nor 1): documented 1 ULP as well, the same 2 ULP between the two p; p >= 1 goes into the
    divisor, so W inherits at most the same relative difference, and W <= frac.                                                 4 u
  * one rounding per stated operation after them whose inputs may now differ -- p + 1e-6, the division, e * W, 1 - q -- each at most
    u relative to a value no larger than M on either side: 2 u each.                                                            8 u
  so two terms differ by at most 16 u M.  A term passes through at most ceil(log2 256) = 8 additions of its block's tree and
  blocks - 1 additions of the block order; the issue's count "ceil(log2 q) + blocks" covers both for every q.  Each addition rounds
  at most u relative to a partial sum of at most q M, on either side: 2 u (ceil(log2 q) + blocks) q M on the sum, the same without
  the q on the mean.  The division by q, the addition L1 + L2 and the (exact) halving: 2 u each side, 4 u.
      dcd_bound(n, m) = (16 + 4 + 2 (ceil(log2 q) + blocks(q))) * 2^-53,   q = max(n, m)
  DCD_BOUND is dcd_bound at the largest cloud the tests run (DCD_MAX_TESTED points); a test uses dcd_bound of its own shape."""
import math

import numpy as np

BLOCK = 256
REFUSED = -1
LDS_TARGETS = 32768                 # dispatch::DCD_LDS_TARGETS (tests/test_dcd_ref_cpu.py pins it)
DCD_MAX_TESTED = LDS_TARGETS + 1
U = 2.0 ** -53


def dcd_bound(n, m):
    q = max(int(n), int(m))
    depth = int(math.ceil(math.log2(q))) if q > 1 else 0
    return (16 + 4 + 2 * (depth + (q + BLOCK - 1) // BLOCK)) * U


DCD_BOUND = dcd_bound(DCD_MAX_TESTED, DCD_MAX_TESTED)


def counts(idx, targets):
    """c[i] = the number of queries that share query i's target"""
    idx = np.asarray(idx, dtype=np.int64)
    return np.bincount(idx, minlength=targets)[idx].astype(np.int32)


def tree_sum(terms):
    """blocks of 256 consecutive terms (+0.0 past the end), inside a block  for stride = 128 .. 1: x[i] += x[i + stride],  the block
    sums added in ascending order starting from block 0's"""
    terms = np.asarray(terms, dtype=np.float64)
    nblk = (len(terms) + BLOCK - 1) // BLOCK
    x = np.zeros((nblk, BLOCK), dtype=np.float64)
    x.reshape(-1)[:len(terms)] = terms
    stride = BLOCK // 2
    with np.errstate(all="ignore"):
        while stride >= 1:
            x[:, :stride] = x[:, :stride] + x[:, stride:2 * stride]
            stride //= 2
        acc = x[0, 0]
        for k in range(1, nblk):
            acc = acc + x[k, 0]
    return np.float64(acc)


def side(dist, idx, targets, alpha, n_lambda, non_reg):
    """(L, count, coef) of one side: len(dist) queries into `targets` targets"""
    q = len(dist)
    frac = np.float64(q) / np.float64(targets)
    if non_reg:
        frac = max(frac, np.float64(1.0))
    c = counts(idx, targets)
    with np.errstate(all="ignore"):
        if n_lambda == 1:
            p = c.astype(np.float64)
        elif n_lambda == 0:
            p = np.ones(q, dtype=np.float64)
        else:
            p = np.power(c.astype(np.float64), np.float64(n_lambda))
        W = frac / (p + np.float64(1e-6))
        e = np.exp(-(np.float64(alpha) * np.asarray(dist, dtype=np.float32).astype(np.float64)))
        qq = e * W
        h = (np.float64(0.5) * np.float64(alpha)) / np.float64(q)
        coef = (h * qq).astype(np.float32)
        L = tree_sum(np.float64(1.0) - qq) / np.float64(q)
    return L, c, coef


def dcd(dist1, idx1, dist2, idx2, alpha=1000.0, n_lambda=1.0, non_reg=False):
    """one cloud -> dict(loss, halves (2,), count1, count2, coef1, coef2, status)"""
    n, m = len(dist1), len(dist2)
    i1, i2 = np.asarray(idx1, dtype=np.int64), np.asarray(idx2, dtype=np.int64)
    if ((i1 < 0) | (i1 >= m)).any() or ((i2 < 0) | (i2 >= n)).any():
        nan = np.float64("nan")
        return dict(loss=nan, halves=np.full(2, nan), count1=np.full(n, -1, np.int32), count2=np.full(m, -1, np.int32),
                    coef1=np.full(n, np.nan, np.float32), coef2=np.full(m, np.nan, np.float32), status=REFUSED)
    L1, c1, k1 = side(dist1, i1, m, alpha, n_lambda, non_reg)
    L2, c2, k2 = side(dist2, i2, n, alpha, n_lambda, non_reg)
    with np.errstate(all="ignore"):
        loss = np.float64(0.5) * (L1 + L2)
    return dict(loss=loss, halves=np.array([L1, L2]), count1=c1, count2=c2, coef1=k1, coef2=k2, status=0)


def dcd_batch(dist1, idx1, dist2, idx2, alpha=1000.0, n_lambda=1.0, non_reg=False):
    """(B, ...) arrays -> dict of stacked outputs"""
    each = [dcd(dist1[b], idx1[b], dist2[b], idx2[b], alpha, n_lambda, non_reg) for b in range(len(dist1))]
    return {k: np.stack([np.asarray(r[k]) for r in each]) for k in each[0]}


# ---- hand-made nn_distance results: hostile inputs need no search -------------------------------------------------------------------
KINDS = ("one", "perm", "random", "zero", "far")


def make(kind, n, m, seed):
    """(dist1 (n,), idx1 (n,), dist2 (m,), idx2 (m,)) of one cloud.  one: every query on one target (count = the number of queries);
    perm: a permutation where the sizes allow, else indices modulo the target count; random: indices with repeats; zero: distances
    0; far: distances so large that exp underflows to 0 at every alpha >= 1."""
    rng = np.random.default_rng(seed)

    def half(q, t):
        if kind == "one":
            idx = np.full(q, int(rng.integers(t)))
        elif kind == "perm":
            idx = rng.permutation(max(q, t))[:q] % t
        else:
            idx = rng.integers(0, t, size=q)
        if kind == "zero":
            d = np.zeros(q)
        elif kind == "far":
            d = rng.uniform(800.0, 1e30, size=q)
        else:
            d = rng.uniform(0.0, 1.0, size=q) ** 4 * 0.05              # squared distances of unit-scale clouds, many near 0
        return d.astype(np.float32), idx.astype(np.int32)

    d1, i1 = half(n, m)
    d2, i2 = half(m, n)
    return d1, i1, d2, i2
