"""tests/swd_ref.py, the numpy restatement of the sliced-Wasserstein contract, against a float64 torch path: float64 projection,
torch.sort(stable=True), and autograd through the gather.  On integer-lattice clouds with dyadic directions every fp32 operation of
the restatement is exact, so the two orders agree exactly and the values to 1e-12."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import swd_ref as R                                                                          # noqa: E402


def f64_path(a, b, dirs):
    """float64 SW2^2 of one pair with autograd: (distance, sorted_a, order_a, sorted_b, order_b, grad_a, grad_b) as numpy"""
    ta = torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    tb = torch.tensor(np.asarray(b, dtype=np.float64), requires_grad=True)
    th = torch.tensor(np.asarray(dirs, dtype=np.float64))
    pa, pb = th @ ta.t(), th @ tb.t()                                                      # (L, n)
    sa, oa = torch.sort(pa, dim=1, stable=True)
    sb, ob = torch.sort(pb, dim=1, stable=True)
    dist = ((sa - sb) ** 2).mean()
    dist.backward()
    return tuple(v.detach().numpy() for v in (dist, sa, oa, sb, ob, ta.grad, tb.grad))


@pytest.mark.parametrize("n,L", [(1, 1), (2, 3), (65, 5), (300, 7)])
def test_lattice_clouds_under_dyadic_directions_agree_with_float64(n, L):
    a, b = R.make_cloud("lattice", n, 3 * n), R.make_cloud("lattice", n, 3 * n + 1)
    dirs = R.make_dirs("dyadic", L, n)
    sa, oa, sta = R.tables(a, dirs)
    sb, ob, stb = R.tables(b, dirs)
    dist, fa, foa, fb, fob, ga, gb = f64_path(a, b, dirs)
    assert sta == 0 and stb == 0
    assert np.array_equal(oa, foa) and np.array_equal(ob, fob)
    assert np.abs(sa.astype(np.float64) - fa).max() <= 1e-12 and np.abs(sb.astype(np.float64) - fb).max() <= 1e-12
    ss = R.sumsq(sa, sb)
    assert abs(ss / (L * n) - dist) <= 1e-12 * max(1.0, abs(dist))
    assert R.distance(ss, L, n) == np.float32(dist)
    ra, rb, bound_a, bound_b = R.grad((sa, oa, sta), (sb, ob, stb), dirs, 1.0)
    for r, g, bound in ((ra, ga, bound_a), (rb, gb, bound_b)):
        # one rounding to fp32 (half an ulp) of a float64 sum that agrees with autograd's to 1e-12 of its terms' magnitudes
        half_ulp = 0.5 * np.spacing(np.abs(g).astype(np.float32)).astype(np.float64)
        assert (np.abs(r.astype(np.float64) - g) <= half_ulp + 1e-12 * (2.0 / (L * n)) * bound).all()


@pytest.mark.parametrize("n,L", [(1, 2), (65, 5), (257, 4)])
def test_gaussian_clouds_agree_with_float64_to_rounding(n, L):
    a, b = R.make_cloud("gauss", n, n), R.make_cloud("gauss", n, n + 1)
    dirs = R.make_dirs("gauss", L, n)
    sa, oa, sta = R.tables(a, dirs)
    sb, ob, stb = R.tables(b, dirs)
    dist, fa, foa, fb, fob, ga, gb = f64_path(a, b, dirs)
    # three products and two sums in fp32: each value within 4 ulp of the largest term; orders may differ only where float64 values
    # lie that close, so the sorted VALUES are compared
    tol = 4 * 2.0 ** -24 * (np.abs(a).max() + np.abs(b).max()) * 3
    assert np.abs(sa - fa).max() <= tol and np.abs(sb - fb).max() <= tol
    assert abs(R.sumsq(sa, sb) / (L * n) - dist) <= 4 * tol * np.sqrt(max(dist, 1e-30)) + tol * tol
    ra, rb, bound_a, bound_b = R.grad((sa, oa, sta), (sb, ob, stb), dirs, 1.0)
    if np.array_equal(oa, foa) and np.array_equal(ob, fob):
        assert np.abs(ra - ga).max() <= 2 * tol * 2.0 / n * 3 + 1e-7 * np.abs(ga).max()
        assert np.abs(rb - gb).max() <= 2 * tol * 2.0 / n * 3 + 1e-7 * np.abs(gb).max()
    assert (bound_a >= 0).all() and (bound_b >= 0).all()


def test_minus_zero_never_appears_in_sorted():
    pts = R.make_cloud("negzero", 200, 5)
    dirs = R.make_dirs("negzero", 9, 5)
    raw = (pts[None, :, 0] * dirs[:, None, 0] + pts[None, :, 1] * dirs[:, None, 1]) + pts[None, :, 2] * dirs[:, None, 2]
    assert np.signbit(raw[raw == 0]).any(), "the case must produce -0 before the final + 0.0f"
    s, o, st = R.tables(pts, dirs)
    assert st == 0
    assert not np.signbit(s[s == 0]).any()
    assert not (s.view(np.uint32) == 0x80000000).any()


def test_ties_resolve_to_the_lowest_index():
    pts = R.make_cloud("lattice", 500, 11)
    dirs = R.make_dirs("axis", 6)
    s, o, st = R.tables(pts, dirs)
    assert st == 0
    for l in range(6):
        assert sorted(o[l].tolist()) == list(range(500))
        runs = np.flatnonzero(np.diff(s[l]) != 0) + 1
        for seg in np.split(o[l], runs):
            assert (np.diff(seg) > 0).all()                                                # one value: ascending index
        assert len(runs) <= 8                                                              # nine lattice values: whole runs of ties
    same = R.make_cloud("same", 40, 2)
    s, o, st = R.tables(same, R.make_dirs("gauss", 3))
    assert (o == np.arange(40)[None]).all() and (s == s[:, :1]).all()


def test_refusals():
    dirs = R.make_dirs("gauss", 4)
    good = R.make_cloud("gauss", 30, 1)
    for bad_value in (np.nan, np.inf, -np.inf):
        c = good.copy()
        c[17, 1] = bad_value
        s, o, st = R.tables(c, dirs)
        assert st == R.REFUSED and np.isnan(s).all() and (o == -1).all()
    big = good.copy()
    big[3] = np.float32(3e38)                                                               # finite, but the projection overflows
    d2 = dirs.copy()
    d2[2] = (1.0, 1.0, 1.0)
    assert R.tables(big, d2)[2] == R.REFUSED
    d3 = dirs.copy()
    d3[1, 0] = np.nan
    assert R.tables(good, d3)[2] == R.REFUSED
    assert R.tables(good, dirs)[2] == 0
    assert np.isnan(R.sumsq(good[None], good[None], refused=True))


def test_one_direction_on_a_lattice_is_the_mean_squared_difference_of_the_sorted_coordinates():
    n = 333
    a, b = R.make_cloud("lattice", n, 20), R.make_cloud("lattice", n, 21)
    dirs = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)
    ss = R.sumsq(R.tables(a, dirs)[0], R.tables(b, dirs)[0])
    want = int(((np.sort(a[:, 0].astype(np.int64)) - np.sort(b[:, 0].astype(np.int64))) ** 2).sum())
    assert ss == want and float(ss).is_integer()
