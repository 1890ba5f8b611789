"""The oracle of the exact-EMD tests (tests/emd_exact_ref.py) against independent solvers, without a GPU: brute force over all
permutations for n <= 7, scipy's linear_sum_assignment on the same integer matrices up to n = 256, and the measurement of K --
how far, in grid steps per point, the Euclidean cost of the grid's optimum sits above the float64 optimum.

K_MEASURED (printed by test_grid_optimum_is_within_K_steps_of_the_float64_optimum, worst over the GPU test's case list at
n <= 256, three seeds each): 0.0220, on a collinear case at n = 256.  A priori K <= 1 (each c_ij is within half a step of d_ij * s, so the grid's
optimum loses at most n/2 steps on its own assignment and n/2 on the true one) plus the fp32 rounding of the distances, <= 2^-4
of a step for clouds whose extent is their scale; the GPU test's cap is 1.25 and is not derived from this measurement."""
import itertools

import numpy as np
import pytest

import emd_exact_ref as R

K_CAP = 1.25
SIZES = (1, 2, 63, 64, 65, 256)


def _small_cases():
    rng = np.random.RandomState(5)
    for n in range(1, 8):
        yield "random", rng.randn(n, 3).astype(np.float32), rng.randn(n, 3).astype(np.float32)
        a = rng.randint(0, 3, (n, 3)).astype(np.float32)                      # a coarse lattice: many equal costs
        yield "tied", a, rng.randint(0, 3, (n, 3)).astype(np.float32)
        b = rng.randn(n, 3).astype(np.float32)
        b[n // 2:] = b[0]
        yield "duplicate", a[rng.randint(0, n, n)], b


def test_oracle_equals_brute_force_up_to_seven_points():
    for kind, a, b in _small_cases():
        n = a.shape[0]
        o = R.solve(a, b)
        assert o["status"] >= 0, (kind, n)
        c = o["c"]
        best = min(int(c[np.arange(n), list(p)].sum()) for p in itertools.permutations(range(n)))
        assert sorted(o["assignment"].tolist()) == list(range(n)), (kind, n)
        assert o["qcost"] == best, (kind, n, o["qcost"], best)


def test_oracle_equals_scipy_on_the_integer_matrices():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for kind in R.KINDS:
        for n in SIZES:
            for seed in range(3):
                a, b, _ = R.make_case(kind, n, 100 * n + seed)
                o = R.solve(a, b)
                assert o["status"] >= 0 and sorted(o["assignment"].tolist()) == list(range(n)), (kind, n, seed)
                rows, cols = lsa(o["c"])
                assert o["qcost"] == int(o["c"][rows, cols].sum()), (kind, n, seed)


def test_grid_optimum_is_within_K_steps_of_the_float64_optimum():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    worst = (0.0, ())
    for kind in R.KINDS:
        for n in SIZES:
            for seed in range(3):
                a, b, _ = R.make_case(kind, n, 100 * n + seed)
                o = R.solve(a, b)
                if o["s"] == 0:
                    assert o["cost"] == 0
                    continue
                d64 = np.sqrt(((a.astype(np.float64)[:, None] - b.astype(np.float64)[None]) ** 2).sum(-1))
                rows, cols = lsa(d64)
                k = (R.cost64(a, b, o["assignment"]) - d64[rows, cols].sum()) * float(o["s"]) / n
                worst = max(worst, (k, (kind, n, seed)))
    print("K_MEASURED = %.4f at %s" % worst)
    assert worst[0] <= K_CAP, worst


def test_refusals_zero_extent_and_the_round_cap():
    a, b, _ = R.make_case("gauss", 8, 1)
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[3, 1] = bad
        assert R.solve(x, b)["status"] == R.STATUS_REFUSED and R.solve(b, x)["status"] == R.STATUS_REFUSED
    big = a.copy()
    big[0, 0], big[1, 0] = 3e38, -3e38                                       # hi - lo overflows
    assert R.solve(big, b)["status"] == R.STATUS_REFUSED
    big[0, 0], big[1, 0] = 1e20, -1e20                                       # E finite, E * E not
    assert R.solve(big, b)["status"] == R.STATUS_REFUSED
    tiny = (a * np.float32(1e-30)).astype(np.float32)                        # E * E underflows
    assert R.solve(tiny, (b * np.float32(1e-30)).astype(np.float32))["status"] == R.STATUS_REFUSED
    same = np.repeat(a[:1], 8, 0)
    o = R.solve(same, same.copy())
    assert o["status"] == 0 and o["qcost"] == 0 and o["cost"] == 0 and o["assignment"].tolist() == list(range(8))
    o = R.solve(*R.make_case("gauss", 64, 2)[:2], max_rounds=1)
    assert o["status"] == R.STATUS_CAP and o["qcost"] == -1 and np.isnan(o["cost"]) and (o["assignment"] == -1).all()


def test_power_of_two_scaling_leaves_the_grid_alone():
    a, b, _ = R.make_case("gauss", 65, 3)
    _, c, s = R.cost_matrix(a, b)
    for k in (10, -10):
        f = np.float32(2.0 ** k)
        _, ck, sk = R.cost_matrix(a * f, b * f)
        assert (ck == c).all() and sk * f == s


# ---- the cases of tests/test_gpu_emd_exact_edges.py ---------------------------------------------------------------------------
EDGE_SIZES = (127, 128, 129, 191, 257, 512, 513)
GAUSS_65_SUMS = (20.422029214911163, 31.698254324379377)         # make_case("gauss", 65, 6500) before the edge kinds were added


def _against_scipy(lsa, a, b, tag, bits=R.BITS):
    o = R.solve(a, b, bits=bits)
    n = a.shape[0]
    assert o["status"] >= 0 and sorted(o["assignment"].tolist()) == list(range(n)), tag
    rows, cols = lsa(o["c"])
    assert o["qcost"] == int(o["c"][rows, cols].sum()), tag
    return o


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_oracle_equals_scipy_at_the_ragged_sizes(n):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for kind in ("gauss", "lattice", "collapsed", "jitter"):
        for seed in range(1 if (kind, n >= 512) == ("collapsed", True) else 2):          # (collapsed: 2 s a pair from 512 on)
            _against_scipy(lsa, *R.make_case(kind, n, 100 * n + seed)[:2], (kind, n, seed))


@pytest.mark.parametrize("bits", (1, 2, 24))
def test_oracle_equals_scipy_on_other_grids(bits):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for kind in ("gauss", "lattice", "collapsed"):
        for n in (2, 3, 65, 257):
            for seed in range(2):
                a, b, _ = R.make_case(kind, n, 100 * n + seed)
                o = _against_scipy(lsa, a, b, (bits, kind, n, seed), bits)
                assert o["c"].max() <= (2 if bits == 1 else (1 << bits) - 1)
                assert float(o["s"]) * 2.0 ** (R.BITS - bits) == float(R.grid_scale(a, b)[1])


def test_one_bit_grid_reaches_a_cost_of_two():
    """c_ij < 2^bits holds from 2 bits on; at 1 bit a diagonal of the extent's box rounds up to 2 (include/dpf_hip.h)"""
    a = np.zeros((2, 3), np.float32)
    b = np.full((2, 3), 0.9, np.float32)                             # E = 0.9, s = 1, d = 0.9 sqrt(3) = 1.559
    assert R.cost_matrix(a, b, 1)[1].max() == 2 and R.cost_matrix(a, b, 2)[1].max() == 3
    assert R.cost_matrix(*R.make_case("lattice", 65, 6500)[:2], 1)[1].max() == 2        # (a case of the GPU test)


def test_jitter_needs_evictions_and_more_rounds_than_the_permutation():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for n in (129, 513, 1025):
        a, b, perm = R.make_case("jitter", n, 100 * n)
        assert perm.shape == (n,) and a.dtype == b.dtype == np.float32
        o = _against_scipy(lsa, a, b, ("jitter", n)) if n <= 513 else R.solve(a, b)
        p = R.solve(*R.make_case("perm", n, 100 * n)[:2])
        assert o["bids"] > n and o["rounds"] > p["rounds"], (n, o["rounds"], o["bids"], p["rounds"])


def test_existing_kinds_are_unchanged_by_the_new_ones():
    """make_case draws `a` first for every kind: the seeds of the first suite give what they gave (two recorded sums)"""
    a, b, _ = R.make_case("gauss", 65, 6500)
    assert (float(a.astype(np.float64).sum()), float(b.astype(np.float64).sum())) == GAUSS_65_SUMS


@pytest.mark.parametrize("n", (2, 70, 300))
def test_point_kinds_are_the_identity_at_no_cost(n):
    for kind in ("point", "point_signed"):
        a, b, _ = R.make_case(kind, n, 100 * n)
        assert (a == a[0]).all() and (b == a[0]).all()
        if kind == "point_signed":
            assert np.signbit(a[:, 1]).any() and not np.signbit(a[:, 1]).all() and np.signbit(b[:, 1]).any()
        o = R.solve(a, b)
        assert o["status"] == 0 and o["s"] == 0 and o["qcost"] == 0 and o["rounds"] == 0
        assert o["assignment"].tolist() == list(range(n))
        assert o["cost"] == 0 and not np.signbit(o["cost"])
        assert R.solve(a, b, max_rounds=0)["status"] == 0


def test_scaling_edges_solve_and_their_neighbours_refuse():
    for seed in range(3):
        a, b, _ = R.make_case("gauss", 65, 6500 + seed)
        lo, hi = R.scaling_edges(a, b)
        base = R.solve(a, b)
        for e, served in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
            f = np.ldexp(np.float32(1), e)
            with np.errstate(over="ignore"):
                x, y = (a * f).astype(np.float32), (b * f).astype(np.float32)
            o = R.solve(x, y)
            assert (o["status"] > 0) == served and (served or o["status"] == R.STATUS_REFUSED), (seed, e)
            if served:
                rows, cols = pytest.importorskip("scipy.optimize").linear_sum_assignment(o["c"])
                assert o["qcost"] == int(o["c"][rows, cols].sum()), (seed, e)
        # the upper edge is the unscaled grid; at the lower one the squares are subnormal and the grid is another
        f = np.ldexp(np.float32(1), hi)
        assert (R.cost_matrix((a * f).astype(np.float32), (b * f).astype(np.float32))[1] == base["c"]).all()
        f = np.ldexp(np.float32(1), lo)
        low = R.cost_matrix((a * f).astype(np.float32), (b * f).astype(np.float32))[1]
        print("seed", seed, "edges", lo, hi, "entries of c that differ at the lower edge:", int((low != base["c"]).sum()))
        assert (low != base["c"]).any()
