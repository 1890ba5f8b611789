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
