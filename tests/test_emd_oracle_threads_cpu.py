"""The approx-EMD oracle run on many cases at once (tests/emd_cases.oracle_emd): one case per host thread gives the same bits as
one thread for all, so what the GPU tests compare with does not depend on the host they run on."""
import numpy as np

from oracle import structural as S
from tests.emd_cases import KINDS, emd_clouds, emd_fuzz_case, oracle_emd, oracle_pair_costs


def test_oracle_bits_do_not_depend_on_the_worker_count():
    """A ragged batch of fuzz cases (n != m both ways, B up to 3): match, cost and both masses with 1 and 4 workers, and against
    S.approxmatch + S.matchcost called directly, bit for bit."""
    rng = np.random.default_rng(7)
    cases = [emd_fuzz_case(rng, max_n=500, max_m=512)[:2] for _ in range(12)]
    one = oracle_emd(cases, workers=1, with_match=True)
    many = oracle_emd(cases, workers=4, with_match=True)
    assert len(one) == len(many) == len(cases)
    for (a, b), r1, r4 in zip(cases, one, many):
        for x1, x4 in zip(r1, r4):
            assert x1.dtype == x4.dtype and np.array_equal(x1, x4, equal_nan=True), (a.shape, b.shape)
        match, _ = S.approxmatch(a, b)
        assert np.array_equal(r1[3], match) and np.array_equal(r1[0], S.matchcost(a, b, match))


def test_oracle_pair_costs_are_the_batched_costs():
    """oracle_pair_costs of single pairs equals the oracle's batched cost of the same pairs, bit for bit."""
    rng = np.random.default_rng(8)
    a, b = emd_clouds(rng, "jitter", 3, 40, 3, 33)
    want = S.matchcost(a, b, S.approxmatch(a, b)[0])
    got = oracle_pair_costs([(a[i], b[i]) for i in range(3)], workers=3)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_emd_clouds_kinds():
    """emd_clouds: every kind gives finite float32 clouds of the asked shapes, for unequal set sizes both ways."""
    rng = np.random.default_rng(9)
    for kind in KINDS:
        for n1, n, n2, m in ((1, 5, 3, 7), (4, 33, 2, 1)):
            a, b = emd_clouds(rng, kind, n1, n, n2, m)
            assert a.shape == (n1, n, 3) and b.shape == (n2, m, 3), kind
            assert a.dtype == b.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(b).all(), kind
