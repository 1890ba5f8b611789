"""Shared pieces of the approx-EMD tests (tests/test_gpu_emd.py, tests/test_gpu_pairwise_emd.py): the seeded cloud generator of
the fuzz, the float64 auction that measures how well conditioned an input is for the fp32 oracle, the conditioning rule built on
it, the CPU oracle run on many cases at once, and the switch of the matrix-core path.  A plain module, not a conftest."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import structural as S

KINDS = ("uniform", "gauss", "jitter", "clustered", "offset", "line", "plane", "dup", "grid")


def emd_clouds(rng, kind, n1, n, n2, m):
    """n1 clouds of n points and n2 clouds of m points of one kind of emd_fuzz_case.  Where the kind ties the second set to the
    first (jitter, dup), cloud j of the second set is drawn from cloud j % n1 of the first.  -> (a (n1, n, 3), b (n2, m, 3))"""
    src = np.arange(n2) % n1
    a = rng.random((n1, n, 3), dtype=np.float32) - 0.5
    b = rng.random((n2, m, 3), dtype=np.float32) - 0.5
    if kind == "gauss":
        a = (0.2 * rng.standard_normal((n1, n, 3))).astype(np.float32)
        b = (0.2 * rng.standard_normal((n2, m, 3))).astype(np.float32)
    elif kind == "clustered":
        a = (a * 0.05 + rng.integers(0, 3, (n1, n, 1)) * 0.3).astype(np.float32)
    elif kind == "line":
        a[:, :, 1:] = 0
        b[:, :, 1:] = 0
    elif kind == "plane":
        a[:, :, 2] = 0
        b[:, :, 2] = 0.01
    elif kind == "jitter":
        b = (a[src][:, rng.integers(0, n, m)] + 0.02 * rng.standard_normal((n2, m, 3))).astype(np.float32)
    elif kind == "dup":
        a = a[:, rng.integers(0, max(1, n // 8), n)]
        b = (a[src][:, rng.integers(0, n, m)] + np.float32(0.001) * (rng.random((n2, m, 3), dtype=np.float32) - 0.5)).astype(np.float32)
    elif kind == "grid":
        a = (rng.integers(-8, 9, (n1, n, 3)) / 16.0).astype(np.float32)
        b = (rng.integers(-8, 9, (n2, m, 3)) / 16.0).astype(np.float32)
    elif kind == "offset":
        a, b = a + 5.0, b + 5.0
    else:
        assert kind == "uniform", kind
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def emd_fuzz_case(rng, max_n=1500, max_m=1024):
    """One case of the approx-EMD fuzz (the generator of tests/diag/emd_matrix_fuzz.py, r05, plus the kinds VERDICT r05 #1 names):
    random ragged shapes, n != m in both directions, and cloud kinds -- uniform, gauss, jitter (a perturbed re-sampling), clustered,
    offset (a far common origin), line (collinear: near-ties are the rule), plane, dup (many exactly repeated points), grid (a
    lattice: exact ties).  -> (a (B, n, 3), b (B, m, 3), kind)"""
    B = int(rng.integers(1, 4))
    n = int(rng.choice([1, 3, 31, 32, 33, 64, 100, 127, 128, 129, 255, 300, 500, 777, 1024, 1500][:16 if max_n >= 1500 else 13]))
    m = int(rng.choice([1, 2, 32, 33, 63, 96, 128, 130, 257, 400, 512, 900, 1024][:13 if max_m >= 1024 else 10]))
    kind = str(rng.choice(list(KINDS)))
    a, b = emd_clouds(rng, kind, B, n, B, m)
    return a, b, kind


def auction64(a1, b1):
    """approxmatch.cu:3-182 + matchcost of ONE cloud pair in float64 (whole passes as matrix expressions;
    tests/test_oracle_golden.py holds the C oracle to this reading): exact arithmetic for practical purposes -- what the fp32
    oracle is compared with to tell how well conditioned an input is.  -> the total cost (not divided by n)"""
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


def assert_cost_in_contract(got, want, a1, b1, tag, div=1.0):
    """One cost `got` against the fp32 oracle's `want` for the pair (a1, b1), both divided by `div`: rtol 1e-4 -- or, by the
    conditioning rule, where the oracle itself is further than 1e-5 from the float64 auction, 1e-4 + 4 x that distance.
    The auction divides by (1e-9 + a sum of weights), and fp32 cannot resolve `remain - consumed` of a size-1 quantity to 1e-9:
    on clouds where some point's neighbours have all been consumed (exact duplicates, near-duplicates) EVERY fp32 evaluation
    returns its own rounding noise amplified -- the fp32 oracle sits up to 4e-4 from the same auction in float64 there and both
    kernel families up to 5e-4 from the oracle (tools/emd_oracle_fuzz.py, profiles/r06_emd_oracle_fuzz_800.txt: 11 of 1 604
    clouds).  A NaN `got` fails.  -> the relative error"""
    got, want = float(got), float(want)
    err = abs(got - want) / max(abs(want), 1e-6)
    if not err <= 1e-4:
        cond = abs(want - auction64(a1, b1) / div) / max(abs(want), 1e-6)
        assert cond > 1e-5 and err <= 1e-4 + 4.0 * cond, (tag, got, want, err, cond)
    return err


def oracle_workers():
    """Host threads for the CPU oracle: the CPUs this process may run on, at most 16 (never os.cpu_count(): a job may be given
    far fewer CPUs than the machine shows)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _oracle_one(case, with_match=False):
    a, b = case
    match, _ = S.approxmatch(a, b)
    out = (S.matchcost(a, b, match), match.sum(1), match.sum(2))
    return out + (match,) if with_match else out


def oracle_emd(cases, workers=None, with_match=False):
    """S.approxmatch + S.matchcost of every case [(a (B, n, 3), b (B, m, 3)), ...], one case per host thread (ctypes releases
    the GIL during the foreign call; each case owns its match and temp, so the bits do not depend on the thread count).
    -> [(cost (B,), column mass match.sum(1) (B, n), row mass match.sum(2) (B, m)[, match (B, m, n)]), ...] in the order of
    `cases`"""
    S.lib()                                                   # (built and loaded once, before the threads)
    cases = [(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)) for a, b in cases]
    with ThreadPoolExecutor(max_workers=workers or oracle_workers()) as ex:
        return list(ex.map(lambda c: _oracle_one(c, with_match), cases))


def oracle_pair_costs(pairs, workers=None):
    """The oracle's total cost (not divided by n) of each cloud pair [(a1 (n, 3), b1 (m, 3)), ...] -> float32 (len(pairs),)"""
    got = oracle_emd([(a1[None], b1[None]) for a1, b1 in pairs], workers)
    return np.array([r[0][0] for r in got], np.float32)


class matrix_path:
    """dpf_emd_set_matrix_path(on) for the duration of a block (restored in finally)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from dpf_nets_amd._lib import lib
        self.prev = lib().dpf_emd_set_matrix_path(1 if self.on else 0)

    def __exit__(self, *exc):
        from dpf_nets_amd._lib import lib
        lib().dpf_emd_set_matrix_path(self.prev)
