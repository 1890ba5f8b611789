"""dispatch::knn_form (csrc/dispatch.h) decides the list capacity dpf_knn's kernel is instantiated for: a pure function of (k, the
forced form), total over its domain.  As tests/test_fps_dispatch_cpu.py does for fps_form: a tiny program with its own main() built
with the host compiler alone; every k under every force, and each capacity boundary at and one past it."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

PROBE = r"""
#include <cstdio>
#include "dispatch.h"
int main() {
    long k, force;
    while (scanf("%ld %ld", &k, &force) == 2) printf("%d\n", dispatch::knn_form((int)k, (int)force).kcap);
    printf("%d %d %d %d\n", dispatch::KNN_MAX_K, dispatch::KNN_WG_QUERIES, dispatch::KNN_TILE, dispatch::KNN_QUEUE);
    return 0;
}
"""

FORCES = (-1, 0, 1, 2, 3, 4, 5)
CAPS = {1: 4, 2: 8, 3: 16, 4: 32}


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("knn_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        text = "".join("%d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        return [int(x) for x in out[:-1]], tuple(int(x) for x in out[-1].split())
    return run


def test_knn_form_at_every_capacity_boundary(ask):
    """by k the smallest capacity that holds k; a forced capacity serves k up to itself; 0 = Unserved"""
    _, consts = ask([])
    assert consts == (32, 256, 256, 16)
    cases = {
        (1, 0): 4, (4, 0): 4, (5, 0): 8, (8, 0): 8, (9, 0): 16, (16, 0): 16, (17, 0): 32, (32, 0): 32, (33, 0): 0, (0, 0): 0, (-3, 0): 0,
        (4, 1): 4, (5, 1): 0, (1, 2): 8, (8, 2): 8, (9, 2): 0, (1, 3): 16, (16, 3): 16, (17, 3): 0, (1, 4): 32, (17, 4): 32, (32, 4): 32,
        (33, 4): 0, (33, 1): 0, (1, 5): 0, (1, -1): 0, (32, 5): 0,
    }
    got, _ = ask(list(cases))
    wrong = {q: (g, w) for (q, w), g in zip(cases.items(), got) if g != w}
    assert not wrong, "(got, expected) per query: %s" % wrong


def test_knn_form_is_total_and_a_served_capacity_holds_k(ask):
    qs = [(k, force) for k in list(range(-2, 40)) + [2 ** 31 - 1] for force in FORCES]
    got, (kmax, _, _, _) = ask(qs)
    table = dict(zip(qs, got))
    for (k, force), cap in table.items():
        served = 1 <= k <= kmax and (force == 0 or (force in CAPS and CAPS[force] >= k))
        if not served:
            assert cap == 0, (k, force, cap)
            continue
        assert cap in CAPS.values() and cap >= k, (k, force, cap)
        if force:
            assert cap == CAPS[force], (k, force, cap)
        else:
            assert cap == 4 or cap // 2 < k, (k, cap)                                       # the smallest
            assert cap == table[(k, {v: f for f, v in CAPS.items()}[cap])]                  # the pick is the forced form it names
