"""dispatch::pm_form (csrc/dispatch.h) decides the kernel form of dpf_point_mesh_distance: a pure function of (B, N, the largest
face count, the forced form), total over its domain.  As tests/test_dispatch_cpu.py does for the other entries: a tiny program
with its own main() built with the host compiler alone, each pair of cases at and one past a threshold."""
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
    long b, n, f, force;
    while (scanf("%ld %ld %ld %ld", &b, &n, &f, &force) == 4) {
        const dispatch::PMForm p = dispatch::pm_form((int)b, (int)n, f, (int)force);
        printf("%s %d\n", p.kernel == dispatch::PMKernel::Whole ? "whole" : "split", p.splits);
    }
    printf("%d %d %d %d\n", dispatch::PM_WG_POINTS, dispatch::PM_TILE, dispatch::PM_FILL_WGS, dispatch::PM_MAX_SPLITS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("pm_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        text = "".join("%d %d %d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        return out[:-1], tuple(int(x) for x in out[-1].split())
    return run


def test_point_mesh_form_thresholds(ask):
    _, (P, T, FILL, CAP) = ask([])
    assert (P, T, FILL, CAP) == (256, 256, 512, 1024)
    cases = {
        (50, 2500, 100000, 0): "split 2",                  # the benchmarked shape: 500 workgroups
        (52, 2500, 100000, 0): "whole 1",                  # 520 workgroups fill the chip
        (51, 2560, 100000, 0): "split 2",                  # 510 do not
        (2, P * FILL // 2, 1, 0): "whole 1",               # exactly FILL workgroups
        (1, P * (FILL - 1), 2 * T, 0): "split 2",          # one fewer, two tiles
        (1, P * (FILL - 1), T, 0): "whole 1",              # one tile: nothing to split
        (1, 1, 3 * T, 0): "split 3", (1, 1, 2 * T + 3, 0): "split 3", (1, P + 1, 100 * T, 0): "split 100",
        (1, P, 100000, 0): "split 391", (1, 2 * P, 100000, 0): "split 256", (1, 1, 10 ** 9, 0): "split 512",
        (4, 2048, 20000, 0): "split 16", (1, 1, 1, 0): "whole 1",
        (1, 1, 3 * T, 1): "whole 1", (50, 2500, 100000, 2): "split 2", (52, 2500, 100000, 2): "split 1", (1, 1, 1, 2): "split 1",
        (1, 1, 2 * T + 3, 2): "split 3", (7, 129, T - 1, 2): "split 1",
    }
    got, _ = ask(list(cases))
    wrong = {q: (g, w) for (q, w), g in zip(cases.items(), got) if g != w}
    assert not wrong, "(got, expected) per query: %s" % wrong


def test_point_mesh_form_is_total(ask):
    """whatever the arguments (empty, negative, past 32 bits of faces, an unknown force), a form with 1..PM_MAX_SPLITS splits"""
    qs = [(b, n, f, force) for b in (-3, 0, 1, 65535, 2 ** 31 - 1) for n in (-1, 0, 1, 255, 257, 2 ** 31 - 1)
          for f in (-5, 0, 1, 255, 257, 2 ** 31 - 1, 2 ** 40) for force in (-1, 0, 1, 2, 3)]
    got, (_, _, _, CAP) = ask(qs)
    for q, g in zip(qs, got):
        kind, splits = g.split()
        assert kind in ("whole", "split") and 1 <= int(splits) <= CAP, (q, g)
        if kind == "whole":
            assert int(splits) == 1, (q, g)
        if q[3] == 1:
            assert kind == "whole", (q, g)
        if q[3] == 2:
            assert kind == "split", (q, g)
