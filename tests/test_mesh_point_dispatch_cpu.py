"""dispatch::mp_form (csrc/dispatch.h) decides the kernel form of dpf_mesh_point_distance: a pure function of (B, N, the largest
face count, the forced form), total over its domain.  As tests/test_point_mesh_dispatch_cpu.py does for pm_form: a tiny program
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
        const dispatch::PMForm p = dispatch::mp_form((int)b, (int)n, f, (int)force);
        printf("%s %d\n", p.kernel == dispatch::PMKernel::Whole ? "whole" : "split", p.splits);
    }
    printf("%d %d %d %d\n", dispatch::MP_WG_FACES, dispatch::MP_TILE, dispatch::PM_FILL_WGS, dispatch::MP_MAX_SPLITS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("mp_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        text = "".join("%d %d %d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        return out[:-1], tuple(int(x) for x in out[-1].split())
    return run


def test_mesh_point_form_thresholds(ask):
    """(B, N, max_faces, force): workgroups = B * ceil(max_faces / 256), point tiles = ceil(N / 256)"""
    _, (P, T, FILL, CAP) = ask([])
    assert (P, T, FILL, CAP) == (256, 256, 512, 1024)
    cases = {
        (50, 2500, 20000, 0): "whole 1",                   # the benchmarked shape: 50 * 79 workgroups
        (50, 2500, 2500, 0): "split 2",                    # 500 workgroups, ten point tiles
        (52, 2500, 2500, 0): "whole 1",                    # 520 workgroups fill the chip
        (51, 2500, 2560, 0): "split 2",                    # 510 do not
        (2, 1, P * FILL // 2, 0): "whole 1",               # exactly FILL workgroups
        (1, 2 * T, P * (FILL - 1), 0): "split 2",          # one fewer, two point tiles
        (1, T, P * (FILL - 1), 0): "whole 1",              # one point tile: nothing to split
        (1, 3 * T, 1, 0): "split 3", (1, 2 * T + 1, 1, 0): "split 3", (1, 100 * T, P + 1, 0): "split 100",
        (1, 100000, P, 0): "split 391", (1, 100000, 2 * P, 0): "split 256", (1, 10 ** 9, 1, 0): "split 512",
        (4, 20000, 2048, 0): "split 16", (1, 1, 1, 0): "whole 1", (1, 513, 515, 0): "split 3", (1, 257, 7, 0): "split 2",
        (1, 3 * T, 1, 1): "whole 1", (50, 2500, 2500, 2): "split 2", (52, 2500, 2500, 2): "split 1", (1, 1, 1, 2): "split 1",
        (1, 2 * T + 3, 1, 2): "split 3", (7, T - 1, 129, 2): "split 1", (1, 0, 12, 2): "split 1",
    }
    got, _ = ask(list(cases))
    wrong = {q: (g, w) for (q, w), g in zip(cases.items(), got) if g != w}
    assert not wrong, "(got, expected) per query: %s" % wrong


def test_mesh_point_form_is_total(ask):
    """whatever the arguments (empty, negative, past 32 bits of faces, an unknown force), a form with 1..MP_MAX_SPLITS splits"""
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
