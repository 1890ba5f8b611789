"""dispatch::chunk_range / dispatch::chunk_grid (csrc/dispatch.h) cut the mesh family's launches to the grid's limits: pure
host code.  As tests/test_point_mesh_dispatch_cpu.py does for the form pickers: a tiny program with its own main() built with
the host compiler alone.  It takes the limits as arguments, so the boundaries are crossed with a handful of items; the
production limits are printed and pinned."""
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
    char kind;
    long a, b, c, d, fail;
    while (scanf(" %c %ld %ld %ld %ld %ld", &kind, &a, &b, &c, &d, &fail) == 6) {
        long calls = 0;
        int e;
        if (kind == 'r')           // r total per - - fail_at: the pieces of [0, total)
            e = dispatch::chunk_range(a, b, [&](long i0, long cnt) { printf("%ld:%ld ", i0, cnt); return ++calls == fail ? 7 : 0; });
        else                       // g slots blocks max_slots max_blocks fail_at
            e = dispatch::chunk_grid((int)a, b, [&](int b0, unsigned nb, long k0, unsigned nk) {
                printf("%d:%u:%ld:%u ", b0, nb, k0, nk);
                return ++calls == fail ? 7 : 0;
            }, (int)c, d);
        printf("-> %d\n", e);
    }
    printf("%ld %d\n", dispatch::MAX_BLOCKS, dispatch::MAX_SLOTS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("chunk_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        """[(pieces as tuples of integers, the returned code)] per query, and the production limits"""
        text = "".join("%s %d %d %d %d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        got = []
        for line in out[:-1]:
            pieces, code = line.split("->")
            got.append(([tuple(int(x) for x in p.split(":")) for p in pieces.split()], int(code)))
        return got, tuple(int(x) for x in out[-1].split())
    return run


def covers(pieces, total, per):
    """contiguous from 0, none empty, none above per, ending at total"""
    at = 0
    for first, count in pieces:
        assert first == at and 1 <= count <= per, (pieces, total, per)
        at += count
    assert at == total, (pieces, total, per)


def test_production_limits(ask):
    _, limits = ask([])
    assert limits == (4194304, 32768)


@pytest.mark.parametrize("per", [1, 2, 5, 256])
def test_range_covers_exactly(ask, per):
    totals = [0, 1, per - 1, per, per + 1, 3 * per + 2]
    got, _ = ask([("r", t, per, 0, 0, 0) for t in totals])
    for t, (pieces, code) in zip(totals, got):
        assert code == 0
        covers(pieces, t, per)
        assert len(pieces) == -(-t // per)


def test_grid_covers_both_axes_slots_outermost(ask):
    sizes = lambda per: [0, 1, per - 1, per, per + 1, 3 * per + 2]          # noqa: E731
    ms, mb = 4, 3
    qs = [("g", s, b, ms, mb, 0) for s in sizes(ms) for b in sizes(mb)]
    got, _ = ask(qs)
    for (_, s, b, _, _, _), (pieces, code) in zip(qs, got):
        assert code == 0
        if s == 0 or b == 0:
            assert pieces == []
            continue
        rows = sorted(set((b0, nb) for b0, nb, _, _ in pieces))
        covers(rows, s, ms)
        for b0, nb in rows:
            covers([(k0, nk) for r0, rn, k0, nk in pieces if (r0, rn) == (b0, nb)], b, mb)
        assert pieces == sorted(pieces) and len(set(pieces)) == len(pieces)      # slots outermost, blocks inside, each piece once
        assert len(pieces) == -(-s // ms) * -(-b // mb)


def test_a_failing_launch_stops_the_loop_and_is_returned(ask):
    got, _ = ask([("r", 10, 3, 0, 0, 2), ("g", 9, 7, 4, 3, 2), ("g", 9, 2, 4, 3, 2), ("r", 10, 3, 0, 0, 9)])
    assert got[0] == ([(0, 3), (3, 3)], 7)
    assert got[1] == ([(0, 4, 0, 3), (0, 4, 3, 3)], 7)                       # the second launch of the first piece of slots
    assert got[2] == ([(0, 4, 0, 2), (4, 4, 0, 2)], 7)                       # the first launch of the second piece of slots
    assert got[3][1] == 0 and len(got[3][0]) == 4                            # a launch that is never reached fails nothing
