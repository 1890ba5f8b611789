"""dispatch::swd_form (csrc/dispatch.h) decides the kernel form, the workgroup size and the keys per thread of dpf_swd_tables: a pure
function of (n, the forced form), total over its domain.  As tests/test_fps_dispatch_cpu.py does for fps_form: a tiny program with
its own main() built with the host compiler alone; every n in 1..max under every force, and each threshold at and one past it."""
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
    long n, force;
    while (scanf("%ld %ld", &n, &force) == 2) {
        const dispatch::SWDForm f = dispatch::swd_form((int)n, (int)force);
        printf("%s %d %d\n", f.kernel == dispatch::SWDKernel::Wave ? "wave" : f.kernel == dispatch::SWDKernel::Quad ? "quad" :
               f.kernel == dispatch::SWDKernel::Full ? "full" : "unserved",
               f.threads, f.kpt);
    }
    printf("%d %d %d %d\n", dispatch::SWD_MAX_POINTS, dispatch::SWD_WAVE_MAX, dispatch::SWD_QUAD_MAX, dispatch::SWD_QUAD_UPTO);
    return 0;
}
"""

FORCES = (-1, 0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("swd_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        text = "".join("%d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        return out[:-1], tuple(int(x) for x in out[-1].split())
    return run


def test_swd_form_thresholds(ask):
    """one wave wherever it serves (512 points), four waves up to SWD_QUAD_UPTO, sixteen above"""
    _, (nmax, wave_max, quad_max, quad_upto) = ask([])
    assert (nmax, wave_max, quad_max) == (8192, 512, 8192)
    assert wave_max <= quad_upto <= quad_max and quad_upto & (quad_upto - 1) == 0
    cases = {
        (0, 0): "unserved 0 0", (1, 0): "wave 64 1", (64, 0): "wave 64 1", (65, 0): "wave 64 2", (128, 0): "wave 64 2",
        (129, 0): "wave 64 4", (256, 0): "wave 64 4", (257, 0): "wave 64 8", (512, 0): "wave 64 8", (8193, 0): "unserved 0 0",
        (512, 1): "wave 64 8", (513, 1): "unserved 0 0",
        (1, 2): "quad 256 1", (256, 2): "quad 256 1", (257, 2): "quad 256 2", (4097, 2): "quad 256 32", (8192, 2): "quad 256 32",
        (8193, 2): "unserved 0 0",
        (1, 3): "full 1024 1", (1024, 3): "full 1024 1", (1025, 3): "full 1024 2", (2500, 3): "full 1024 4", (8192, 3): "full 1024 8",
        (8193, 3): "unserved 0 0", (100, 4): "unserved 0 0", (100, -1): "unserved 0 0", (0, 1): "unserved 0 0",
    }
    for at in (wave_max, quad_upto):                        # each by-size threshold at it and one past it
        for n in (at, at + 1):
            if n > nmax:
                cases[(n, 0)] = "unserved 0 0"
                continue
            kind, threads = ("wave", 64) if n <= wave_max else ("quad", 256) if n <= quad_upto else ("full", 1024)
            kpt = 1
            while threads * kpt < n:
                kpt *= 2
            cases[(n, 0)] = "%s %d %d" % (kind, threads, kpt)
    got, _ = ask(list(cases))
    wrong = {q: (g, w) for (q, w), g in zip(cases.items(), got) if g != w}
    assert not wrong, "(got, expected) per query: %s" % wrong


def test_swd_form_is_total_and_every_served_form_holds_the_cloud(ask):
    """every n in 1..max and a margin either side, every force: a form; Unserved exactly outside the limits; a served form's
    threads * kpt hold the cloud with the LOWEST power of two, and the by-size pick is the forced form it names"""
    NMAX = 8192
    ns = list(range(-2, NMAX + 3)) + [2 ** 31 - 1]
    qs = [(n, force) for n in ns for force in FORCES]
    got, (nmax, wave_max, quad_max, quad_upto) = ask(qs)
    assert nmax == NMAX
    table = dict(zip(qs, got))
    kinds = {1: ("wave", 64, wave_max), 2: ("quad", 256, quad_max), 3: ("full", 1024, nmax)}
    for (n, force), g in table.items():
        kind, threads, kpt = g.split()
        threads, kpt = int(threads), int(kpt)
        limit = nmax if force == 0 else kinds[force][2] if force in kinds else 0
        if kind == "unserved":
            assert n < 1 or n > limit, (n, force, g)
            assert (threads, kpt) == (0, 0)
            continue
        assert 1 <= n <= limit, (n, force, g)
        named = force if force else 1 if n <= wave_max else 2 if n <= quad_upto else 3
        assert (kind, threads) == kinds[named][:2], (n, force, g)
        assert kpt in (1, 2, 4, 8, 16, 32) and threads * kpt >= n and (kpt == 1 or threads * kpt // 2 < n), (n, force, g)
        assert threads * kpt <= max(kinds[named][2], threads), (n, force, g)                 # (an instantiation the launcher has)
        if force == 0:
            assert g == table[(n, named)], (n, g)
