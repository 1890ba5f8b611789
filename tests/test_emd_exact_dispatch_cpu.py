"""dispatch::ee_form (csrc/dispatch.h) decides the kernel form, the workgroup size and the LDS per point of dpf_emd_exact: a pure
function of (n, the forced form), total over its domain.  As tests/test_mesh_point_dispatch_cpu.py does for mp_form: a tiny
program with its own main() built with the host compiler alone, each pair of cases at and one past a threshold."""
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
        const dispatch::EEForm f = dispatch::ee_form((int)n, (int)force);
        printf("%s %d %d\n", f.kernel == dispatch::EEKernel::Resident ? "resident" : f.kernel == dispatch::EEKernel::Streamed ? "streamed" : "unserved",
               f.threads, f.lds_per_point);
    }
    printf("%d %d %d %d %d %d\n", dispatch::EE_MAX_POINTS, dispatch::EE_LDS_POINTS, dispatch::EE_MIN_BITS, dispatch::EE_MAX_BITS,
           dispatch::EE_EPS0_SHIFT, dispatch::EE_EPS_SHIFT);
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("ee_dispatch")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)

    def run(queries):
        text = "".join("%d %d\n" % q for q in queries)
        out = subprocess.run([str(d / "probe")], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(queries) + 1
        return out[:-1], tuple(int(x) for x in out[-1].split())
    return run


def test_emd_exact_form_thresholds(ask):
    _, consts = ask([])
    assert consts == (8192, 4096, 1, 24, 4, 3)
    cases = {
        (1, 0): "resident 64 36", (64, 0): "resident 64 36", (65, 0): "resident 256 36", (512, 0): "resident 256 36",
        (513, 0): "resident 1024 36", (2048, 0): "resident 1024 36", (4096, 0): "resident 1024 36",
        (4097, 0): "streamed 1024 16", (8192, 0): "streamed 1024 16", (8193, 0): "unserved 0 0", (0, 0): "unserved 0 0",
        (4096, 1): "resident 1024 36", (4097, 1): "unserved 0 0", (1, 2): "streamed 64 16", (300, 2): "streamed 256 16",
        (8192, 2): "streamed 1024 16", (8193, 2): "unserved 0 0",
    }
    got, _ = ask(list(cases))
    wrong = {q: (g, w) for (q, w), g in zip(cases.items(), got) if g != w}
    assert not wrong, "(got, expected) per query: %s" % wrong


def test_emd_exact_form_is_total_and_fits_the_lds(ask):
    """whatever the arguments, a form; a served one has 1..16 waves and at most 160 KB of LDS less the kernel's static kilobyte"""
    qs = [(n, force) for n in (-5, 0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 2 ** 31 - 1)
          for force in (-1, 0, 1, 2, 3)]
    got, (NMAX, NLDS, _, _, _, _) = ask(qs)
    for (n, force), g in zip(qs, got):
        kind, threads, per = g.split()
        threads, per = int(threads), int(per)
        if kind == "unserved":
            assert n < 1 or n > NMAX or (force == 1 and n > NLDS), (n, force, g)
            continue
        assert 1 <= n <= NMAX and threads in (64, 256, 1024), (n, force, g)
        assert ((n + 7) // 8 * 8) * per <= 160 * 1024 - 1024, (n, force, g)
        assert (kind == "resident") == (per == 36) and (kind == "resident" or per == 16), (n, force, g)
        if force == 1:
            assert kind == "resident", (n, force, g)
        if force == 2:
            assert kind == "streamed", (n, force, g)
