"""The deterministic Chamfer backward without a GPU: its numpy restatement (tests/chamfer_grad_ref.py, the bit-exact yardstick of
tests/test_gpu_chamfer_grad_det.py) against the oracle's double-precision gradient at the project's bar for this backward, and the
rows of dispatch::cg_form (csrc/dispatch.h) -- which form serves an output, and where the long-list path takes over."""
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from oracle import structural as S
from tests import chamfer_grad_ref as R

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _case(seed, b, n, m, collapse=None):
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((b, n, 3)).astype(np.float32)
    x2 = rng.standard_normal((b, m, 3)).astype(np.float32)
    if collapse == "target":                   # every point of cloud 2 the same: idx1 == 0 everywhere, one list of length n
        x2[:] = x2[:, :1]
    if collapse == "halves":                   # cloud 1 = its first half twice
        x1[:, n // 2:2 * (n // 2)] = x1[:, :n // 2]
    _, i1, _, i2 = S.nndistance(x1, x2)
    gd1 = rng.standard_normal((b, n)).astype(np.float32)
    gd2 = rng.standard_normal((b, m)).astype(np.float32)
    gd1[:, ::7] = 0
    if collapse == "target":
        # one list of N = n entries: a sequential fp32 sum is off by at most N * 2^-24 * sum|c| from the oracle's double one.  With
        # N <= 300 and |c| = |2 gd dx| of the order 1e-3 (sum|c| < 1) that is < 2e-5 in the worst case, a few 1e-7 typically:
        # inside the bar's absolute term.  (Rows of order 1 would put a cancelling sum of 300 terms outside it by rounding alone.)
        gd1 *= np.float32(1e-3); gd2 *= np.float32(1e-3)
    return x1, x2, i1, i2, gd1, gd2


@pytest.mark.parametrize("b,n,m,collapse", [(1, 1, 1, None), (2, 7, 3, None), (3, 257, 130, None), (2, 130, 515, None),
                                            (2, 300, 64, "target"), (1, 150, 33, "target"), (2, 256, 200, "halves")])
def test_restatement_agrees_with_the_oracle(b, n, m, collapse):
    x1, x2, i1, i2, gd1, gd2 = _case(11 + n, b, n, m, collapse)
    if collapse == "target":
        assert not i1.any()
    g1, g2 = R.nndistancegrad_det(x1, x2, i1, i2, gd1, gd2)
    o1, o2 = S.nndistancegrad(x1, x2, i1, i2, gd1, gd2)
    assert g1.dtype == np.float32 and g2.dtype == np.float32
    np.testing.assert_allclose(g1, o1, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g2, o2, rtol=1e-5, atol=1e-5)


def test_restatement_adds_in_ascending_query_order():
    """three queries at one target whose contributions do not associate: (1 + 2^-24) + 2^-24 rounds to 1 twice, 2^-24 + 2^-24
    first would reach 1 + 2^-23 -- the restatement must give the former"""
    x1 = np.zeros((1, 1, 3), np.float32)
    x2 = np.array([[[-1, 0, 0], [-1, 0, 0], [-1, 0, 0]]], np.float32)
    i1, i2 = np.zeros((1, 1), np.int32), np.zeros((1, 3), np.int32)
    gd1 = np.zeros((1, 1), np.float32)
    gd2 = np.array([[0.5, 2.0 ** -25, 2.0 ** -25]], np.float32)       # contributions 1, 2^-24, 2^-24 on x
    g1, _ = R.nndistancegrad_det(x1, x2, i1, i2, gd1, gd2)
    assert g1[0, 0, 0] == np.float32(1.0)


def test_per_cloud_form_is_the_row_form_with_divided_rows():
    x1, x2, i1, i2, _, _ = _case(5, 3, 100, 60)
    gcd = np.array([1.0, -0.3, 7.25], np.float32)
    a = R.chamfer_cd_backward(x1, x2, i1, i2, gcd)
    gd1 = np.broadcast_to((gcd / np.float32(100))[:, None], (3, 100))
    gd2 = np.broadcast_to((gcd / np.float32(60))[:, None], (3, 60))
    b = R.nndistancegrad_det(x1, x2, i1, i2, gd1, gd2)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


PROBE = r"""
#include <cstdio>
#include "dispatch.h"
int main() {
    int targets, queries, lds;
    while (scanf("%d %d %d", &targets, &queries, &lds) == 3) {
        dispatch::Switches sw;
        sw.cg_lds = lds;
        const dispatch::CGForm f = dispatch::cg_form(targets, queries, sw);
        printf("%s %d\n", f.kernel == dispatch::CGKernel::Lds ? "lds" : "workspace", f.long_list);
    }
    return 0;
}
"""


def test_dispatch_rows(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    (tmp_path / "probe.cpp").write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(tmp_path / "probe.cpp"), "-o", str(exe)], check=True)
    rows = {                                   # (targets, queries, DPF_CG_LDS) -> form, long-list threshold
        (1, 1, -1): "lds 64",
        (2048, 2048, -1): "lds 64",
        (8192, 8192, -1): "lds 64",            # 8192 queries: 32 KB of keys + 96 KB of contributions, the LDS form's limit
        (8192, 8193, -1): "workspace 64",
        (8193, 8192, -1): "lds 64",            # the targets only cost their direct terms ...
        (65536, 8192, -1): "lds 64",
        (65537, 8192, -1): "workspace 64",     # ... up to what one workgroup should serve alone
        (64, 715827882, -1): "workspace 64",
        (2048, 2048, 0): "workspace 64",       # the switch: never the LDS form
        (2048, 2048, 1): "lds 64",
        (8192, 8193, 1): "workspace 64",       # ... which cannot be forced past its limits
    }
    out = subprocess.run([str(exe)], input="".join("%d %d %d\n" % k for k in rows), text=True, capture_output=True,
                         check=True).stdout.splitlines()
    assert dict(zip(rows, out)) == rows
