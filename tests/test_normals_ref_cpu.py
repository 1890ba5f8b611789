"""The numpy restatement of dpf_normals (tests/normals_ref.py) against numpy.linalg.eigh on its own covariance: what keeps the bounds
of tests/test_gpu_normals.py honest.  The restatement must hold the four bounds BY ITSELF -- each 64 eps = 2^-46, at least 6 x the
worst value measured over 160 000 neighbourhoods per k -- on the eight kinds of neighbourhood at k in {3, 4, 8, 16, 32}:

    1. |C v - lambda_0 v| <= 2^-46 lambda_max           2. | |v| - 1 | <= 2^-46
    3. every eigenvalue within 2^-46 lambda_max of eigh's
    4. where lambda_1 - lambda_0 > 2^-20 lambda_max:  |v x u_0| (lambda_1 - lambda_0) / lambda_max <= 2^-46, u_0 eigh's vector (the
       angle by the cross product: sqrt(1 - dot^2) bottoms out at 1.5e-8 on its own rounding)

Also here: the build's no-scratch check of normals.o, the sign rule on hand-made vectors, the flags, and the Python surface's
argument checks that need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import normals_ref as R                                                                      # noqa: E402

BOUND = 2.0 ** -46
EPS = 2.0 ** -52
KS = (3, 4, 8, 16, 32)
COUNT = 1500


@pytest.mark.parametrize("k", KS)
def test_the_restatement_holds_the_four_bounds_against_eigh(k):
    for kind in R.KINDS:
        pts = R.neighbourhoods(kind, COUNT, k, 1000 * k + R.KINDS.index(kind))
        _, cov = R.covariance(pts)
        vec, lam = R.eigen(cov)
        res, norm, ev, angle, measured = R.measures(cov, vec, lam)
        print("k %2d %-9s residual %6.2f eps, | |v| - 1 | %5.2f eps, eigenvalues %6.2f eps, angle %6.2f eps on %d of %d"
              % (k, kind, res / EPS, norm / EPS, ev / EPS, angle / EPS, measured, COUNT))
        assert np.isfinite(vec).all() and np.isfinite(lam).all(), kind
        assert (np.diff(lam, axis=1) >= 0).all(), kind
        assert res <= BOUND and norm <= BOUND and ev <= BOUND and angle <= BOUND, (kind, res, norm, ev, angle)
        assert (R.canonical_flip(vec) == 0).all(), kind
        if kind in ("gauss", "squashed", "offset", "scaled") and k > 3:
            assert measured == COUNT, kind                                                  # (the angle bound is not vacuous there)


@pytest.mark.parametrize("k", KS)
def test_the_restatement_holds_the_four_bounds_at_small_scales(k):
    """gauss x 2^-70 (covariances near 2^-140) and gauss x 2^-135, whose fp32 coordinates are themselves subnormal (covariances near
    2^-270): float64 is nowhere near its own underflow at 2^-1022, and numpy.linalg.eigh keeps its accuracy there -- measured, the
    figures equal those of the same covariances multiplied by 2^140 and 2^270 -- so the bounds are held against eigh of the
    covariance as it is, and against the scaled one as well."""
    for kind in R.SMALL_KINDS:
        pts = R.neighbourhoods(kind, COUNT, k, 1000 * k + 50 + R.SMALL_KINDS.index(kind))
        if kind == "denormal":
            assert ((np.abs(pts) < 2.0 ** -126) & (pts != 0)).mean() > 0.99                  # subnormal, and not flushed away
        _, cov = R.covariance(pts)
        vec, lam = R.eigen(cov)
        assert np.isfinite(vec).all() and np.isfinite(lam).all() and (np.diff(lam, axis=1) >= 0).all(), kind
        assert 0 < np.abs(cov).max() < 2.0 ** (-130 if kind == "tiny" else -255)
        up = 2.0 ** (140 if kind == "tiny" else 270)
        for what, scale in (("as it is", 1.0), ("scaled up", up)):
            res, norm, ev, angle, measured = R.measures(cov * scale, vec, lam * scale)
            print("k %2d %-8s %-9s residual %6.2f eps, | |v| - 1 | %5.2f eps, eigenvalues %6.2f eps, angle %6.2f eps on %d of %d"
                  % (k, kind, what, res / EPS, norm / EPS, ev / EPS, angle / EPS, measured, COUNT))
            assert res <= BOUND and norm <= BOUND and ev <= BOUND and angle <= BOUND, (kind, what, res, norm, ev, angle)
            assert k == 3 or measured == COUNT, kind
        assert (R.canonical_flip(vec) == 0).all(), kind
        gauss = R.neighbourhoods("gauss", COUNT, k, 1000 * k + 50 + R.SMALL_KINDS.index(kind))
        if kind == "tiny":                                                                  # an exact power of two: the unit-scale cloud's digits
            assert np.array_equal(pts.astype(np.float64) * 2.0 ** 70, gauss.astype(np.float64))


def test_a_viewpoint_per_row():
    n = np.array([[0.0, 0.0, 1.0]] * 4)
    c = np.array([[1.0, 2.0, 0.5]] * 4)
    w = np.array([[0, 0, 3], [0, 0, -3], [np.nan, 0, -3], [7, -9, 0.5]], dtype=np.float32)
    assert R.orient(n, c, w)[:, 2].tolist() == [1.0, -1.0, 1.0, 1.0]
    for row in range(4):
        assert np.array_equal(R.orient(n, c, w)[row], R.orient(n[row:row + 1], c[row:row + 1], w[row])[0])


def test_three_sweeps_are_not_enough_and_four_equal_six():
    """the sweep count's margin: 3 sweeps leave a residual far above the bound somewhere, 4 give what 6 give"""
    worst3 = 0.0
    for kind in R.KINDS:
        pts = R.neighbourhoods(kind, COUNT, 8, 77 + R.KINDS.index(kind))
        _, cov = R.covariance(pts)
        out = {}
        for sweeps in (3, 4, 6):
            vec, lam = R.eigen(cov, sweeps)
            out[sweeps] = R.measures(cov, vec, lam)[:4]
        worst3 = max(worst3, out[3][0])
        assert max(out[4]) <= BOUND and max(out[6]) <= BOUND, (kind, out)
    print("3 sweeps: worst residual %.3g eps" % (worst3 / EPS))
    assert worst3 > 1000 * BOUND


def test_the_covariance_is_the_two_pass_sum_in_the_stated_order():
    """against an explicit scalar loop, bit for bit; and the offset cloud keeps its digits (the one-pass form would not)"""
    pts = R.neighbourhoods("offset", 40, 5, 3)
    centroid, cov = R.covariance(pts)
    for i in range(pts.shape[0]):
        p = pts[i].astype(np.float64)
        c = [((((p[0, a] + p[1, a]) + p[2, a]) + p[3, a]) + p[4, a]) / 5.0 for a in range(3)]
        assert centroid[i].tolist() == c
        for (a, b), slot in R.SLOT.items():
            acc = (p[0, a] - c[a]) * (p[0, b] - c[b])
            for s in range(1, 5):
                acc = acc + (p[s, a] - c[a]) * (p[s, b] - c[b])
            assert cov[i, slot] == acc
    exact = np.array([np.cov(p.astype(np.float64).T, bias=True) * 5 for p in pts])            # (numpy centres too: a float64 yardstick)
    assert np.abs(R.full(cov) - exact).max() <= 1e-12 * np.abs(exact).max()


def test_exact_neighbourhoods():
    rng = np.random.default_rng(4)
    for axis in range(3):                                                                   # a plane at 0.5 along one axis: exactly +e_axis, lambda_0 == 0
        pts = rng.standard_normal((50, 8, 3)).astype(np.float32)
        pts[:, :, axis] = 0.5
        _, cov = R.covariance(pts)
        vec, lam = R.eigen(cov)
        want = np.zeros(3)
        want[axis] = 1.0
        assert (vec == want).all() and (lam[:, 0] == 0.0).all() and (lam[:, 1] > 0).all(), axis
        assert (R.surface_variation(lam) == 0.0).all()
    pts = R.neighbourhoods("equal", 20, 7, 5)                                               # all neighbours at one point
    _, cov = R.covariance(pts)
    vec, lam = R.eigen(cov)
    assert (cov == 0.0).all() and (lam == 0.0).all() and (vec == np.array([1.0, 0.0, 0.0])).all()
    assert (R.surface_variation(lam) == 0.0).all()
    pts = R.neighbourhoods("gauss", 500, 3, 6)                                              # three points: rank 2
    _, cov = R.covariance(pts)
    vec, lam = R.eigen(cov)
    assert (np.abs(lam[:, 0]) <= BOUND * lam[:, 2]).all()


def test_the_stable_order_puts_the_lower_column_first_among_equals():
    lam = np.array([[2.0, 1.0, 1.0], [1.0, 1.0, 1.0], [3.0, 2.0, 1.0], [1.0, 2.0, 1.0], [2.0, 2.0, 1.0]])
    v = np.tile(np.arange(3.0)[None, None, :], (5, 3, 1))                                    # column c holds the value c
    out, cols = R.sort3(lam, v)
    assert out.tolist() == [[1, 1, 2], [1, 1, 1], [1, 2, 3], [1, 1, 2], [1, 2, 2]]
    assert cols[:, 0, :].tolist() == [[1, 2, 0], [0, 1, 2], [2, 1, 0], [0, 2, 1], [2, 0, 1]]


def test_the_sign_rule_on_hand_made_vectors():
    vec = np.array([[0.6, -0.8, 0.0], [-0.6, 0.8, 0.0], [-1.0, 0.0, 0.0], [0.5, 0.5, -0.5], [-0.5, 0.5, 0.5], [0.5, -0.5, 0.5],
                    [0.0, -0.7, 0.7], [0.0, 0.7, -0.7], [0.1, -0.2, -0.2], [-0.0, 0.0, -1.0]])
    want = np.array([[-0.6, 0.8, 0.0], [-0.6, 0.8, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, -0.5], [0.5, -0.5, -0.5], [0.5, -0.5, 0.5],
                     [0.0, 0.7, -0.7], [0.0, 0.7, -0.7], [-0.1, 0.2, 0.2], [0.0, 0.0, 1.0]])
    assert np.array_equal(R.canonical(vec), want)
    # orientation against the centroid: t < 0 flips, t == 0 and a non-finite viewpoint keep the canonical sign
    n = np.array([[0.0, 0.0, 1.0]] * 5)
    c = np.array([[1.0, 2.0, 0.5]] * 5)
    assert (R.orient(n, c, np.array([0, 0, 3], dtype=np.float32)) == n).all()
    assert (R.orient(n, c, np.array([0, 0, -3], dtype=np.float32)) == -n).all()
    assert (R.orient(n, c, np.array([7, -9, 0.5], dtype=np.float32)) == n).all()              # in the plane: t == 0
    assert (R.orient(n, c, np.array([0, np.nan, -3], dtype=np.float32)) == n).all()
    assert (R.orient(n, c, np.array([np.inf, 0, -3], dtype=np.float32)) == n).all()
    assert (R.orient(n, c, None) == n).all()


def test_flags_are_per_point():
    rng = np.random.default_rng(8)
    m, n, k = 30, 12, 4
    cloud = rng.standard_normal((m, 3)).astype(np.float32)
    index = rng.integers(0, m - 3, size=(n, k))
    clean = R.normals(cloud, index)
    assert (clean[3] == 0).all() and np.isfinite(clean[0]).all()
    bad_index = index.copy()
    bad_index[2, 1], bad_index[5, 3] = -1, m
    cloud2 = cloud.copy()
    cloud2[m - 1, 0], cloud2[m - 2, 2], cloud2[m - 3, 1] = np.nan, 2.0 ** 62, 2.0 ** 61           # (the bound itself is served)
    bad_index[7, 0], bad_index[9, 2], bad_index[10, 2] = m - 1, m - 2, m - 3
    got = R.normals(cloud2, bad_index)
    assert got[3].tolist() == [0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0]
    flagged = got[3] == 1
    untouched = ~flagged & (np.arange(n) != 10)
    for o, c in zip(got[:3], clean[:3]):
        assert np.isnan(o[flagged]).all() and np.array_equal(o[untouched], c[untouched]) and np.isfinite(o[10]).all()
    allbad = R.normals(cloud, np.full((n, k), -1))
    assert (allbad[3] == 1).all() and all(np.isnan(o).all() for o in allbad[:3])


def test_surface_variation():
    lam = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 2.0], [1.0, 1.0, 1.0], [1.0, 2.0, 5.0]])
    assert R.surface_variation(lam).tolist() == [0.0, 0.0, 1.0 / 3.0, 0.125]
    torch = pytest.importorskip("torch")
    from dpf_nets_amd.metrics import surface_variation
    got = surface_variation(torch.from_numpy(lam))
    assert got.dtype == torch.float64 and got.tolist() == [0.0, 0.0, 1.0 / 3.0, 0.125]


def test_cpu_tensors_and_bad_k_are_refused_without_a_gpu():
    torch = pytest.importorskip("torch")
    from dpf_nets_amd.metrics import estimate_normals, normals_from_index
    pts = torch.randn(2, 40, 3)
    with pytest.raises(RuntimeError):
        estimate_normals(pts, 8)
    with pytest.raises(RuntimeError):
        normals_from_index(pts, torch.zeros((2, 40, 8), dtype=torch.int32))
    for k in (2, 33, 41):
        with pytest.raises(ValueError):
            estimate_normals(pts, k)


# ---- the build: normals.o through the one rule, refused where it spills ------------------------------------------------------------
def test_make_builds_normals_o_through_the_one_rule_with_a_no_scratch_check_that_bites(tmp_path):
    csrc = os.path.join(ROOT, "dpf_nets_amd", "csrc")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "normals.o"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    cmds = [ln.split() for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("make")]
    assert len(cmds) == 4, cmds
    listing, gate, check, obj = cmds
    assert listing[-3:] == ["normals.hip", "-o", "normals.s"] and "-S" in listing and "-ffp-contract=off" in listing
    assert gate[1].endswith("mfma_overlap_check.py") and gate[-1] == "normals.s"
    assert check[1:] == ["../../tools/no_scratch_check.py", "normals_kernel", "normals.s"]
    assert obj[-3:] == ["normals.hip", "-o", "normals.o"] and "-ffp-contract=off" in obj
    assert set(listing[:-2]) - {"-S", "--cuda-device-only"} == set(obj[:-2]) - {"-c"}         # the checked listing and the object: one build
    link = subprocess.run(["make", "-n", "-B", "-C", csrc], capture_output=True, text=True, timeout=60).stdout
    assert any("-shared" in ln and " normals.o" in ln for ln in link.splitlines())
    tool = os.path.join(ROOT, "tools", "no_scratch_check.py")
    spilled = tmp_path / "spilled.s"
    spilled.write_text("_ZN14normals_kernelILi32EEE: ; @kernel\n\tscratch_load_dword v1, off\n.Lfunc_end0:\n")
    clean = tmp_path / "clean.s"
    clean.write_text("_ZN14normals_kernelILi32EEE: ; @kernel\n\tv_add_f64 v[0:1], v[2:3], v[4:5]\n.Lfunc_end0:\n")
    absent = tmp_path / "absent.s"
    absent.write_text("_ZN5otherE: ; @kernel\n\tscratch_load_dword v1, off\n.Lfunc_end0:\n")
    run = lambda p: subprocess.run([sys.executable, tool, "normals_kernel", str(p)], capture_output=True, text=True, timeout=60).returncode
    assert run(spilled) == 1 and run(clean) == 0 and run(absent) == 1


def test_dispatch_picks_the_smallest_capacity(tmp_path):
    """dispatch.h (host-only C++): normals_form over every k"""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include "dispatch.h"\nint main() { for (int k = 0; k <= 34; ++k) std::printf("%d ", dispatch::normals_form(k).kcap);'
                   ' std::printf("%d %d\\n", dispatch::NORMALS_SWEEPS, dispatch::NORMALS_WG_POINTS); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "dpf_nets_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    want = [0, 0, 0, 4, 4] + [8] * 4 + [16] * 8 + [32] * 16 + [0, 0]
    assert out[:35] == want and out[35:] == [R.SWEEPS, 64]
