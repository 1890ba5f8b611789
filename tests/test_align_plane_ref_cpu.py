"""The numpy restatement of dpf_icp_plane (tests/align_plane_ref.py) against independent float64 linear algebra, and what of the
contract needs no GPU: the restated LDL^T solve against numpy.linalg.lstsq on the same damped system (the deviation is MEASURED here
and written down as align_plane_ref.SOLVE_WORST_MEASURED; the bound is that figure times 8), the sign of the normals, the tree and the
block order, the pivot rule, the orthogonality bound, refusal, degeneracy, tol, align_plane_form, the package's argument checks, and
the recovery of a known pose where point-to-point ICP stalls.  Failing without the feature: the parent commit has neither
align_plane_form nor metrics.icp_plane."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import align_ref as A                                                                        # noqa: E402
import align_plane_ref as P                                                                  # noqa: E402


def first_sums(src, dst, normals, init=None, max_dist2=0.0):
    r = P.icp_plane(src, dst, normals, iters=0, max_dist2=max_dist2, init=init)
    assert r["status"] == 0
    return r["sums"], int(r["inliers"][0])


def solve_cases():
    """(name, src, dst, normals, init): every pair kind and every fit kind of align_ref under seeded unit normals, an ellipsoid pair
    under its analytic normals, a planar and a collinear target"""
    for s, kind in enumerate(A.PAIR_KINDS):
        src, dst = A.make_pair(kind, 300, 280, 50 + s)
        yield kind, src, dst, P.pair_normals(dst, s), (A.make_init(s, 3.0) if kind in ("gauss", "rotated", "far") else None)
    for s, kind in enumerate(A.FIT_KINDS + ("collinear",)):
        src, dst, _, _ = A.make_fit(kind, 300, 70 + s)
        yield "fit-" + kind, src, dst, P.pair_normals(dst, 20 + s), None
    src, dst, nrm, _, _ = P.make_ellipsoid_pair(600, 513, 0)
    yield "ellipsoid", src, dst, nrm, None
    yield ("planar-target",) + P.make_planar_target(200, 220, 1) + (None,)
    yield ("collinear-target",) + P.make_collinear_target(200, 220, 2) + (None,)


def solve_deviation(S):
    """|A (x - x_lstsq)| / |b| in the maximum norm, A the undamped matrix: the difference of the two solutions where the system sees
    it (a direction the data leave free is free in both)"""
    M, b = P.system(S)
    x, ok = P.ldl_solve(S)
    damped = M + np.diag(np.diag(M) * (P.DAMP - 1.0))
    want = np.linalg.lstsq(damped, -b, rcond=None)[0]
    return float(np.abs(M @ (np.array(x) - want)).max() / np.abs(b).max()), ok


def test_the_restated_solve_agrees_with_lstsq_and_the_bound_is_what_was_measured():
    worst = {}
    for name, src, dst, nrm, init in solve_cases():
        S, _ = first_sums(src, dst, nrm, init)
        worst[name], ok = solve_deviation(S)
        print("%-18s deviation from lstsq %.3g  pivots kept %s" % (name, worst[name], "".join("x" if o else "-" for o in ok)))
    top = max(worst.values())
    print("the worst of all: %.3g; SOLVE_BOUND = 8 x %.3g" % (top, P.SOLVE_WORST_MEASURED))
    assert top <= P.SOLVE_WORST_MEASURED <= 1.25 * top                                       # the constant is the measurement, not a guess
    assert P.SOLVE_BOUND == 8 * P.SOLVE_WORST_MEASURED


def test_flipping_the_sign_of_any_subset_of_the_normals_changes_no_bit():
    src, dst, nrm, _, _ = P.make_ellipsoid_pair(257, 255, 3)
    rng = np.random.default_rng(0)
    base = P.icp_plane(src, dst, nrm, iters=4, max_dist2=0.3)
    for subset in (rng.random(255) < 0.5, np.ones(255, dtype=bool), np.arange(255) == 7):
        flipped = np.where(subset[:, None], -nrm, nrm)
        got = P.icp_plane(src, dst, flipped, iters=4, max_dist2=0.3)
        for key in ("T", "index", "dist", "rmse", "rmse_plane", "step", "inliers", "sums"):
            assert np.array_equal(base[key], got[key], equal_nan=True), key
            assert np.array_equal(np.signbit(base[key]), np.signbit(got[key])), key            # (a zero keeps its sign too)
    # lattice coordinates and axis normals: full of zero products, the case the + 0.0 is there for
    src, dst = A.make_pair("lattice", 64, 64, 5)
    nrm = np.eye(3)[np.arange(64) % 3]
    a, b = P.icp_plane(src, dst, nrm, iters=0)["sums"], P.icp_plane(src, dst, -nrm, iters=0)["sums"]
    assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and (a[1:22] == 0).any()


def test_the_tree_and_the_block_order_on_257_hand_made_terms():
    """257 matched points whose squared distances are 2^53, 1, 1, ...: a running sum loses every 1, the tree keeps the pairs it adds
    first; block 1 holds one term and comes after block 0.  Through the thirty-one sums: column 28 is S_d, column 0 counts."""
    n = 257
    dist = np.ones(n, dtype=np.float32)
    dist[0] = np.float32(2.0 ** 53)
    y = np.zeros((n, 3), dtype=np.float32)
    dst = np.zeros((n, 3), dtype=np.float32)
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    S = P.plane_sums(y, dst, nrm, np.arange(n, dtype=np.int32), dist, np.ones(n))
    blocks = dist[:256].astype(np.float64)
    for stride in (128, 64, 32, 16, 8, 4, 2, 1):
        for i in range(stride):
            blocks[i] = blocks[i] + blocks[i + stride]
    assert S[28] == blocks[0] + 1.0 and S[0] == 257.0
    running = 0.0
    for v in dist.astype(np.float64):
        running = running + v
    assert running == 2.0 ** 53 and S[28] > running + 200
    assert S[1 + P.tri(5, 5)] == 257.0 and S[1 + P.tri(3, 3)] == 0.0 and S[29] == 0.0      # a = (0, 0, 0, 0, 0, 1), r = 0
    assert [P.tri(i, j) for i in range(6) for j in range(i, 6)] == list(range(21))           # row-major upper triangle


def hand_sums(M, b):
    S = np.zeros(P.NSUMS)
    S[0] = 10.0
    for i in range(6):
        for j in range(i, 6):
            S[1 + P.tri(i, j)] = M[i][j]
    S[22:28] = b
    S[30] = 10.0
    return S


def test_a_pivot_that_is_not_positive_drops_its_unknown_on_a_hand_made_singular_matrix():
    M = np.diag([2.0, 0.0, 4.0, 1.0, 1.0, 8.0])                                               # a zero pivot: unknown 1 has no data
    M[0, 2] = M[2, 0] = 1.0
    b = np.array([1.0, 0.0, 2.0, -3.0, 0.5, 4.0])
    x, ok = P.ldl_solve(hand_sums(M, b))
    assert ok == [True, False, True, True, True, True] and x[1] == 0.0
    keep = [0, 2, 3, 4, 5]
    damped = M + np.diag(np.diag(M) * (P.DAMP - 1.0))
    want = np.linalg.solve(damped[np.ix_(keep, keep)], -b[keep])
    assert np.abs(np.array(x)[keep] - want).max() <= 1e-15 * np.abs(want).max() * 8
    # a NEGATIVE second pivot (1 - 4 < 0, not a sum of squares at all): the same rule, the rest is the system without unknown 1
    M = np.eye(6)
    M[0, 1] = M[1, 0] = 2.0
    M[1, 4] = M[4, 1] = 0.5
    x, ok = P.ldl_solve(hand_sums(M, b))
    assert ok == [True, False, True, True, True, True] and x[1] == 0.0
    damped = M + np.diag(np.diag(M) * (P.DAMP - 1.0))
    want = np.linalg.solve(damped[np.ix_(keep, keep)], -b[keep])
    assert np.abs(np.array(x)[keep] - want).max() <= 1e-15 * np.abs(want).max() * 8
    # every pivot dropped: the zero matrix gives the zero step, and the composition leaves R in place up to its rounding
    x, ok = P.ldl_solve(hand_sums(np.zeros((6, 6)), np.zeros(6)))
    assert not any(ok) and x == [0.0] * 6
    assert P.increment(x) == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def test_the_orthogonality_bound_holds_over_fifty_compositions():
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        T = A.IDENTITY.copy()
        for k in range(50):
            x = list(np.concatenate([rng.standard_normal(3) * 10.0 ** rng.uniform(-6, 0), rng.standard_normal(3)]))
            T = P.compose(T, x, rng.standard_normal(3).astype(np.float32))
            R = A.unpack(T)[0]
            dev = np.abs(R.T @ R - np.eye(3)).max()
            assert dev <= P.ortho_bound(k + 1), (seed, k, dev)
        worst = max(worst, dev)
        assert abs(np.linalg.det(R) - 1.0) <= 3 * P.ortho_bound(50)
    print("worst |R^T R - I| after 50 compositions %.3g (bound %.3g)" % (worst, P.ortho_bound(50)))
    # a first-order check of the increment itself: dR = I + [omega]x up to omega^2
    w = [1e-5, -2e-5, 3e-5]
    dR = np.array(P.increment(w + [0.0, 0.0, 0.0]))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    assert np.abs(dR - (np.eye(3) + K)).max() <= 1e-9


def test_refusal_degeneracy_and_the_nan_normal_rule():
    src, dst, nrm, _, _ = P.make_ellipsoid_pair(40, 50, 1)
    clean = P.icp_plane(src, dst, nrm, iters=2)
    assert clean["status"] == 0
    for what in ("src", "dst", "init", "scale", "normal"):
        s2, d2, n2, init = src.copy(), dst.copy(), nrm.copy(), None
        if what == "src":
            s2[7, 1] = np.nan
        elif what == "dst":
            d2[3, 0] = np.float32(2.0 ** 30 * 1.001)
        elif what == "init":
            init = A.IDENTITY.copy()
            init[10] = np.inf
        elif what == "scale":
            init = A.IDENTITY.copy()
            init[12] = 1.5
        else:
            n2[49, 2] = 2.0 ** 30 * 1.5                                                       # finite and too large: a VALUE error
        r = P.icp_plane(s2, d2, n2, iters=2, init=init)
        assert r["status"] == P.REFUSED and np.isnan(r["T"]).all() and (r["index"] == -1).all() and np.isnan(r["step"]).all(), what
    n2 = nrm.copy()
    n2[5, 0] = 2.0 ** 30                                                                     # the bound itself is served
    assert P.icp_plane(src, dst, n2, iters=1)["status"] == 0
    # a normal that is not finite takes its own matches out and nothing else
    first = P.icp_plane(src, dst, nrm, iters=0)
    hit = int(first["index"][0])
    for bad in (np.nan, np.inf):
        n2 = nrm.copy()
        n2[hit, 1] = bad
        r = P.icp_plane(src, dst, n2, iters=0)
        lost = first["index"] == hit
        assert r["status"] == 0 and np.array_equal(r["index"], first["index"]) and r["inliers"][0] == 40 - lost.sum()
        keep = P.plane_sums(P.match(src, dst, nrm, A.IDENTITY)[4][~lost], dst, nrm, first["index"][~lost], first["dist"][~lost],
                            np.ones((~lost).sum()))
        assert r["sums"][0] == keep[0] and np.isfinite(r["sums"]).all()
    # five inliers: degenerate, the init is kept
    init = A.make_init(3, 2.0)
    r = P.icp_plane(src[:5], dst, nrm, iters=3, init=init)
    assert r["status"] == P.DEGENERATE and np.array_equal(r["T"], init) and r["iterations"] == 0 and (r["inliers"] == 5).all()
    assert (r["step"] == 0.0).all() and np.isfinite(r["rmse_plane"]).all()
    assert P.icp_plane(src[:6], dst, nrm, iters=3, init=init)["status"] == 0
    far = P.icp_plane(src + np.float32(50), dst, nrm, iters=3, max_dist2=1e-3)
    assert far["status"] == P.DEGENERATE and (far["index"] == -1).all() and np.isnan(far["rmse"]).all()


def test_tol_zero_stops_on_a_zero_step_only_and_a_tol_stops_a_run():
    src, dst, nrm, _, _ = P.make_ellipsoid_pair(257, 255, 0)
    loose = P.icp_plane(src, dst, nrm, iters=30, tol=1e-3)
    tight = P.icp_plane(src, dst, nrm, iters=30, tol=1e-9)
    exact = P.icp_plane(src, dst, nrm, iters=12, tol=0.0)
    assert loose["status"] == tight["status"] == 0
    assert 0 < loose["iterations"] < tight["iterations"] <= 30
    k = loose["iterations"]
    assert loose["changed"][-1] == 0 and loose["step"][k - 1] <= 1e-3 and loose["step"][k] == 0.0
    assert (loose["step"][k:] == 0.0).all() and (loose["rmse_plane"][k:] == loose["rmse_plane"][k]).all()
    assert all(not (c == 0 and s <= 1e-3) for c, s in zip(loose["changed"][1:-1], loose["step"][:k - 1]))   # it stopped at the FIRST such match
    # tol = 0: steps of 1e-17 are not zero; the run goes on to its end unless a step is exactly 0
    assert exact["iterations"] == 12 or exact["step"][exact["iterations"] - 1] == 0.0
    assert np.array_equal(exact["T"], P.icp_plane(src, dst, nrm, iters=12, tol=0.0)["T"])
    # an exactly zero step: source on the target's plane already
    s2, d2, n2 = P.make_planar_target(50, 60, 4)
    s2[:, :] = np.concatenate([s2[:, :2] * 0 + d2[:50, :2], np.full((50, 1), 0.25, dtype=np.float32)], axis=1)
    z = P.icp_plane(s2, d2, n2, iters=9, tol=0.0)
    assert z["status"] == 0 and z["iterations"] == 1 and z["step"][0] == 0.0 and z["rmse_plane"][0] == 0.0


def test_align_plane_form_is_pure_and_picks_as_expected(tmp_path):
    """dispatch.h (host-only C++): the block count, the launch count, the partials, the constants; align_form is as it was"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include <initializer_list>\n#include "dispatch.h"\nint main() { const int ns[] = {-1, 0, 1, 256, 257, 600, 2048, 2500};\n'
                   ' for (int n : ns) for (int it : {-1, 0, 1, 30}) { auto f = dispatch::align_plane_form(n, it); auto g = dispatch::align_plane_form(n, it);\n'
                   '  auto h = dispatch::align_form(n, it);\n'
                   '  if (f.blocks != g.blocks || f.launches != g.launches || f.partial_doubles != g.partial_doubles) return 1;\n'
                   '  if (f.blocks != h.blocks || f.launches != h.launches) return 2;\n'
                   '  std::printf("%ld %ld %ld ", f.blocks, f.launches, f.partial_doubles); }\n'
                   ' std::printf("%d %d %d\\n", dispatch::ALIGN_PLANE_SUMS, dispatch::ALIGN_PLANE_MIN_INLIERS, dispatch::ALIGN_SUMS); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "dpf_nets_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    want = []
    for n in (-1, 0, 1, 256, 257, 600, 2048, 2500):
        for it in (-1, 0, 1, 30):
            want += [0, 0, 0] if n < 1 or it < 0 else [(n + 255) // 256, 2 * (it + 1), 31 * ((n + 255) // 256)]
    assert out[:-3] == want and out[-3:] == [P.NSUMS, P.MIN_INLIERS, A.NSUMS]


def test_cpu_tensors_and_bad_arguments_are_refused_without_a_gpu():
    torch = pytest.importorskip("torch")
    from dpf_nets_amd.metrics import icp_plane, PlaneICPInfo
    from dpf_nets_amd.metrics.align import icp_plane_raw
    a, b = torch.randn(2, 40, 3), torch.randn(2, 50, 3)
    nb = torch.randn(2, 50, 3, dtype=torch.float64)
    for call in (lambda: icp_plane(a, b, nb), lambda: icp_plane(a.double(), b, nb), lambda: icp_plane(a[0], b[0], nb[0]),
                 lambda: icp_plane_raw(a, b, nb)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert PlaneICPInfo._fields == ("index", "dist", "rmse", "inliers", "iterations", "status", "rmse_plane", "step")


def test_point_to_plane_recovers_the_pose_where_point_to_point_stalls():
    src, dst, nrm, R, t = P.make_ellipsoid_pair(600, 513, 0, 5.0)
    plane = P.icp_plane(src, dst, nrm, iters=30, tol=1e-7)
    point = A.icp(src, dst, iters=60)
    e_plane = P.rotation_error_degrees(A.unpack(plane["T"])[0], R)
    e_point = P.rotation_error_degrees(A.unpack(point["T"])[0], R)
    print("rotation error: point-to-plane %.3f degrees after %d solves, point-to-point %.3f after %d"
          % (e_plane, plane["iterations"], e_point, point["iterations"]))
    assert plane["status"] == 0 and e_plane < e_point and e_plane < 0.5
    assert plane["rmse_plane"][-1] < 0.5 * plane["rmse_plane"][0]
    Rg = A.unpack(plane["T"])[0]
    assert np.abs(Rg.T @ Rg - np.eye(3)).max() <= P.ortho_bound(plane["iterations"])
    # the planar target: three unknowns are free; the damped solve moves the plane onto the plane and the free ones do not run away
    s2, d2, n2 = P.make_planar_target(200, 220, 1)
    flat = P.icp_plane(s2, d2, n2, iters=10, tol=1e-12)
    assert flat["status"] == 0 and flat["rmse_plane"][-1] < 1e-6 < flat["rmse_plane"][0]
    assert flat["rmse_plane"][-1] < flat["rmse_plane"][0]
    assert np.abs(A.unpack(flat["T"])[1]).max() < 1.0 and np.isfinite(flat["T"]).all()
    moved = A.apply(flat["T"], s2)
    assert np.abs(moved[:, 2] - 0.25).max() < 1e-5 and np.abs(moved[:, :2]).max() < 2.0
