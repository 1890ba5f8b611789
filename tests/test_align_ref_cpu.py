"""The numpy restatement of dpf_rigid_fit and dpf_icp (tests/align_ref.py) against an independent float64 SVD solution (Kabsch /
Umeyama with the determinant fix): what keeps the bound of tests/test_gpu_align.py honest, and the arbiter of Horn's formula and its
sign conventions.  The bound on R, t and s is MEASURED here (the worst deviation over the kinds, times 8, never looser than 2^-40) and
written down as align_ref.ALIGN_BOUND; the sweep count's floor is measured here too.

Also here: the tree and the block order on a hand-made case, the fixed point, the monotone rmse, the trim, the tie rule, refusal, the
Python surface's argument checks that need no GPU, the build of align.o and the no-scratch check that guards it, and align_form."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import align_ref as A                                                                        # noqa: E402

SIZES = (3, 7, 300, 700)
SEEDS = 12


def svd_fit(p, q, w=None, with_scale=False):
    """Kabsch / Umeyama in float64 with the determinant fix: nothing of the restatement's"""
    p, q = p.astype(np.float64), q.astype(np.float64)
    w = np.ones(len(p)) if w is None else w.astype(np.float64)
    W = w.sum()
    pm, qm = (w[:, None] * p).sum(0) / W, (w[:, None] * q).sum(0) / W
    pc, qc = p - pm, q - qm
    U, D, Vt = np.linalg.svd((w[:, None] * qc).T @ pc)
    fix = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ np.diag(fix) @ Vt
    s = (D * fix).sum() / (w * (pc * pc).sum(1)).sum() if with_scale else 1.0
    return R, qm - s * R @ pm, s, np.linalg.det(U) * np.linalg.det(Vt) < 0


def deviation(T, R, t, s, p, q):
    """the largest of |dR|, |ds| / s and |dt| / (|t| + s * the source's largest coordinate + the target's)"""
    R1, t1, s1 = A.unpack(T)
    extent = np.abs(t).max() + abs(s) * np.abs(p).max() + np.abs(q).max()
    return max(np.abs(R1 - R).max(), abs(s1 - s) / abs(s), np.abs(t1 - t).max() / extent)


def residual(T, p, q, w=None):
    w = np.ones(len(p)) if w is None else w.astype(np.float64)
    return float((w * ((A.apply(T, p) - q.astype(np.float64)) ** 2).sum(1)).sum())


def cases(kind):
    for seed in range(SEEDS):
        n = SIZES[seed % 4]
        yield (n, seed) + A.make_fit(kind, n, 100 * seed + n)


def worst_deviation(kind, sweeps):
    worst = 0.0
    for n, seed, p, q, w, ws in cases(kind):
        r = A.rigid_fit(p, q, w, ws, sweeps=sweeps)
        assert r["status"] == 0, (kind, n, seed)
        R, t, s, _ = svd_fit(p, q, w, ws)
        worst = max(worst, deviation(r["T"], R, t, s, p, q))
    return worst


def test_the_restatement_agrees_with_the_svd_solution_and_the_bound_is_what_was_measured():
    worst = {}
    for kind in A.FIT_KINDS:
        worst[kind] = worst_deviation(kind, A.SWEEPS)
        print("%-10s worst deviation from the SVD solution %.3g" % (kind, worst[kind]))
        for n, seed, p, q, w, ws in cases(kind):
            r = A.rigid_fit(p, q, w, ws)
            R1, _, s1 = A.unpack(r["T"])
            assert abs(np.linalg.det(R1) - 1.0) <= A.ALIGN_BOUND and np.abs(R1 @ R1.T - np.eye(3)).max() <= A.ALIGN_BOUND
            assert ws or s1 == 1.0
    top = max(worst.values())
    print("the worst of all: %.3g; 8 x = %.3g; ALIGN_BOUND = %.3g; 2^-40 = %.3g" % (top, 8 * top, A.ALIGN_BOUND, 2.0 ** -40))
    assert top <= A.WORST_MEASURED <= 1.25 * top                                             # the constant is the measurement, not a guess
    assert A.ALIGN_BOUND == min(8 * A.WORST_MEASURED, 2.0 ** -40)


def test_a_reflected_pair_gets_a_proper_rotation_with_the_det_fixed_svd_residual():
    seen = 0
    for n, seed, p, q, w, ws in cases("reflection"):
        R, t, s, improper = svd_fit(p, q)
        seen += int(improper or n == 3)                                                       # (three points lie in a plane: either sign fits)
        r = A.rigid_fit(p, q)
        assert abs(np.linalg.det(A.unpack(r["T"])[0]) - 1.0) <= A.ALIGN_BOUND
        mine, theirs = residual(r["T"], p, q), residual(A.pack(R, t, s), p, q)
        spread = float(((q.astype(np.float64) - q.astype(np.float64).mean(0)) ** 2).sum())       # (a residual is a difference of sums this large)
        assert abs(mine - theirs) <= 1e-12 * theirs + 1e-13 * spread and (n == 3 or theirs > 1e-3 * spread), (n, seed, mine, theirs)
        # the closed-form rmse is the residual's, up to its cancellation
        assert abs(r["rmse"] ** 2 * n - mine) <= 2.0 ** -40 * float(r["sums"][17])
    assert seen == SEEDS                                                                     # every pair's unconstrained optimum is improper


def test_weights_with_zeros_leave_their_points_out():
    p, q, w, ws = A.make_fit("weighted", 300, 5)
    assert (w == 0).sum() >= 50
    keep = w > 0
    full, cut = A.rigid_fit(p, q, w), A.rigid_fit(p[keep], q[keep], w[keep])
    R, t, s, _ = svd_fit(p[keep], q[keep], w[keep])
    assert deviation(full["T"], R, t, s, p, q) <= A.ALIGN_BOUND and deviation(cut["T"], R, t, s, p, q) <= A.ALIGN_BOUND


def test_collinear_points_reach_the_svd_residual():
    """R is not unique there (any turn about the line): only the residual is compared"""
    for seed in range(6):
        p, q, _, _ = A.make_fit("collinear", 40, seed)
        R, t, s, _ = svd_fit(p, q)
        r = A.rigid_fit(p, q)
        assert r["status"] == 0 and abs(np.linalg.det(A.unpack(r["T"])[0]) - 1.0) <= A.ALIGN_BOUND
        mine, theirs = residual(r["T"], p, q), residual(A.pack(R, t, s), p, q)
        assert mine <= theirs * (1 + 1e-9), (seed, mine, theirs)


def test_one_sweep_fewer_than_the_floor_is_not_enough_and_the_floor_equals_the_shipped_count():
    assert A.SWEEPS == A.FLOOR_SWEEPS + 2
    short = floor = shipped = 0.0
    for kind in ("gauss", "offset", "small", "large", "scale"):
        d = {sw: worst_deviation(kind, sw) for sw in (A.FLOOR_SWEEPS - 1, A.FLOOR_SWEEPS, A.SWEEPS)}
        print("%-8s %d sweeps %.3g, %d sweeps %.3g, %d sweeps %.3g" % (kind, A.FLOOR_SWEEPS - 1, d[A.FLOOR_SWEEPS - 1], A.FLOOR_SWEEPS,
                                                                     d[A.FLOOR_SWEEPS], A.SWEEPS, d[A.SWEEPS]))
        assert d[A.FLOOR_SWEEPS - 1] > 5 * d[A.FLOOR_SWEEPS], kind                          # visibly above the floor
        short, floor, shipped = max(short, d[A.FLOOR_SWEEPS - 1]), max(floor, d[A.FLOOR_SWEEPS]), max(shipped, d[A.SWEEPS])
    for kind in A.FIT_KINDS:
        for n, seed, p, q, w, ws in cases(kind):
            a, b = A.rigid_fit(p, q, w, ws, sweeps=A.FLOOR_SWEEPS)["T"], A.rigid_fit(p, q, w, ws, sweeps=A.SWEEPS)["T"]
            R, t, s = A.unpack(b)
            assert deviation(a, R, t, s, p, q) <= A.ALIGN_BOUND, (kind, n, seed)


def test_the_tree_and_the_block_order_on_a_hand_made_case():
    """257 points: block 0 is a tree over 256 terms, block 1 holds one term and 255 zeros, and block 0's sum comes first.  The terms
    2^53, 1, 1, ... tell the tree from a running sum: ascending addition loses every 1, the tree keeps the pairs it adds first."""
    x = np.ones(257)
    x[0] = 2.0 ** 53
    t = np.zeros((257, A.NSUMS))
    t[:, 0] = x
    got = A.reduce_terms(t)[0]
    blocks = x[:256].copy()
    for stride in (128, 64, 32, 16, 8, 4, 2, 1):
        for i in range(stride):
            blocks[i] = blocks[i] + blocks[i + stride]
    assert got == blocks[0] + 1.0
    running = 0.0
    for v in x:
        running = running + v
    assert running == 2.0 ** 53 and got > running + 200                                      # the tree kept what a running sum loses
    # the same through the sums of a fit: weights as the terms, every point at its pivot but one
    p = np.zeros((257, 3), dtype=np.float32)
    p[5] = [1.0, 2.0, 3.0]
    w = np.ones(257, dtype=np.float32)
    w[0] = 2.0 ** 25
    S = A.rigid_fit(p, p, w)["sums"]
    assert S[0] == 2.0 ** 25 + 256 and S[1] == 1.0 and S[7] == 1.0 and S[16] == 14.0 and S[17] == 14.0


def test_icp_of_a_moved_copy_reaches_the_fixed_point():
    src, dst = A.make_pair("rotated", 200, 200, 3)
    r = A.icp(src, dst, iters=30)
    assert r["status"] == 0 and r["iterations"] < 30 and r["changed"][-1] == 0
    moved = A.apply(r["T"], src)
    assert np.abs(moved - dst[r["index"]].astype(np.float64)).max() < 1e-6
    assert len(set(r["index"].tolist())) == 200 and r["index"][0] == 0
    R, t, s = A.unpack(r["T"])
    assert np.abs(R - A.KNOWN_R).max() < 1e-6 and np.abs(t - A.KNOWN_T).max() < 1e-6 and s == 1.0
    assert (r["rmse"][r["iterations"]:] == r["rmse"][r["iterations"]]).all() and r["rmse"][-1] < 1e-6
    # on a copy of itself, from a known turn: the index is the identity
    turned = A.icp(dst, dst, iters=30, init=A.pack(A.KNOWN_R, A.KNOWN_T))
    assert turned["iterations"] < 30 and turned["changed"][-1] == 0 and np.array_equal(turned["index"], np.arange(200))
    assert np.abs(A.unpack(turned["T"])[0] - np.eye(3)).max() < 1e-7


def test_rmse_never_rises_for_untrimmed_rigid_icp():
    for seed, kind in enumerate(("gauss", "rotated", "offset")):
        src, dst = A.make_pair(kind, 150, 170, 20 + seed)
        r = A.icp(src, dst, iters=12, init=A.make_init(seed, 8.0) if kind != "offset" else None)
        assert (np.diff(r["rmse"]) <= 1e-12 * r["rmse"][:-1]).all(), (kind, r["rmse"])


def test_a_trim_that_excludes_everything_is_degenerate_and_returns_the_init():
    src, dst = A.make_pair("gauss", 50, 60, 1)
    init = A.make_init(4)
    r = A.icp(src + np.float32(50), dst, iters=5, max_dist2=1e-3, init=init)
    assert r["status"] == A.DEGENERATE and np.array_equal(r["T"], init) and r["iterations"] == 0
    assert (r["index"] == -1).all() and (r["inliers"] == 0).all() and np.isnan(r["rmse"]).all() and np.isfinite(r["dist"]).all()
    part = A.icp(*A.make_pair("far", 60, 60, 2), iters=3, max_dist2=25.0)
    assert part["status"] == 0 and (part["index"][::3] == -1).all() and part["inliers"][-1] == 40


def test_duplicated_target_points_match_the_lower_index():
    src, dst = A.make_pair("gauss", 40, 30, 6)
    dst = np.concatenate([dst, dst[::-1]])
    index, dist, _, _ = A.match(src, dst, A.IDENTITY)
    assert (index < 30).all()
    lat = A.match(*A.make_pair("lattice", 80, 90, 7), A.IDENTITY)
    d = A.distances(A.make_pair("lattice", 80, 90, 7)[0], A.make_pair("lattice", 80, 90, 7)[1])
    assert all((d[i, :lat[0][i]] > lat[1][i]).all() and d[i, lat[0][i]] == lat[1][i] for i in range(80))


def test_a_nan_refuses_its_slot_only():
    src, dst = A.make_pair("gauss", 30, 30, 8)
    clean = A.icp(src, dst, iters=2)
    for what in ("src", "dst", "init", "big"):
        s2, d2, init = src.copy(), dst.copy(), None
        if what == "src":
            s2[7, 1] = np.nan
        elif what == "dst":
            d2[29, 2] = np.inf
        elif what == "big":
            d2[3, 0] = np.float32(2.0 ** 30 * 1.001)
        else:
            init = A.IDENTITY.copy()
            init[10] = np.nan
        r = A.icp(s2, d2, iters=2, init=init)
        assert r["status"] == A.REFUSED and np.isnan(r["T"]).all() and (r["index"] == -1).all() and np.isnan(r["dist"]).all(), what
    d2 = dst.copy()
    d2[3, 0] = np.float32(2.0 ** 30)                                                          # the bound itself is served
    assert A.icp(src, d2, iters=1)["status"] == 0
    again = A.icp(src, dst, iters=2)
    assert np.array_equal(again["T"], clean["T"])
    assert A.rigid_fit(src, dst, np.full(30, -1.0, dtype=np.float32))["status"] == A.REFUSED
    assert A.rigid_fit(src[:2], dst[:2])["status"] == A.DEGENERATE
    assert A.rigid_fit(np.repeat(src[:1], 9, 0), dst[:9], with_scale=True)["status"] == A.DEGENERATE


# ---- the package and the build -----------------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments_are_refused_without_a_gpu():
    torch = pytest.importorskip("torch")
    from dpf_nets_amd.metrics import icp, rigid_fit, apply_transform, RigidTransform
    a, b = torch.randn(2, 40, 3), torch.randn(2, 50, 3)
    for call in (lambda: icp(a, b), lambda: rigid_fit(a, a), lambda: icp(a.double(), b), lambda: rigid_fit(a[0], a[0])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    T = RigidTransform(torch.eye(3, dtype=torch.float64).expand(2, 3, 3), torch.ones(2, 3, dtype=torch.float64), torch.full((2,), 2.0, dtype=torch.float64))
    x = a.clone().requires_grad_(True)
    y = apply_transform(T, x)
    assert y.dtype == torch.float32 and torch.allclose(y, 2 * a + 1)
    y.sum().backward()
    assert torch.allclose(x.grad, torch.full_like(a, 2.0))
    yc = apply_transform(T, a.transpose(1, 2), channels_first=True)
    assert torch.equal(yc.transpose(1, 2), y.detach())


def test_make_builds_align_o_through_the_one_rule_with_a_no_scratch_check_that_bites(tmp_path):
    csrc = os.path.join(ROOT, "dpf_nets_amd", "csrc")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "align.o"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    cmds = [ln.split() for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("make")]
    assert len(cmds) == 4, cmds
    listing, gate, check, obj = cmds
    assert listing[-3:] == ["align.hip", "-o", "align.s"] and "-S" in listing and "-ffp-contract=off" in listing
    assert gate[1].endswith("mfma_overlap_check.py") and gate[-1] == "align.s"
    assert check[1:] == ["../../tools/no_scratch_check.py", "align_", "align.s"]
    assert obj[-3:] == ["align.hip", "-o", "align.o"] and "-ffp-contract=off" in obj
    assert set(listing[:-2]) - {"-S", "--cuda-device-only"} == set(obj[:-2]) - {"-c"}         # the checked listing and the object: one build
    link = subprocess.run(["make", "-n", "-B", "-C", csrc], capture_output=True, text=True, timeout=60).stdout
    assert any("-shared" in ln and " align.o" in ln for ln in link.splitlines())
    tool = os.path.join(ROOT, "tools", "no_scratch_check.py")
    spilled = tmp_path / "spilled.s"
    spilled.write_text("_ZN12_GLOBAL__N_118align_solve_kernelILb0EEE: ; @kernel\n\tscratch_store_dwordx2 off, v[1:2], off\n.Lfunc_end0:\n")
    clean = tmp_path / "clean.s"
    clean.write_text("_ZN12_GLOBAL__N_118align_solve_kernelILb0EEE: ; @kernel\n\tv_add_f64 v[0:1], v[2:3], v[4:5]\n.Lfunc_end0:\n")
    absent = tmp_path / "absent.s"
    absent.write_text("_ZN5otherE: ; @kernel\n\tscratch_load_dword v1, off\n.Lfunc_end0:\n")
    run = lambda p: subprocess.run([sys.executable, tool, "align_", str(p)], capture_output=True, text=True, timeout=60).returncode
    assert run(spilled) == 1 and run(clean) == 0 and run(absent) == 1
    built = os.path.join(csrc, "align.s")
    if os.path.exists(built) and os.path.getmtime(built) >= os.path.getmtime(os.path.join(csrc, "align.hip")):
        text = open(built).read()
        assert run(built) == 0 and text.count("align_match_kernel") and text.count("align_solve_kernel")


def test_align_form_is_pure_and_picks_as_expected(tmp_path):
    """dispatch.h (host-only C++): the block count, the launch count, the constants"""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include <initializer_list>\n#include "dispatch.h"\nint main() { const int ns[] = {-1, 0, 1, 256, 257, 600, 2048, 2500};\n'
                   ' for (int n : ns) for (int it : {-1, 0, 1, 30}) { auto f = dispatch::align_form(n, it); auto g = dispatch::align_form(n, it);\n'
                   '  if (f.blocks != g.blocks || f.launches != g.launches) return 1; std::printf("%ld %ld ", f.blocks, f.launches); }\n'
                   ' std::printf("%d %d %d %d %d\\n", dispatch::ALIGN_SWEEPS, dispatch::ALIGN_WG_POINTS, dispatch::ALIGN_TILE, dispatch::ALIGN_SUMS,'
                   ' dispatch::ALIGN_MIN_INLIERS); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "dpf_nets_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    want = []
    for n in (-1, 0, 1, 256, 257, 600, 2048, 2500):
        for it in (-1, 0, 1, 30):
            want += [0, 0] if n < 1 or it < 0 else [(n + 255) // 256, 2 * (it + 1)]
    assert out[:-5] == want and out[-5:] == [A.SWEEPS, A.BLOCK, 256, A.NSUMS, A.MIN_INLIERS]
