"""tests/dcd_ref.py, the numpy restatement of dpf_dcd, against the published per-cloud formulation (calc_dcd of Wu et al.: bincount, gather,
exp, mean) in float64 torch on the CPU -- what keeps the bound of tests/test_gpu_dcd.py honest.  The two differ in the order of the
sums alone (a mean against the block tree) and in a reciprocal against a division, so they agree within a few roundings of the mean.

Also here: hand-made cases, n != m with and without non_reg, n_lambda in {0, 0.5, 1, 2}, the tree and the block order on 257 terms,
refusal, dispatch::dcd_form on the host (the cap and cap + 1), the Makefile carrying dcd.o, the package's argument checks that need no
GPU, and compute_all_metrics' dcd= keys on stubs."""
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
import dcd_ref as D                                                                          # noqa: E402

SHAPES = ((1, 1), (2, 2), (63, 257), (257, 63), (300, 300), (513, 255), (1000, 700))


def published(d1, i1, d2, i2, alpha, n_lambda, non_reg):
    """calc_dcd's arithmetic for one cloud, float64 torch: (loss, loss1, loss2, count of side 1's queries, of side 2's)"""
    torch = pytest.importorskip("torch")
    d1, d2 = torch.from_numpy(d1.astype(np.float64)), torch.from_numpy(d2.astype(np.float64))
    i1, i2 = torch.from_numpy(i1.astype(np.int64)), torch.from_numpy(i2.astype(np.int64))
    n, m = d1.numel(), d2.numel()
    frac1, frac2 = n / m, m / n
    if non_reg:
        frac1, frac2 = max(1.0, frac1), max(1.0, frac2)
    e1, e2 = torch.exp(-d1 * alpha), torch.exp(-d2 * alpha)
    c1 = torch.bincount(i1, minlength=m).gather(0, i1)
    c2 = torch.bincount(i2, minlength=n).gather(0, i2)
    w1 = (c1.double() ** n_lambda + 1e-6) ** (-1) * frac1
    w2 = (c2.double() ** n_lambda + 1e-6) ** (-1) * frac2
    l1, l2 = (1 - e1 * w1).mean(), (1 - e2 * w2).mean()
    return float((l1 + l2) / 2), float(l1), float(l2), c1.numpy(), c2.numpy()


@pytest.mark.parametrize("kind", D.KINDS)
def test_the_restatement_agrees_with_the_published_formulation(kind):
    worst = 0.0
    for n, m in SHAPES:
        for alpha in (1.0, 40.0, 1000.0):
            for n_lambda in (0.0, 0.5, 1.0, 2.0):
                for non_reg in (False, True):
                    case = D.make(kind, n, m, 17 * n + m)
                    got = D.dcd(*case, alpha=alpha, n_lambda=n_lambda, non_reg=non_reg)
                    loss, l1, l2, c1, c2 = published(*case, alpha, n_lambda, non_reg)
                    assert got["status"] == 0 and np.array_equal(got["count1"], c1) and np.array_equal(got["count2"], c2)
                    scale = max(1.0, n / m, m / n)
                    dev = max(abs(got["loss"] - loss), abs(got["halves"][0] - l1), abs(got["halves"][1] - l2)) / scale
                    worst = max(worst, dev)
                    # another order of the same sum and a reciprocal for a division: well inside the bound between two libraries
                    assert dev <= D.dcd_bound(n, m), (kind, n, m, alpha, n_lambda, non_reg, dev)
    print("%-6s worst deviation from the published formulation %.3g (DCD_BOUND %.3g)" % (kind, worst, D.DCD_BOUND))


def test_the_coefficient_is_the_gradient_of_the_published_loss_with_detached_weights():
    torch = pytest.importorskip("torch")
    n, m, alpha = 300, 200, 40.0
    d1, i1, d2, i2 = D.make("random", n, m, 3)
    got = D.dcd(d1, i1, d2, i2, alpha=alpha, n_lambda=0.5)
    t1, t2 = (torch.from_numpy(d.astype(np.float64)).requires_grad_(True) for d in (d1, d2))
    w1 = torch.from_numpy((n / m) / (D.counts(i1, m).astype(np.float64) ** 0.5 + 1e-6))
    w2 = torch.from_numpy((m / n) / (D.counts(i2, n).astype(np.float64) ** 0.5 + 1e-6))
    (((1 - torch.exp(-alpha * t1) * w1).mean() + (1 - torch.exp(-alpha * t2) * w2).mean()) / 2).backward()
    for coef, t in ((got["coef1"], t1), (got["coef2"], t2)):
        assert coef.dtype == np.float32
        assert (np.abs(coef.astype(np.float64) - t.grad.numpy()) <= 2.0 ** -23 * np.abs(t.grad.numpy()) + 2.0 ** -149).all()


def test_two_queries_on_one_target():
    d = np.zeros(2, dtype=np.float32)
    got = D.dcd(d, np.array([1, 1]), d, np.array([0, 1]), alpha=1000.0)
    assert got["count1"].tolist() == [2, 2] and got["count2"].tolist() == [1, 1]
    assert got["halves"][0] == 1.0 - 1.0 / (2.0 + 1e-6) and got["halves"][1] == 1.0 - 1.0 / (1.0 + 1e-6)
    assert got["loss"] == 0.5 * (got["halves"][0] + got["halves"][1])
    assert got["coef1"][0] == np.float32((0.5 * 1000.0) / 2.0 * (1.0 / (2.0 + 1e-6)))


def test_a_permutation_counts_one_everywhere_and_identical_clouds_give_the_floor():
    rng = np.random.default_rng(0)
    n = 300
    perm = rng.permutation(n).astype(np.int32)
    d = rng.uniform(0, 0.01, n).astype(np.float32)
    got = D.dcd(d, perm, d, np.argsort(perm).astype(np.int32), alpha=40.0)
    assert (got["count1"] == 1).all() and (got["count2"] == 1).all()
    same = D.dcd(np.zeros(n, np.float32), np.arange(n), np.zeros(n, np.float32), np.arange(n))
    floor = 1.0 - 1.0 / (1.0 + 1e-6)
    assert abs(same["loss"] - floor) <= 4 * D.U and same["loss"] > 0
    # every term is the same value v, so the tree returns 256 v per block exactly and the block order adds 256 v + 44 v
    v = np.float64(1.0) - np.float64(1.0) / (np.float64(1.0) + np.float64(1e-6))
    assert same["halves"][0] == (256 * v + 44 * v) / 300


def test_unequal_sizes_with_and_without_non_reg():
    n, m = 513, 100
    case = D.make("random", n, m, 5)
    free, clamped = D.dcd(*case, alpha=40.0), D.dcd(*case, alpha=40.0, non_reg=True)
    assert free["halves"][0] == clamped["halves"][0]                                        # n / m > 1: the clamp leaves side 1 alone
    assert clamped["halves"][1] < free["halves"][1]                                         # m / n < 1 became 1: larger weights
    # side 2 alone, by hand
    d2, i2 = case[2], case[3]
    c2 = D.counts(i2, n).astype(np.float64)
    for non_reg, r in ((False, free), (True, clamped)):
        frac = max(1.0, m / n) if non_reg else m / n
        terms = 1.0 - np.exp(-(40.0 * d2.astype(np.float64))) * (frac / (c2 + 1e-6))
        assert r["halves"][1] == D.tree_sum(terms) / m
    # a heavily weighted side goes below zero: frac 5 against counts of 1 and distances of 0
    assert D.dcd(np.zeros(500, np.float32), np.arange(500) % m, np.zeros(m, np.float32), np.arange(m), alpha=1.0, n_lambda=0.0)["halves"][0] < -1


@pytest.mark.parametrize("n_lambda", [0.0, 0.5, 1.0, 2.0])
def test_the_count_exponent(n_lambda):
    n, m = 257, 64
    case = D.make("random", n, m, 11)
    got = D.dcd(*case, alpha=40.0, n_lambda=n_lambda)
    c1 = D.counts(case[1], m).astype(np.float64)
    p = {0.0: np.ones(n), 0.5: np.sqrt(c1), 1.0: c1, 2.0: c1 * c1}[n_lambda]
    terms = 1.0 - np.exp(-(40.0 * case[0].astype(np.float64))) * ((n / m) / (p + 1e-6))
    assert abs(got["halves"][0] - D.tree_sum(terms) / n) <= D.dcd_bound(n, m) * (n / m)
    if n_lambda in (0.0, 1.0):
        assert got["halves"][0] == D.tree_sum(terms) / n                                     # no pow: the same bits
    if n_lambda == 0.0:
        assert got["halves"][0] == D.dcd(case[0], np.zeros(n, np.int32), case[2], case[3], alpha=40.0, n_lambda=0.0)["halves"][0]


def test_the_tree_and_the_block_order_on_257_hand_made_terms():
    """Block 0 is a tree over 256 terms, block 1 holds one term and 255 zeros, block 0's sum comes first.  2^53, 1, 1, ... tells the
    tree from a running sum: ascending addition loses every 1, the tree keeps the pairs it adds first."""
    x = np.ones(257)
    x[0] = 2.0 ** 53
    got = D.tree_sum(x)
    blocks = x[:256].copy()
    for stride in (128, 64, 32, 16, 8, 4, 2, 1):
        for i in range(stride):
            blocks[i] = blocks[i] + blocks[i + stride]
    assert got == blocks[0] + 1.0
    running = 0.0
    for v in x:
        running = running + v
    assert running == 2.0 ** 53 and got > running + 200
    # the block order: three blocks whose sums are 2^53, 1, 1 -- ascending loses both ones, any other order keeps them
    y = np.zeros(513)
    y[0], y[256], y[512] = 2.0 ** 53, 1.0, 1.0
    assert D.tree_sum(y) == 2.0 ** 53 and D.tree_sum(y[::-1]) == 2.0 ** 53 + 2.0
    assert D.tree_sum(np.array([3.5])) == 3.5 and D.tree_sum(np.array([-0.0])) == 0.0


def test_an_index_outside_its_target_set_refuses_the_cloud():
    n, m = 40, 30
    d1, i1, d2, i2 = D.make("random", n, m, 2)
    clean = D.dcd(d1, i1, d2, i2)
    for which, value in ((1, m), (1, -1), (3, n), (3, -5), (1, 2 ** 31 - 1)):
        case = [d1, i1.copy(), d2, i2.copy()]
        case[which][7] = value
        r = D.dcd(*case)
        assert r["status"] == D.REFUSED and np.isnan(r["loss"]) and np.isnan(r["halves"]).all()
        assert (r["count1"] == -1).all() and (r["count2"] == -1).all() and np.isnan(r["coef1"]).all() and np.isnan(r["coef2"]).all()
    edge = [d1, i1.copy(), d2, i2.copy()]
    edge[1][7], edge[3][7] = m - 1, n - 1                                                    # the last valid index is served
    assert D.dcd(*edge)["status"] == 0
    assert D.dcd(d1, i1, d2, i2)["loss"] == clean["loss"]
    # distances that are negative or not finite are not refused: they go through the arithmetic
    odd = d1.copy()
    odd[3], odd[4] = np.nan, -1.0
    r = D.dcd(odd, i1, d2, i2, alpha=1.0)
    assert r["status"] == 0 and np.isnan(r["loss"]) and np.isnan(r["coef1"][3]) and r["coef1"][4] > 0 and not np.isnan(r["halves"][1])
    inf = d1.copy()
    inf[3] = np.inf
    r = D.dcd(inf, i1, d2, i2)
    assert r["status"] == 0 and np.isfinite(r["loss"]) and r["coef1"][3] == 0.0


def test_the_bound_grows_with_the_depth_and_the_blocks_only():
    assert D.dcd_bound(1, 1) == 22 * D.U and D.dcd_bound(256, 3) == (20 + 2 * (8 + 1)) * D.U
    assert D.dcd_bound(257, 513) == (20 + 2 * (10 + 3)) * D.U
    assert D.DCD_BOUND == D.dcd_bound(D.LDS_TARGETS + 1, 1) == (20 + 2 * (16 + 129)) * D.U < 4e-14


# ---- dispatch.h, the build, the package ---------------------------------------------------------------------------------------------------
def test_dcd_form_is_pure_and_picks_as_expected(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    cap = D.LDS_TARGETS
    asks = [(1, 1, 1, 0), (32, 2048, 2048, 0), (50, 2500, 2500, 0), (1, cap, cap, 0), (1, cap + 1, cap, 0), (1, cap, cap + 1, 0),
            (1, cap, cap, 1), (1, cap + 1, 5, 1), (1, 5, cap + 1, 1), (1, cap + 1, cap + 1, 2), (3, 257, 513, 2), (3, 257, 513, 1),
            (0, 4, 4, 0), (-1, 4, 4, 0), (1, 0, 4, 0), (1, 4, 0, 0), (1, 4, 4, 3), (1, 4, 4, -1)]
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include "dispatch.h"\nint main(int argc, char **argv) {\n'
                   ' for (int a = 1; a + 3 < argc; a += 4) { int v[4]; for (int k = 0; k < 4; ++k) v[k] = atoi(argv[a + k]);\n'
                   '  auto f = dispatch::dcd_form(v[0], v[1], v[2], v[3]), g = dispatch::dcd_form(v[0], v[1], v[2], v[3]);\n'
                   '  if (f.kernel != g.kernel || f.blocks1 != g.blocks1 || f.blocks2 != g.blocks2 || f.launches != g.launches) return 1;\n'
                   '  std::printf("%s %ld %ld %d\\n", f.kernel == dispatch::DCDKernel::Lds ? "lds" : f.kernel == dispatch::DCDKernel::Workspace ?'
                   ' "workspace" : "unserved", f.blocks1, f.blocks2, f.launches); }\n'
                   ' std::printf("%d %d %d\\n", dispatch::DCD_BLOCK, dispatch::DCD_LDS_THREADS, dispatch::DCD_LDS_TARGETS); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "dpf_nets_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    out = subprocess.run([str(exe)] + [str(x) for a in asks for x in a], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    assert [int(t) for t in out[-1].split()] == [D.BLOCK, 1024, cap]
    assert cap * 4 + 1024 * 8 <= 160 * 1024                                                  # the histogram and the tree: the workgroup's LDS
    want = []
    for B, n, m, force in asks:
        if B < 0 or n < 1 or m < 1 or force not in (0, 1, 2) or (force == 1 and max(n, m) > cap):
            want.append("unserved 0 0 0")
            continue
        lds = force == 1 or (force == 0 and max(n, m) <= cap)
        want.append("%s %d %d %d" % ("lds" if lds else "workspace", (n + 255) // 256, (m + 255) // 256, 1 if lds else 4))
    assert out[:-1] == want
    assert out[3].startswith("lds") and out[4].startswith("workspace") and out[5].startswith("workspace")     # the cap and cap + 1


def test_make_builds_dcd_o_through_the_one_rule():
    csrc = os.path.join(ROOT, "dpf_nets_amd", "csrc")
    r = subprocess.run(["make", "-n", "-B", "-C", csrc, "dcd.o"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    cmds = [ln.split() for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("make")]
    assert len(cmds) == 3, cmds
    listing, gate, obj = cmds
    assert listing[-3:] == ["dcd.hip", "-o", "dcd.s"] and "-S" in listing and "-ffp-contract=off" in listing
    assert gate[1].endswith("mfma_overlap_check.py") and gate[-1] == "dcd.s" and "--no-scratch" not in gate
    assert obj[-3:] == ["dcd.hip", "-o", "dcd.o"] and "-ffp-contract=off" in obj
    assert set(listing[:-2]) - {"-S", "--cuda-device-only"} == set(obj[:-2]) - {"-c"}
    link = subprocess.run(["make", "-n", "-B", "-C", csrc], capture_output=True, text=True, timeout=60).stdout
    assert any("-shared" in ln and " dcd.o" in ln for ln in link.splitlines())


def test_the_header_declares_what_the_package_binds():
    from dpf_nets_amd import _lib
    text = open(os.path.join(ROOT, "include", "dpf_hip.h")).read()
    assert "int dpf_dcd(int B, int n, int m," in text and "size_t dpf_dcd_workspace_bytes(int B, int n, int m);" in text
    assert len(_lib.SIGNATURES["dpf_dcd"][1]) == 21 and len(_lib.SIGNATURES["dpf_dcd_workspace_bytes"][1]) == 3


def test_cpu_tensors_and_bad_arguments_are_refused_without_a_gpu():
    torch = pytest.importorskip("torch")
    from dpf_nets_amd import metrics
    from dpf_nets_amd.metrics import density_aware_chamfer, density_aware_chamfer_raw, pairwise_DCD
    assert metrics.density_aware_chamfer is density_aware_chamfer
    a, b = torch.randn(2, 40, 3), torch.randn(2, 50, 3)
    for call in (lambda: density_aware_chamfer(a, b), lambda: density_aware_chamfer(a.double(), b), lambda: density_aware_chamfer(a[0], b[0]),
                 lambda: pairwise_DCD(a, b, 4),
                 lambda: density_aware_chamfer_raw(torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")), dict(alpha=float("nan")), dict(n_lambda=-0.5),
               dict(n_lambda=float("inf")), dict(n_lambda=float("nan"))):
        with pytest.raises(ValueError, match="alpha|n_lambda"):
            density_aware_chamfer(a, b, **kw)
        with pytest.raises(ValueError, match="alpha|n_lambda"):
            density_aware_chamfer_raw(None, None, None, None, **kw)
    with pytest.raises(ValueError, match="bs"):
        pairwise_DCD(a, b, 0)


def test_compute_all_metrics_dcd_keys_on_stubs(monkeypatch):
    """the swd= branch's orientation: (reference, sample) transposed for lgan_mmd_cov, (rr, rs, ss) for the 1-NN test; dcd=None adds nothing"""
    torch = pytest.importorskip("torch")
    from dpf_nets_amd.metrics import evaluation_metrics as E
    from dpf_nets_amd.metrics import dcd as dcd_module
    g = torch.Generator().manual_seed(0)
    ns, nr = 7, 9
    fx = {"rs": torch.rand(nr, ns, generator=g), "rr": torch.rand(nr, nr, generator=g), "ss": torch.rand(ns, ns, generator=g)}
    fx["rr"], fx["ss"] = fx["rr"] + fx["rr"].t(), fx["ss"] + fx["ss"].t()
    sample, ref = torch.zeros(ns, 4, 3), torch.zeros(nr, 4, 3)
    lookup = {(id(ref), id(sample)): "rs", (id(ref), id(ref)): "rr", (id(sample), id(sample)): "ss"}
    calls = []

    def matrices(metric):
        def fn(a, b, bs=None, shard_rows=False, **kw):
            which = lookup[(id(a), id(b))]                 # (a KeyError here: a matrix in the wrong orientation)
            calls.append((metric, which, bs, tuple(sorted(kw.items()))))
            return fx[which] * (1.0 if metric == "dcd" else 2.0)
        return fn

    monkeypatch.setattr(E, "pairwise_CD", matrices("cd"))
    monkeypatch.setattr(E, "pairwise_EMD", matrices("emd"))
    monkeypatch.setattr(dcd_module, "pairwise_DCD", matrices("dcd"))
    base = E.compute_all_metrics(sample, ref, 5)
    assert not any("DCD" in k for k in base) and not any(c[0] == "dcd" for c in calls)
    got = E.compute_all_metrics(sample, ref, 5, dcd=40.0)
    new = ["lgan_mmd-DCD", "lgan_cov-DCD", "lgan_mmd_smp-DCD", "1-NN-DCD-acc_t", "1-NN-DCD-acc_f", "1-NN-DCD-acc"]
    assert list(got.keys()) == list(base.keys()) + new
    assert all(torch.equal(got[k], base[k]) for k in base)
    assert sorted(c for c in calls if c[0] == "dcd") == sorted(("dcd", w, 5, (("alpha", 40.0),)) for w in ("rs", "rr", "ss"))
    want = {"%s-DCD" % k: v for k, v in E.lgan_mmd_cov(fx["rs"].t()).items()}
    want.update({"1-NN-DCD-%s" % k: v for k, v in E.knn(fx["rr"], fx["rs"], fx["ss"], 1).items() if "acc" in k})
    assert all(torch.equal(got[k], want[k]) for k in new)
    for bad in (0, -1.0, float("inf"), float("nan"), True, "40"):
        with pytest.raises(ValueError, match="dcd"):
            E.compute_all_metrics(sample, ref, 5, dcd=bad)
