"""dpf_swd_* on the GPU against the numpy restatement of the contract (tests/swd_ref.py; the restatement itself is checked against a
float64 path in tests/test_swd_ref_cpu.py).  The tables are bit-defined: sorted, order and status are compared for EQUALITY.  The pair
sums are float64 sums of the same non-negative terms in an order the kernel chooses, so kernel and restatement are each within
L * n * 2^-53 relative of the exact sum; they are held to 2^-40 relative of each other.  The fp32 distance is one further rounding of
the float64 quotient: within 1 ulp.  The gradient is held to 1 ulp of the restatement's plus 2^-40 of its float64 sum of magnitudes.
A table's reference is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import swd_ref as R                                                                          # noqa: E402
from test_swd_ref_cpu import f64_path                                                        # noqa: E402

pytestmark = pytest.mark.gpu

NMAX = 8192
FORMS = {1: 512, 2: NMAX, 3: NMAX}                  # forced form -> the largest cloud it serves
REL = 2.0 ** -40
SENT_F, SENT_I, GUARD = -12345.5, -7777, 256
_REF = {}


def dev():
    return torch.device("cuda", 0)


def S():
    from dpf_nets_amd.metrics import sliced
    return sliced


def lib():
    from dpf_nets_amd import _lib
    return _lib


def serving(n):
    return [f for f, limit in FORMS.items() if n <= limit]


def dirs_for(kind, L, seed=0):
    return R.make_dirs({"lattice": "axis", "negzero": "negzero"}.get(kind, "gauss"), L, seed)


def ref(kind, n, seed, L, dseed=0):
    """the reference tables of one cloud under its kind's first L directions, cached"""
    key = (kind, n, seed, L, dseed)
    if key not in _REF:
        _REF[key] = R.tables(R.make_cloud(kind, n, seed), dirs_for(kind, L, dseed))
    return _REF[key]


def run(pts, dirs, form=0, channels_first=False, order=True):
    t = torch.from_numpy(pts).to(dev()) if isinstance(pts, np.ndarray) else pts
    d = torch.from_numpy(dirs).to(dev()) if isinstance(dirs, np.ndarray) else dirs
    out = S().sliced_tables(t, d, channels_first, order, form)
    return tuple(o.cpu().numpy() for o in out)


def raw(v):
    return np.ascontiguousarray(v).view(np.uint8)


def same_bits(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(raw(g), raw(w))
                                         for g, w in zip(got, want))


def stack(refs):
    return (np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs]), np.array([r[2] for r in refs], dtype=np.int32))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


EDGES = (1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 1000, 1024, 1025, 4096, 4097, 8191, 8192)


@pytest.mark.parametrize("n", EDGES)
def test_tables_at_the_kernel_edges_every_form(n):
    kinds = ("gauss", "lattice", "wide")
    pts = np.stack([R.make_cloud(kd, n, n + i) for i, kd in enumerate(kinds)])
    dirs = R.make_dirs("gauss", 5, n)
    dirs[3] = (0.0, -1.0, 0.0)                                                              # an axis: the lattice cloud ties in whole runs
    full = [R.tables(p, dirs) for p in pts]
    for form in [0] + serving(n):
        for L in (1, 2, 5):
            for B in (1, 3):
                want = stack([(f[0][:L], f[1][:L], f[2]) for f in full[:B]])
                got = run(pts[:B], dirs[:L], form)
                assert same_bits(got, want), (n, form, L, B)


@pytest.mark.parametrize("n", (65, 300, 1500))
@pytest.mark.parametrize("kind", R.KINDS)
def test_cloud_kinds(kind, n):
    L = 6 if kind == "lattice" else 3
    pts = R.make_cloud(kind, n, 7)[None]
    want = stack([ref(kind, n, 7, L)])
    assert want[2][0] == 0
    if kind == "same":
        assert (want[1] == np.arange(n)).all()
    if kind in ("lattice", "negzero"):
        assert not (want[0].view(np.uint32) == 0x80000000).any()
        assert (np.diff(want[0], axis=2) == 0).mean() > 0.5                                 # ties fill whole runs
    for form in [0] + serving(n):
        assert same_bits(run(pts, dirs_for(kind, L), form), want), (kind, n, form)


def test_refusals_touch_no_other_cloud():
    n, L = 130, 4
    dirs = R.make_dirs("gauss", L)
    dirs[2] = (1.0, 1.0, 1.0)
    good = [R.make_cloud("gauss", n, 50 + i) for i in range(3)]
    nan_c, inf_c, big_c = good[0].copy(), good[1].copy(), good[2].copy()
    nan_c[n - 1, 2] = np.nan
    inf_c[0, 0] = -np.inf
    big_c[64] = np.float32(3e38)                                                            # finite; overflows on direction 2 only
    batch = np.stack([good[0], nan_c, good[1], inf_c, big_c, good[2]])
    want = stack([R.tables(c, dirs) for c in batch])
    assert want[2].tolist() == [0, -1, 0, -1, -1, 0]
    for form in [0] + serving(n):
        got = run(batch, dirs, form)
        assert same_bits(got, want), form
        for i, b in enumerate((0, 2, 5)):
            assert same_bits(run(good[i][None], dirs, form), tuple(g[b:b + 1] for g in got)), (form, b)
    bad_dirs = dirs.copy()
    bad_dirs[1, 1] = np.nan
    got = run(np.stack(good), bad_dirs)
    assert (got[2] == -1).all() and np.isnan(got[0]).all() and (got[1] == -1).all()
    big_dirs = dirs.copy()
    big_dirs[0] = np.float32(1e38)                                                          # per cloud: refused where |x| * 1e38 overflows
    mixed = np.stack([good[0] * np.float32(0.01), good[1], good[2] * np.float32(0.01)])
    want = stack([R.tables(c, big_dirs) for c in mixed])
    assert want[2].tolist() == [0, -1, 0] and same_bits(run(mixed, big_dirs), want)
    tiny = np.stack([c * np.float32(0.1) for c in good])                                    # the largest coordinate times the largest
    big_dirs[0] = (3e38, 0.0, 0.0)                                                          # component passes 2^125, yet every
    assert np.abs(tiny).max() * 3e38 >= 2.0 ** 125                                          # projection is finite: accepted
    want = stack([R.tables(c, big_dirs) for c in tiny])
    assert (want[2] == 0).all() and same_bits(run(tiny, big_dirs), want)


def test_layouts_strides_and_a_broadcast_cloud():
    n, L, B = 333, 3, 3
    dirs = R.make_dirs("gauss", L)
    pts = np.stack([R.make_cloud("gauss", n, 40 + b) for b in range(B)])
    want = stack([ref("gauss", n, 40 + b, L) for b in range(B)])
    t = torch.from_numpy(pts).to(dev())
    assert same_bits(run(t, dirs), want)
    cf = t.transpose(1, 2).contiguous()
    assert same_bits(run(cf, dirs, channels_first=True), want)
    assert same_bits(run(t.transpose(1, 2), dirs, channels_first=True), want)
    big = torch.full((2 * B + 1, n + 9, 5), float("nan"), device=dev())                     # anything read outside the slice would refuse
    view = big[1::2, 4:4 + n, 1:4]
    view.copy_(t)
    assert not view.is_contiguous() and same_bits(run(view, dirs), want)
    bigc = torch.full((B + 2, 3, 2 * n + 6), float("nan"), device=dev())
    viewc = bigc[1:1 + B, :, 3:3 + 2 * n:2]
    viewc.copy_(cf)
    assert same_bits(run(viewc, dirs, channels_first=True), want)
    one = t[1:2].expand(4, n, 3)
    assert one.stride(0) == 0
    assert same_bits(run(one, dirs), stack([ref("gauss", n, 41, L)] * 4))


def test_guards_a_null_order_and_repeat_runs():
    n, L, B = 257, 3, 2
    dirs = torch.from_numpy(R.make_dirs("gauss", L)).to(dev())
    pts = torch.from_numpy(np.stack([R.make_cloud("gauss", n, 60 + b) for b in range(B)])).to(dev())
    want = stack([ref("gauss", n, 60 + b, L) for b in range(B)])
    for form in [0] + serving(n):
        for with_order in (True, False):
            so = torch.full((B * L * n + 2 * GUARD,), SENT_F, device=dev())
            od = torch.full((B * L * n + 2 * GUARD,), SENT_I, dtype=torch.int32, device=dev())
            st = torch.full((B + 2 * GUARD,), SENT_I, dtype=torch.int32, device=dev())
            rc = lib().lib().dpf_swd_tables(B, n, pts.data_ptr(), 3 * n, 3, 1, L, dirs.data_ptr(), form, so[GUARD:].data_ptr(),
                                            od[GUARD:].data_ptr() if with_order else None, st[GUARD:].data_ptr(),
                                            lib().current_stream())
            assert rc == 0
            torch.cuda.synchronize()
            for buf, sent, size in ((so, SENT_F, B * L * n), (od, SENT_I, B * L * n), (st, SENT_I, B)):
                assert (buf[:GUARD] == sent).all() and (buf[GUARD + size:] == sent).all()
            assert np.array_equal(raw(so[GUARD:GUARD + B * L * n].cpu().numpy().reshape(B, L, n)), raw(want[0]))
            assert np.array_equal(st[GUARD:GUARD + B].cpu().numpy(), want[2])
            if with_order:
                assert np.array_equal(od[GUARD:GUARD + B * L * n].cpu().numpy().reshape(B, L, n), want[1])
            else:
                assert (od == SENT_I).all()
    first = run(pts, dirs)
    assert all(same_bits(run(pts, dirs), first) for _ in range(3))
    assert same_bits(run(pts, dirs, order=False), (first[0], first[2]))


def test_arguments():
    f = lib().lib()
    n, L = 8, 2
    x = torch.zeros((1, n, 3), device=dev())
    d = torch.from_numpy(R.make_dirs("gauss", L)).to(dev())
    so = torch.empty((1, L, n), device=dev())
    st = torch.empty((1,), dtype=torch.int32, device=dev())
    s = lib().current_stream()

    def call(B=1, n=n, xyz=x.data_ptr(), L=L, dirs=d.data_ptr(), form=0, sorted_=so.data_ptr()):
        return f.dpf_swd_tables(B, n, xyz, 3 * n, 3, 1, L, dirs, form, sorted_, None, st.data_ptr(), s)
    assert call() == 0
    assert f.dpf_swd_max_points() == NMAX
    for kw in (dict(B=-1), dict(n=0), dict(L=0), dict(xyz=None), dict(dirs=None), dict(sorted_=None), dict(form=4), dict(form=-1),
               dict(B=2 ** 30, L=2)):
        assert call(**kw) == -1, kw
    assert call(n=NMAX + 1) == -2 and call(n=600, form=1) == -2
    assert call(B=0, xyz=None, sorted_=None) == 0
    torch.cuda.synchronize()


def test_seventy_thousand_sorts_for_the_grid_limits():
    n, L, B = 8, 7, 10000
    rng = np.random.default_rng(5)
    pts = rng.integers(-3, 4, size=(B, n, 3)).astype(np.float32)
    dirs = R.make_dirs("dyadic", L)
    p = ((pts[:, None, :, 0] * dirs[None, :, None, 0] + pts[:, None, :, 1] * dirs[None, :, None, 1])
         + pts[:, None, :, 2] * dirs[None, :, None, 2]) + np.float32(0.0)                   # (B, L, n), exact
    order = np.argsort(p, axis=2, kind="stable").astype(np.int32)
    want = (np.take_along_axis(p, order.astype(np.int64), axis=2), order, np.zeros((B,), dtype=np.int32))
    for b in (0, B - 1):
        assert same_bits(tuple(w[b] for w in want[:2]), R.tables(pts[b], dirs)[:2])
    assert same_bits(run(pts, dirs), want)


# ---- pair sums --------------------------------------------------------------------------------------------------------------------
def tables_of(clouds, dirs, order=False):
    return S().sliced_tables(torch.from_numpy(clouds).to(dev()), torch.from_numpy(dirs).to(dev()), False, order)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    print(what, "largest relative error", (err / np.maximum(np.abs(want[ok]), 1e-300)).max() if ok.any() else 0.0)
    assert (err <= REL * np.abs(want[ok])).all(), what


@pytest.mark.parametrize("n,L", [(1, 1), (65, 5), (1025, 5), (8192, 2)])
def test_pair_sums_and_the_distance(n, L):
    B = 4
    dirs = R.make_dirs("gauss", L, n)
    a = np.stack([R.make_cloud("gauss", n, 100 + b) for b in range(B)])
    b_ = np.stack([R.make_cloud("wide" if b == 3 else "gauss", n, 200 + b) for b in range(B)])
    b_[2, n // 2, 0] = np.nan                                                               # a refused side: NaN for that pair only
    sa, sta = tables_of(a, dirs)
    sb, stb = tables_of(b_, dirs)
    ra, rb = stack([R.tables(c, dirs) for c in a]), stack([R.tables(c, dirs) for c in b_])
    assert same_bits((sa.cpu().numpy(), sta.cpu().numpy()), (ra[0], ra[2]))
    want = np.array([R.sumsq(ra[0][i], rb[0][i], ra[2][i] != 0 or rb[2][i] != 0) for i in range(B)])
    assert np.isnan(want).tolist() == [False, False, True, False]
    got = S().sliced_pair_sums(sa, sta, sb, stb).cpu().numpy()
    assert got.dtype == np.float64
    close(got, want, "pairs")
    again = S().sliced_pair_sums(sa, sta, sb, stb).cpu().numpy()
    assert np.array_equal(raw(got), raw(again))
    one = S().sliced_pair_sums(sa[1:2], sta[1:2], sb, stb).cpu().numpy()                    # a_stride = 0
    close(one, [R.sumsq(ra[0][1], rb[0][i], rb[2][i] != 0) for i in range(B)], "broadcast")
    x, y = torch.from_numpy(a[:2]).to(dev()), torch.from_numpy(b_[:2]).to(dev())
    dist = S().sliced_wasserstein(x, y, torch.from_numpy(dirs).to(dev())).cpu().numpy()
    assert dist.dtype == np.float32
    ref_d = np.array([R.distance(want[i], L, n) for i in range(2)])
    assert (np.abs(dist.astype(np.float64) - ref_d.astype(np.float64)) <= ulp32(ref_d)).all()


@pytest.mark.parametrize("N1,N2", [(5, 7), (17, 9), (70, 33)])
def test_the_matrix_against_the_batched_entry(N1, N2):
    n, L = 130, 5
    dirs = R.make_dirs("gauss", L, N1)
    c1 = np.stack([R.make_cloud("gauss", n, 300 + i) for i in range(N1)])
    c2 = np.stack([R.make_cloud("gauss", n, 400 + j) for j in range(N2)])
    c1[3, 0, 0] = np.inf                                                                    # NaN in row 3 only
    c2[N2 - 1, 5, 1] = np.nan                                                               # and in the last column only
    s1, st1 = tables_of(c1, dirs)
    s2, st2 = tables_of(c2, dirs)
    M = S().sliced_matrix_sums(s1, st1, s2, st2).cpu().numpy()
    nan = np.isnan(M)
    assert nan[3].all() and nan[:, N2 - 1].all() and nan.sum() == N1 + N2 - 1
    ii, jj = np.meshgrid(np.arange(N1), np.arange(N2), indexing="ij")
    ii, jj = torch.from_numpy(ii.ravel()).to(dev()), torch.from_numpy(jj.ravel()).to(dev())
    batched = S().sliced_pair_sums(s1[ii].contiguous(), st1[ii].contiguous(), s2[jj].contiguous(), st2[jj].contiguous())
    close(M, batched.cpu().numpy().reshape(N1, N2), "matrix vs pairs")
    r1, r2 = stack([R.tables(c, dirs) for c in c1]), stack([R.tables(c, dirs) for c in c2])
    want = np.array([[R.sumsq(r1[0][i], r2[0][j], r1[2][i] != 0 or r2[2][j] != 0) for j in range(N2)] for i in range(N1)])
    close(M, want, "matrix vs restatement")
    # two direction chunks with accumulate = 1 against one call over all directions
    acc = torch.full((N1, N2), -5.0, dtype=torch.float64, device=dev())
    S().sliced_matrix_sums(s1[:, :2].contiguous(), st1, s2[:, :2].contiguous(), st2, out=acc, accumulate=False)
    S().sliced_matrix_sums(s1[:, 2:].contiguous(), st1, s2[:, 2:].contiguous(), st2, out=acc, accumulate=True)
    close(acc.cpu().numpy(), M, "two chunks")
    pacc = torch.zeros((N1 * N2,), dtype=torch.float64, device=dev())
    for lo, hi in ((0, 2), (2, L)):
        S().sliced_pair_sums(s1[ii][:, lo:hi].contiguous(), st1[ii].contiguous(), s2[jj][:, lo:hi].contiguous(), st2[jj].contiguous(),
                             out=pacc, accumulate=lo > 0)
    close(pacc.cpu().numpy().reshape(N1, N2), M, "pairs, two chunks")
    D = S().pairwise_SWD(torch.from_numpy(c1).to(dev()), torch.from_numpy(c2).to(dev()), torch.from_numpy(dirs).to(dev()), dir_chunk=2)
    ok = ~nan
    ref_d = (want / (L * n)).astype(np.float32)
    assert D.dtype == torch.float32 and tuple(D.shape) == (N1, N2)
    D = D.cpu().numpy()
    assert np.array_equal(np.isnan(D), nan) and (np.abs(D[ok].astype(np.float64) - ref_d[ok]) <= ulp32(ref_d[ok])).all()


def test_one_direction_on_a_lattice_is_an_exact_integer():
    n = 1000
    a, b = R.make_cloud("lattice", n, 20), R.make_cloud("lattice", n, 21)
    dirs = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)
    want = int(((np.sort(a[:, 0].astype(np.int64)) - np.sort(b[:, 0].astype(np.int64))) ** 2).sum())
    sa, sta = tables_of(a[None], dirs)
    sb, stb = tables_of(b[None], dirs)
    assert float(S().sliced_pair_sums(sa, sta, sb, stb)[0]) == want
    assert float(S().sliced_matrix_sums(sa, sta, sb, stb)[0, 0]) == want
    d = S().sliced_wasserstein(torch.from_numpy(a[None]).to(dev()), torch.from_numpy(b[None]).to(dev()), torch.from_numpy(dirs).to(dev()))
    assert float(d[0]) == float(np.float32(want / n))


# ---- gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 65, 1025))
@pytest.mark.parametrize("L", (1, 5))
def test_gradient_against_the_restatement(n, L):
    B = 3
    dirs = R.make_dirs("gauss", L, n)
    a = np.stack([R.make_cloud("gauss", n, 500 + b) for b in range(B)])
    b_ = np.stack([R.make_cloud("gauss", n, 600 + b) for b in range(B)])
    b_[1, 0, 0] = np.nan                                                                    # a refused pair: gradient 0
    gc = np.array([1.5, -2.0, 0.25], dtype=np.float32)
    ta, tb = tables_of(a, dirs, True), tables_of(b_, dirs, True)
    ra, rb = [R.tables(c, dirs) for c in a], [R.tables(c, dirs) for c in b_]
    want = [R.grad(ra[i], rb[i], dirs, gc[i]) for i in range(B)]
    d = torch.from_numpy(dirs).to(dev())
    g = torch.from_numpy(gc).to(dev())
    both = S().sliced_grad(d, ta, tb, g, True, True)
    only_a = S().sliced_grad(d, ta, tb, g, True, False)
    only_b = S().sliced_grad(d, ta, tb, g, False, True)
    assert only_a[1] is None and only_b[0] is None
    assert torch.equal(both[0], only_a[0]) and torch.equal(both[1], only_b[1])
    again = S().sliced_grad(d, ta, tb, g, True, True)
    assert np.array_equal(raw(both[0].cpu().numpy()), raw(again[0].cpu().numpy()))
    assert np.array_equal(raw(both[1].cpu().numpy()), raw(again[1].cpu().numpy()))
    for side in (0, 1):
        got = both[side].cpu().numpy().astype(np.float64)
        for i in range(B):
            w, bound = want[i][side], want[i][2 + side]
            allowed = ulp32(w) + REL * (2.0 / (L * n)) * abs(float(gc[i])) * bound
            err = np.abs(got[i] - w.astype(np.float64))
            print("grad side", side, "pair", i, "largest error / allowed", (err / np.maximum(allowed, 1e-300)).max())
            assert (err <= allowed).all(), (side, i)
        assert (got[1] == 0).all()


def test_backward_against_float64_autograd_and_x_against_itself():
    n, L = 257, 5
    dirs = R.make_dirs("gauss", L, 9)
    a, b = R.make_cloud("gauss", n, 700), R.make_cloud("gauss", n, 701)
    dist, _, foa, _, fob, ga, gb = f64_path(a, b, dirs)
    ra, rb = R.tables(a, dirs), R.tables(b, dirs)
    assert np.array_equal(ra[1], foa) and np.array_equal(rb[1], fob)                        # (tie-free: fp32 and float64 orders agree)
    d = torch.from_numpy(dirs).to(dev())
    for cf in (False, True):
        x = torch.from_numpy(a[None]).to(dev())
        y = torch.from_numpy(b[None]).to(dev())
        if cf:
            x, y = x.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous()
        x.requires_grad_(True)
        y.requires_grad_(True)
        out = S().sliced_wasserstein(x, y, d, channels_first=cf)
        out.sum().backward()
        gx, gy = x.grad, y.grad
        if cf:
            gx, gy = gx.transpose(1, 2), gy.transpose(1, 2)
        # fp32 projections (three products, three sums) and one fp32 difference: each g within e of its float64 value
        e = 8 * 2.0 ** -24 * 3 * max(np.abs(a).max(), np.abs(b).max())
        assert abs(float(out.detach()[0]) - dist) <= 2 * e * np.sqrt(dist) + e * e + 2.0 ** -23 * dist
        tol = 2.0 / (L * n) * L * e
        assert np.abs(gx[0].cpu().numpy() - ga).max() <= tol + 2.0 ** -23 * np.abs(ga).max()
        assert np.abs(gy[0].cpu().numpy() - gb).max() <= tol + 2.0 ** -23 * np.abs(gb).max()
        if not cf:
            both_x = gx.clone()
    x = torch.from_numpy(a[None]).to(dev()).requires_grad_(True)
    y = torch.from_numpy(b[None]).to(dev())
    S().sliced_wasserstein(x, y, d).sum().backward()                                        # only x asks for a gradient
    assert y.grad is None and torch.equal(x.grad, both_x)
    x2 = torch.from_numpy(a[None]).to(dev()).requires_grad_(True)
    self_d = S().sliced_wasserstein(x2, x2, d)
    self_d.sum().backward()
    assert float(self_d.detach()[0]) == 0.0 and (x2.grad == 0).all()


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_python_surface_errors_and_directions():
    x = torch.randn((2, 50, 3), device=dev())
    with pytest.raises(RuntimeError):
        S().sliced_wasserstein(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError):
        S().sliced_wasserstein(x.double(), x.double())
    with pytest.raises(ValueError, match="farthest_point_sample"):
        S().sliced_wasserstein(x, x[:, :40])
    with pytest.raises(ValueError, match="farthest_point_sample"):
        S().pairwise_SWD(x, x[:, :40])
    bad = x.clone()
    bad[1, 3, 0] = float("nan")
    with pytest.raises(ValueError, match="cloud 1 of 2 of y"):
        S().sliced_wasserstein(x, bad)
    d1, d2 = S().sliced_directions(128, 0), S().sliced_directions(128, 0)
    assert d1.dtype == torch.float32 and tuple(d1.shape) == (128, 3) and torch.equal(d1, d2)
    assert (d1.double().norm(dim=1) - 1).abs().max() <= 1e-7
    assert not torch.equal(d1, S().sliced_directions(128, 1))
    assert torch.equal(S().sliced_directions(128, 0, dev()).cpu(), d1)
    from dpf_nets_amd import metrics
    assert metrics.sliced_wasserstein is S().sliced_wasserstein and metrics.pairwise_SWD is S().pairwise_SWD
    default = S().sliced_wasserstein(x, x.flip(0))
    assert torch.equal(default, S().sliced_wasserstein(x, x.flip(0), S().sliced_directions(128, 0, dev())))


def test_compute_all_metrics_with_swd():
    from dpf_nets_amd.metrics import evaluation_metrics as E
    g = torch.Generator().manual_seed(3)
    smp = torch.randn((6, 64, 3), generator=g).to(dev())
    refc = (torch.randn((6, 64, 3), generator=g) * 1.1).to(dev())
    base = E.compute_all_metrics(smp, refc, 4)
    assert set(base) == {"%s-%s" % (k, m) for m in ("CD", "EMD") for k in ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")} | \
        {"1-NN-%s-%s" % (m, k) for m in ("CD", "EMD") for k in ("acc_t", "acc_f", "acc")}
    none = E.compute_all_metrics(smp, refc, 4, swd=None)
    assert set(none) == set(base) and all(torch.equal(none[k], base[k]) for k in base)
    full = E.compute_all_metrics(smp, refc, 4, swd=4)
    new = set(full) - set(base)
    assert new == {"lgan_mmd-SWD", "lgan_cov-SWD", "lgan_mmd_smp-SWD", "1-NN-SWD-acc_t", "1-NN-SWD-acc_f", "1-NN-SWD-acc"}
    assert all(torch.equal(full[k], base[k]) for k in base)
    M_rs, M_rr, M_ss = (S().pairwise_SWD(a, b, n_directions=4, seed=0) for a, b in ((refc, smp), (refc, refc), (smp, smp)))
    for k, v in E.lgan_mmd_cov(M_rs.t()).items():
        assert torch.equal(full["%s-SWD" % k], v)
    for k, v in E.knn(M_rr, M_rs, M_ss, 1, sqrt=False).items():
        if "acc" in k:
            assert torch.equal(full["1-NN-SWD-%s" % k], v)
    same = E.compute_all_metrics(refc, refc.clone(), 4, swd=4)
    assert float(same["lgan_mmd-SWD"]) == 0.0 and float(same["lgan_cov-SWD"]) == 1.0
    with pytest.raises(ValueError):
        E.compute_all_metrics(smp, refc, 4, swd=0)
