"""dpf_fps on the GPU against the numpy restatement of its contract (tests/fps_ref.py; the restatement itself is checked against a
float64 brute force in tests/test_fps_ref_cpu.py).  The contract is bit-defined, so index, radius2 and status are compared for
EQUALITY: no tolerance appears anywhere in this file.  The reference of a cloud is computed once, at k = n -- a smaller k is its
prefix, which is part of what is checked -- and shared."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import fps_ref as R                                                                          # noqa: E402

pytestmark = pytest.mark.gpu

NMAX = 8192
FORMS = {1: (64, 512), 2: (256, NMAX), 3: (1024, NMAX)}     # forced form -> (threads, the largest cloud it serves)
WAVE_UPTO, QUAD_UPTO = 512, 4096                    # dispatch.h: by size, form 1 up to the first, form 2 up to the second, form 3 above
SENTINEL_I, SENTINEL_F, GUARD = -7777, -12345.5, 256
_REF = {}


def dev():
    return torch.device("cuda", 0)


def L():
    from dpf_nets_amd import _lib
    return _lib


def F():
    from dpf_nets_amd.metrics import fps
    return fps


def named_form(n):
    return 1 if n <= WAVE_UPTO else 2 if n <= QUAD_UPTO else 3


def serving(n):
    return [f for f, (_, limit) in FORMS.items() if n <= limit]


def cloud(kind, n, seed):
    return R.make_cloud(kind, n, seed)


def ref(kind, n, seed, start=0):
    """the full run (k = n) of one cloud, cached"""
    key = (kind, n, seed, start)
    if key not in _REF:
        _REF[key] = R.fps(cloud(kind, n, seed), n, start)
    return _REF[key]


def run(pts, k, start=None, form=0, channels_first=False):
    """numpy or tensor clouds -> numpy index, radius2, status"""
    t = torch.from_numpy(pts).to(dev()) if isinstance(pts, np.ndarray) else pts
    out = F().farthest_point_index(t, k, None if start is None else torch.tensor(start, dtype=torch.int32), channels_first, form)
    return tuple(o.cpu().numpy() for o in out)


def raw(v):
    return np.ascontiguousarray(v).view(np.uint8)


def same_bits(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(raw(g), raw(w)) for g, w in zip(got, want))


def expect(refs, k):
    return (np.stack([r[0][:k] for r in refs]), np.stack([r[1][:k] for r in refs]), np.array([r[2] for r in refs], dtype=np.int32))


# each form's thread count and every step of the points per thread, at and either side; the shipped cloud sizes; the maximum
EDGES = sorted({1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2500, 4095, 4096,
                4097, NMAX - 1, NMAX})


@pytest.mark.parametrize("n", EDGES)
def test_sizes_at_the_kernel_edges_every_form_every_k(n):
    kinds = ("gauss", "lattice") if n <= 1100 else ("lattice" if n % 2 else "gauss",)
    starts = [(n // 3, n - 1)[s] for s in range(len(kinds))]
    pts = np.stack([cloud(kd, n, n) for kd in kinds])
    refs = [ref(kd, n, n, s) for kd, s in zip(kinds, starts)]
    ks = sorted({1, min(2, n), max(1, min(n, 70 + n // 7)), n})
    picked = {}
    for form in [0] + serving(n):
        for k in ks:
            if k == n and n >= NMAX - 1 and (form != 0 or n != NMAX):
                continue                                    # (the full-size case n = k = maximum: one cloud, once, the by-size pick)
            got = run(pts, k, starts, form)
            assert same_bits(got, expect(refs, k)), (n, form, k)
            picked[(form, k)] = got
    for k in ks:                                            # the by-size pick IS the forced form dispatch.h names
        if (0, k) in picked and (named_form(n), k) in picked:
            assert same_bits(picked[(0, k)], picked[(named_form(n), k)]), (n, k)


@pytest.mark.parametrize("n", (65, 300, 1500))
@pytest.mark.parametrize("kind", ("lattice", "dup", "same", "line"))
def test_ties(kind, n):
    pts = cloud(kind, n, 7)[None]
    want = expect([ref(kind, n, 7, 5)], n)
    if kind == "same":
        assert want[0][0].tolist() == [5] + [0] * (n - 1) and (want[1] == 0).all()
    for form in [0] + serving(n):
        assert same_bits(run(pts, n, [5], form), want), (kind, n, form)


def test_layouts_strides_and_a_broadcast_cloud():
    n, k, B = 333, 120, 3
    pts = np.stack([cloud("gauss", n, 40 + b) for b in range(B)])
    want = expect([ref("gauss", n, 40 + b) for b in range(B)], k)
    t = torch.from_numpy(pts).to(dev())
    assert same_bits(run(t, k), want)
    cf = t.transpose(1, 2).contiguous()                                                     # (B, 3, N)
    assert same_bits(run(cf, k, channels_first=True), want)
    assert same_bits(run(t.transpose(1, 2), k, channels_first=True), want)                 # a (B, 3, N) view of point-major memory
    big = torch.full((2 * B + 1, n + 9, 5), float("nan"), device=dev())                     # anything read outside the slice would refuse
    view = big[1::2, 4:4 + n, 1:4]
    view.copy_(t)
    assert not view.is_contiguous() and same_bits(run(view, k), want)
    bigc = torch.full((B + 2, 3, 2 * n + 6), float("nan"), device=dev())
    viewc = bigc[1:1 + B, :, 3:3 + 2 * n:2]
    viewc.copy_(cf)
    assert same_bits(run(viewc, k, channels_first=True), want)
    starts = [0, 17, n - 1, 200, 17]
    one = t[1:2].expand(len(starts), n, 3)                                                  # cloud_stride == 0
    assert one.stride(0) == 0
    assert same_bits(run(one, k, starts), expect([ref("gauss", n, 41, s) for s in starts], k))


def test_a_cloud_gives_the_same_bits_alone_first_and_last_of_300():
    n, k = 200, 60
    mine = cloud("gauss", n, 90)
    want = expect([ref("gauss", n, 90, 9)], k)
    rng = np.random.default_rng(5)
    others = rng.standard_normal((299, n, 3)).astype(np.float32)
    alone = run(mine[None], k, [9])
    assert same_bits(alone, want)
    first = run(np.concatenate([mine[None], others[:2]]), k, [9, 0, 1])
    last = run(np.concatenate([others, mine[None]]), k, [0] * 299 + [9])                    # 300 workgroups: more than the chip has CUs
    assert same_bits([o[:1] for o in first], want) and same_bits([o[-1:] for o in last], want)
    assert (last[2] == 0).all()
    for b in (0, 150, 298):
        assert same_bits([o[b:b + 1] for o in last], expect([R.fps(others[b], k, 0)], k)), b


@pytest.mark.parametrize("n,form", ((100, 0), (100, 2), (1300, 0)))
def test_refused_clouds_touch_no_neighbour(n, form):
    k = 33
    pts = np.stack([cloud("gauss", n, 60 + b) for b in range(7)])
    starts = [0, 0, 3, 0, n, 0, -1]
    pts[1, n - 1, 2] = np.nan
    pts[3, n // 2, 0] = -np.inf
    refs = [R.fps(pts[b], k, starts[b]) for b in range(7)]
    assert [r[2] for r in refs] == [0, -1, 0, -1, -1, 0, -1]
    got = run(pts, k, starts, form)
    assert same_bits(got, expect(refs, k))
    assert (got[0][[1, 3, 4, 6]] == -1).all() and np.isnan(got[1][[1, 3, 4, 6]]).all() and (got[0][[0, 2, 5]] >= 0).all()


def test_overflow_to_infinity_is_served():
    big = np.float32(3.0e38)
    pts = np.zeros((1, 70, 3), dtype=np.float32)
    pts[0, :, 1] = np.arange(70)
    pts[0, 0, 0], pts[0, 1, 0], pts[0, 66, 0], pts[0, 69, 0] = big, -big, 1.0e20, big
    want = expect([R.fps(pts[0], 70, 0)], 70)
    assert want[2][0] == 0 and np.isinf(want[1][0, 0]) and not np.isnan(want[1]).any()
    for form in [0] + serving(70):
        assert same_bits(run(pts, 70, None, form), want), form


def guarded(count, dtype, sentinel):
    buf = torch.full((GUARD + count + GUARD,), sentinel, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + count]


def call(t, k, start=None, form=0, want_radius=True, want_status=True):
    """the C entry itself on a dense (B, n, 3) tensor, every output between sentinel-filled guards"""
    lib, B, n = L().lib(), t.shape[0], t.shape[1]
    ibuf, index = guarded(B * k, torch.int32, SENTINEL_I)
    rbuf, radius2 = guarded(B * k, torch.float32, SENTINEL_F)
    sbuf, status = guarded(B, torch.int32, SENTINEL_I)
    st = None if start is None else torch.tensor(start, dtype=torch.int32, device=dev())
    rc = lib.dpf_fps(B, n, t.data_ptr(), n * 3, 3, 1, k, None if st is None else st.data_ptr(), form, index.data_ptr(),
                     radius2.data_ptr() if want_radius else None, status.data_ptr() if want_status else None, L().current_stream())
    torch.cuda.synchronize()
    return rc, [b.cpu().numpy() for b in (ibuf, rbuf, sbuf)]


def inner(bufs, B, k):
    return bufs[0][GUARD:-GUARD].reshape(B, k), bufs[1][GUARD:-GUARD].reshape(B, k), bufs[2][GUARD:-GUARD]


def guards_intact(bufs):
    return all((b[:GUARD] == s).all() and (b[-GUARD:] == s).all() for b, s in zip(bufs, (SENTINEL_I, SENTINEL_F, SENTINEL_I)))


@pytest.mark.parametrize("n,k", ((65, 65), (300, 7), (1025, 1025), (2500, 1030)))
def test_nothing_is_written_outside_the_outputs_and_null_outputs_change_nothing_else(n, k):
    B = 3
    pts = np.stack([cloud("gauss" if b else "same", n, 70 + b) for b in range(B)])
    pts[2, 0, 0] = np.nan                                                                   # (a refused cloud's fill stays inside too)
    want = expect([R.fps(pts[b], k, b) for b in range(B)], k)
    t = torch.from_numpy(pts).to(dev())
    for form in [0] + serving(n):
        rc, bufs = call(t, k, [0, 1, 2], form)
        assert rc == 0 and guards_intact(bufs) and same_bits(inner(bufs, B, k), want), (n, form)
        rc, bufs = call(t, k, [0, 1, 2], form, want_radius=False)
        assert rc == 0 and guards_intact(bufs) and (bufs[1] == SENTINEL_F).all(), (n, form)
        assert same_bits((inner(bufs, B, k)[0], inner(bufs, B, k)[2]), (want[0], want[2])), (n, form)
        rc, bufs = call(t, k, [0, 1, 2], form, want_status=False)
        assert rc == 0 and guards_intact(bufs) and (bufs[2] == SENTINEL_I).all(), (n, form)
        assert same_bits(inner(bufs, B, k)[:2], want[:2]), (n, form)


def test_return_codes():
    lib, st = L().lib(), L().current_stream()
    t = torch.from_numpy(cloud("gauss", 600, 1)[None]).to(dev())
    ibuf, index = guarded(600, torch.int32, SENTINEL_I)

    def rc(B=1, n=600, xyz=t.data_ptr(), k=4, form=0, out=index.data_ptr()):
        return lib.dpf_fps(B, n, xyz, n * 3, 3, 1, k, None, form, out, None, None, st)

    assert lib.dpf_fps_max_points() == NMAX
    assert rc(B=0) == 0                                                                     # nothing to do, nothing launched
    for bad in (dict(B=-1), dict(n=0), dict(k=0), dict(k=601), dict(form=-1), dict(form=len(FORMS) + 1), dict(xyz=None), dict(out=None)):
        assert rc(**bad) == -1, bad
    assert rc(form=1) == -2                                                                 # 600 points: past the one-wave form
    assert rc(n=NMAX + 1) == -2
    torch.cuda.synchronize()
    assert (ibuf.cpu().numpy() == SENTINEL_I).all()


def test_three_runs_give_identical_bits():
    pts = np.stack([cloud(kd, 2500, 3) for kd in ("gauss", "lattice", "dup")])
    runs = [run(pts, 700, [1, 2, 3]) for _ in range(3)]
    assert same_bits(runs[1], runs[0]) and same_bits(runs[2], runs[0])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_the_subset_is_the_gather_by_the_reference_indices_in_both_layouts():
    from dpf_nets_amd.metrics import farthest_point_sample
    n, k, B = 333, 50, 3
    pts = np.stack([cloud("gauss", n, 40 + b) for b in range(B)])
    idx, r2, _ = expect([ref("gauss", n, 40 + b) for b in range(B)], k)
    sub_want = np.stack([pts[b][idx[b]] for b in range(B)])
    t = torch.from_numpy(pts).to(dev())
    sub, index, radius = farthest_point_sample(t, k, return_index=True, return_radius=True)
    assert sub.shape == (B, k, 3) and np.array_equal(raw(sub.cpu().numpy()), raw(sub_want))
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), idx.astype(np.int64))
    # the radius, not its square: the device's own square root of the reference's radius2 (torch's sqrt is the one thing here that the
    # contract does not define bit for bit, so it is taken on the same device)
    assert torch.equal(radius, torch.from_numpy(r2).to(dev()).sqrt()) and (radius[:, 0] > 1).all()
    assert not torch.equal(radius, torch.from_numpy(r2).to(dev()))
    only = farthest_point_sample(t, k)
    assert torch.is_tensor(only) and torch.equal(only, sub)
    subc = farthest_point_sample(t.transpose(1, 2).contiguous(), k, channels_first=True)
    assert subc.shape == (B, 3, k) and torch.equal(subc, sub.transpose(1, 2))
    sub5 = farthest_point_sample(t[:1], k, start=5)
    assert np.array_equal(raw(sub5.cpu().numpy()), raw(pts[0][ref("gauss", n, 40, 5)[0][:k]][None]))


def test_backward_puts_ones_at_the_selected_points():
    from dpf_nets_amd.metrics import farthest_point_sample
    n, k = 129, 40
    pts = cloud("gauss", n, 11)
    idx = ref("gauss", n, 11)[0][:k]
    want = np.zeros((n, 3), dtype=np.float32)
    want[idx] = 1.0
    for cf in (False, True):
        t = torch.from_numpy(pts[None]).to(dev())
        t = (t.transpose(1, 2).contiguous() if cf else t).requires_grad_(True)
        farthest_point_sample(t, k, channels_first=cf).sum().backward()
        g = t.grad[0].t() if cf else t.grad[0]
        assert np.array_equal(g.cpu().numpy(), want), cf


def test_cpu_tensors_bad_k_and_refused_clouds_raise():
    from dpf_nets_amd.metrics import farthest_point_sample
    pts = torch.from_numpy(np.stack([cloud("gauss", 50, b) for b in range(3)]))
    with pytest.raises(RuntimeError):
        farthest_point_sample(pts, 10)
    with pytest.raises(RuntimeError):
        farthest_point_sample(pts.to(dev()).double(), 10)
    for k in (0, 51):
        with pytest.raises(ValueError):
            farthest_point_sample(pts.to(dev()), k)
    bad = pts.clone()
    bad[1, 7, 0] = float("nan")
    bad[2, 0, 1] = float("inf")
    with pytest.raises(ValueError, match="cloud 1 of 3"):
        farthest_point_sample(bad.to(dev()), 10)
    with pytest.raises(ValueError, match="cloud 2 of 3"):
        farthest_point_sample(pts.to(dev()), 10, start=[0, 49, 50])


@pytest.mark.parametrize("emd", ("approx", "exact"))
def test_compute_all_metrics_reduces_both_sets_by_fps(emd):
    from dpf_nets_amd.metrics.evaluation_metrics import compute_all_metrics
    K = 64
    smp = np.stack([cloud("gauss", 100, 200 + b) for b in range(6)])
    refc = np.stack([cloud("gauss", 130, 300 + b) * np.float32(0.9) for b in range(6)])
    smp_k = np.stack([smp[b][R.fps(smp[b], K)[0]] for b in range(6)])
    ref_k = np.stack([refc[b][R.fps(refc[b], K)[0]] for b in range(6)])
    to = lambda a: torch.from_numpy(a).to(dev())                                            # noqa: E731
    got = compute_all_metrics(to(smp), to(refc), 8, emd=emd, n_points=K)
    want = compute_all_metrics(to(smp_k), to(ref_k), 8, emd=emd)
    assert set(got) == set(want) and len(got) == 12
    for key in want:
        assert torch.equal(got[key], want[key]), key
    for bad in (101, 131):
        with pytest.raises(ValueError):
            compute_all_metrics(to(smp), to(refc), 8, emd=emd, n_points=bad)
