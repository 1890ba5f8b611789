"""dpf_rigid_fit and dpf_icp (csrc/align.hip) on the device against tests/align_ref.py, the numpy restatement of include/dpf_hip.h.
What is bit-defined (index, dist, inliers, sums, rmse, status) is compared for equality; R, t and s against the restatement's solve
of the KERNEL'S OWN sums, within align_ref.ALIGN_BOUND (measured on the CPU: test_align_ref_cpu.py).  The C ABI is called directly,
with sentinel guards around every output.  Failing without the feature: nothing exports metrics.icp on the parent commit."""
import os
import sys
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import align_ref as A                                                                        # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16
BOUND = A.ALIGN_BOUND


def _dev():
    return torch.device("cuda", 0)


class Guarded:
    """an output with GUARD sentinel elements on either side"""

    def __init__(self, shape, dtype):
        count = int(np.prod(shape))
        self.sentinel = -77 if dtype in (torch.int32,) else -7.7e7
        self.buf = torch.full((count + 2 * GUARD,), self.sentinel, dtype=dtype, device=_dev())
        self.view = self.buf[GUARD:GUARD + count].view(*shape)

    def ptr(self):
        return self.view.data_ptr()

    def take(self):
        edge = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((edge == self.sentinel).all()), "an output was written outside its extent"
        return self.view.cpu().numpy()


def _strides(t, channels_first):
    return (t.stride(0), t.stride(2), t.stride(1)) if channels_first else t.stride()


def raw_icp(src, dst, iters=0, max_dist2=0.0, with_scale=False, init=None, channels_first=False):
    """src, dst: float32 CUDA tensors (any strides) -> dict of numpy outputs, guards checked"""
    from dpf_nets_amd._lib import lib, check, current_stream
    B = src.shape[0]
    n, m = (src.shape[2], dst.shape[2]) if channels_first else (src.shape[1], dst.shape[1])
    o = dict(R=Guarded((B, 3, 3), torch.float64), t=Guarded((B, 3), torch.float64), s=Guarded((B,), torch.float64),
             index=Guarded((B, n), torch.int32), dist=Guarded((B, n), torch.float32), rmse=Guarded((B, iters + 1), torch.float64),
             inliers=Guarded((B, iters + 1), torch.int32), iterations=Guarded((B,), torch.int32), sums=Guarded((B, 18), torch.float64),
             status=Guarded((B,), torch.int32))
    nbytes = lib().dpf_align_workspace_bytes(B, n)
    ws = Guarded(((nbytes + 7) // 8,), torch.float64)
    T0 = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64).reshape(B, 13)).to(_dev())
    check(lib().dpf_icp(B, n, src.data_ptr(), *_strides(src, channels_first), m, dst.data_ptr(), *_strides(dst, channels_first), iters,
                        float(max_dist2), int(with_scale), None if T0 is None else T0.data_ptr(), o["R"].ptr(), o["t"].ptr(), o["s"].ptr(),
                        o["index"].ptr(), o["dist"].ptr(), o["rmse"].ptr(), o["inliers"].ptr(), o["iterations"].ptr(), o["sums"].ptr(),
                        o["status"].ptr(), ws.ptr(), nbytes, current_stream()), "icp")
    torch.cuda.synchronize()
    ws.take()
    out = {k: v.take() for k, v in o.items()}
    out["T"] = np.concatenate([out["R"].reshape(B, 9), out["t"], out["s"][:, None]], axis=1)
    return out


def raw_fit(src, dst, weights=None, with_scale=False):
    from dpf_nets_amd._lib import lib, check, current_stream
    B, n = src.shape[0], src.shape[1]
    o = dict(R=Guarded((B, 3, 3), torch.float64), t=Guarded((B, 3), torch.float64), s=Guarded((B,), torch.float64),
             rmse=Guarded((B,), torch.float64), sums=Guarded((B, 18), torch.float64), status=Guarded((B,), torch.int32))
    nbytes = lib().dpf_align_workspace_bytes(B, n)
    ws = Guarded(((nbytes + 7) // 8,), torch.float64)
    check(lib().dpf_rigid_fit(B, n, src.data_ptr(), *src.stride(), dst.data_ptr(), *dst.stride(), None if weights is None else weights.data_ptr(),
                              int(with_scale), o["R"].ptr(), o["t"].ptr(), o["s"].ptr(), o["rmse"].ptr(), o["sums"].ptr(), o["status"].ptr(),
                              ws.ptr(), nbytes, current_stream()), "rigid_fit")
    torch.cuda.synchronize()
    ws.take()
    out = {k: v.take() for k, v in o.items()}
    out["T"] = np.concatenate([out["R"].reshape(B, 9), out["t"], out["s"][:, None]], axis=1)
    return out


def batch(kinds, n, m, seed):
    pairs = [A.make_pair(kind, n, m, seed + 10 * b) for b, kind in enumerate(kinds)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def close(T, want, src, dst):
    """the bound of align_ref.py: |dR| <= BOUND, |ds| <= BOUND s, |dt| <= BOUND (|t| + s |src| + |dst|)"""
    R1, t1, s1 = A.unpack(T)
    R, t, s = A.unpack(want)
    extent = np.abs(t).max() + abs(s) * np.abs(src).max() + np.abs(dst).max()
    dev = max(np.abs(R1 - R).max(), abs(s1 - s) / abs(s), np.abs(t1 - t).max() / extent)
    print("deviation %.3g (bound %.3g)" % (dev, BOUND))
    return dev <= BOUND


def check_match(got, src, dst, inits, max_dist2, b):
    ref = A.icp(src[b], dst[b], iters=0, max_dist2=max_dist2, init=None if inits is None else inits[b])
    assert same(got["index"][b], ref["index"]), b
    assert same(got["dist"][b], ref["dist"]), b
    assert got["inliers"][b, 0] == ref["inliers"][0] and got["status"][b] == ref["status"] and got["iterations"][b] == 0, b
    assert same(got["sums"][b], ref["sums"]), (b, got["sums"][b] - ref["sums"])
    assert same(got["rmse"][b], ref["rmse"]), (b, got["rmse"][b], ref["rmse"])
    assert same(got["T"][b], A.IDENTITY if inits is None else inits[b]), b                  # iters = 0 returns what it was given


KINDS = ("gauss", "lattice", "far")


@pytest.mark.parametrize("trim", [0.0, 0.75])
@pytest.mark.parametrize("n,m", [(1, 1), (3, 3), (255, 257), (257, 255), (600, 513)])
def test_match_and_sums_under_a_given_init(n, m, trim):
    """iters = 0: one match under the init and its reduction.  lattice: integer coordinates, full of ties and duplicated targets."""
    src, dst = batch(KINDS, n, m, 1000 + n)
    inits = np.stack([A.make_init(b) if b != 1 else A.IDENTITY for b in range(3)])          # (the lattice keeps its ties under the identity)
    got = raw_icp(cuda(src), cuda(dst), 0, trim, init=inits)
    for b in range(3):
        check_match(got, src, dst, inits, trim, b)
    if trim and n >= 255:
        assert (got["index"][2] == -1).sum() >= n // 3 and 0 < got["inliers"][2, 0] < n
    if n >= 255:
        d = A.distances(src[1], dst[1])
        assert (np.sort(d, axis=1)[:, 0] == np.sort(d, axis=1)[:, 1]).mean() > 0.5            # the tie rule was exercised


def test_match_with_a_broadcast_target_channels_first_and_odd_strides():
    n, m = 257, 255
    src, dst = batch(KINDS, n, m, 77)
    dst = np.repeat(dst[:1], 3, axis=0)
    inits = np.stack([A.make_init(40 + b) for b in range(3)])
    one = cuda(dst[:1])
    got = raw_icp(cuda(src), one.expand(3, m, 3), 0, 0.0, init=inits)                        # cloud stride 0
    assert one.expand(3, m, 3).stride(0) == 0
    for b in range(3):
        check_match(got, src, dst, inits, 0.0, b)
    wide_s = torch.zeros((3, 3, 2 * n + 1), device=_dev())
    wide_d = torch.zeros((3, 5, m, 3), device=_dev())
    wide_s[:, :, 1::2] = cuda(src).transpose(1, 2)[:, :, :n]
    cf_src = wide_s[:, :, 1::2][:, :, :n]                                                     # (B, 3, n): point stride 2
    cf_dst = cuda(dst).transpose(1, 2).contiguous()                                          # (B, 3, m)
    got = raw_icp(cf_src, cf_dst, 0, 0.75, init=inits, channels_first=True)
    for b in range(3):
        check_match(got, src, dst, inits, 0.75, b)
    wide_d[:, 2] = cuda(dst)
    got = raw_icp(cuda(src), wide_d[:, 2], 0, 0.0, init=None)                                 # cloud stride 5 m 3, no init
    for b in range(3):
        check_match(got, src, dst, None, 0.0, b)
    from dpf_nets_amd.metrics import icp
    T, info = icp(cf_src, cf_dst, iters=0, max_dist=0.75 ** 0.5, init=(cuda(inits[:, :9].reshape(3, 3, 3)), cuda(inits[:, 9:12]), cuda(inits[:, 12])),
                  return_info=True, channels_first=True)
    got = raw_icp(cf_src, cf_dst, 0, float(0.75 ** 0.5) ** 2, init=inits, channels_first=True)
    assert same(info.index.cpu().numpy(), got["index"]) and same(info.dist.cpu().numpy(), got["dist"]) and same(T.R.cpu().numpy(), got["R"])
    assert T.R.dtype == torch.float64 and info.index.dtype == torch.int64 and not T.R.requires_grad


@pytest.mark.parametrize("with_scale", [False, True])
def test_the_solve_agrees_with_the_restatement_on_the_kernels_own_sums(with_scale):
    src, dst = batch(("rotated", "scaled", "offset"), 600, 513, 5)
    inits = np.stack([A.make_init(60 + b, 3.0) for b in range(3)])
    inits[2] = A.IDENTITY
    first = raw_icp(cuda(src), cuda(dst), 0, 0.0, init=inits)
    got = raw_icp(cuda(src), cuda(dst), 1, 0.0, with_scale, init=inits)
    for b in range(3):
        want, _ = A.solve(first["sums"][b], int(first["inliers"][b, 0]), src[b, 0], dst[b, 0], with_scale)
        assert got["status"][b] == 0 and got["iterations"][b] == 1
        assert close(got["T"][b], want, src[b], dst[b]), b
        assert abs(np.linalg.det(got["R"][b]) - 1.0) <= BOUND
        assert with_scale or got["s"][b] == 1.0
        assert same(got["rmse"][b, 0], first["rmse"][b, 0])
        again = A.match(src[b], dst[b], got["T"][b])                                        # the reported match belongs to what is returned
        assert same(got["index"][b], again[0]) and same(got["dist"][b], again[1])


def test_chained_single_iterations_and_a_repeat_give_the_same_bits():
    src, dst = batch(("rotated", "gauss", "scaled"), 300, 280, 9)
    s, d = cuda(src), cuda(dst)
    whole = raw_icp(s, d, 4, 0.0, True)
    again = raw_icp(s, d, 4, 0.0, True)
    for key in whole:
        assert same(whole[key], again[key]), key
    step, T = None, None
    for _ in range(4):
        step = raw_icp(s, d, 1, 0.0, True, init=T)
        T = step["T"]
    for key in ("R", "t", "s", "index", "dist", "sums"):
        assert same(whole[key], step[key]), key
    assert same(whole["rmse"][:, -1], step["rmse"][:, -1])


def test_a_converged_run_is_the_fit_of_its_own_matches():
    from dpf_nets_amd.metrics import rigid_fit
    src, dst = batch(("rotated", "rotated", "scaled"), 300, 300, 21)
    got = raw_icp(cuda(src), cuda(dst), 30, 0.0, True)
    assert (got["iterations"] < 30).all() and (got["status"] == 0).all()
    for b in range(3):
        index, dist, _, _ = A.match(src[b], dst[b], got["T"][b])
        assert same(got["index"][b], index) and same(got["dist"][b], dist) and index[0] == 0 and len(set(index.tolist())) == 300
    matched = torch.gather(cuda(dst), 1, cuda(got["index"]).long()[:, :, None].expand(-1, -1, 3))
    fit = raw_fit(cuda(src), matched, None, True)
    assert same(fit["T"], got["T"])                                                          # the same accumulate, the same solve
    T = rigid_fit(cuda(src), matched, with_scale=True)
    assert same(T.R.cpu().numpy(), got["R"]) and same(T.t.cpu().numpy(), got["t"]) and same(T.s.cpu().numpy(), got["s"])


def test_rigid_fit_sums_are_the_restatements_and_its_transform_is_within_the_bound():
    kinds = ("offset", "weighted", "scale")
    for n in (3, 257, 600):
        fits = [A.make_fit(kind, n, 300 + n + b) for b, kind in enumerate(kinds)]
        src, dst = np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits])
        w = np.stack([np.ones(n, dtype=np.float32) if f[2] is None else f[2] for f in fits])
        for with_scale in (False, True):
            got = raw_fit(cuda(src), cuda(dst), cuda(w), with_scale)
            for b in range(3):
                ref = A.rigid_fit(src[b], dst[b], w[b], with_scale)
                assert got["status"][b] == ref["status"] == 0
                assert same(got["sums"][b], ref["sums"]), (n, b)
                assert close(got["T"][b], ref["T"], src[b], dst[b]), (n, b)
                assert abs(got["rmse"][b] ** 2 - ref["rmse"] ** 2) * ref["sums"][0] <= 2.0 ** -40 * ref["sums"][17]


@pytest.mark.parametrize("kind,with_scale", [("rotated", False), ("scaled", True)])
def test_icp_recovers_a_known_transform(kind, with_scale):
    from dpf_nets_amd.metrics import icp, apply_transform
    src, dst = batch((kind,) * 3, 600, 600, 31)
    T, info = icp(cuda(src), cuda(dst), iters=40, with_scale=with_scale, return_info=True)
    assert (info.iterations.cpu().numpy() < 40).all() and (info.status == 0).all()
    s = 1.3 if with_scale else 1.0
    assert np.abs(T.R.cpu().numpy() - A.KNOWN_R).max() <= 1e-5 and np.abs(T.t.cpu().numpy() - A.KNOWN_T).max() <= 1e-5
    assert np.abs(T.s.cpu().numpy() - s).max() <= 1e-5
    moved = apply_transform(T, cuda(src))
    near = torch.gather(cuda(dst), 1, info.index[:, :, None].expand(-1, -1, 3))
    assert moved.dtype == torch.float32 and float((moved - near).abs().max()) <= 1e-5
    assert (np.diff(info.rmse.cpu().numpy(), axis=1) <= 1e-12 * info.rmse.cpu().numpy()[:, :-1]).all() or with_scale


def test_a_refused_and_a_degenerate_slot_leave_the_served_one_alone():
    from dpf_nets_amd.metrics import icp
    src, dst = batch(("rotated", "gauss", "gauss"), 257, 255, 41)
    src[1, 100, 2] = np.nan                                                                  # refused
    src[2] += np.float32(500.0)                                                              # everything beyond the trim: degenerate
    inits = np.stack([A.make_init(70 + b, 2.0) for b in range(3)])
    got = raw_icp(cuda(src), cuda(dst), 3, 0.25, init=inits)
    alone = raw_icp(cuda(src[:1]), cuda(dst[:1]), 3, 0.25, init=inits[:1])
    assert got["status"].tolist() == [0, A.REFUSED, A.DEGENERATE]
    for key in alone:
        assert same(got[key][:1], alone[key]), key
    ref = A.icp(src[0], dst[0], iters=3, max_dist2=0.25, init=inits[0])
    assert same(got["index"][0], ref["index"]) and same(got["inliers"][0], ref["inliers"]) and got["iterations"][0] == ref["iterations"]
    assert np.isnan(got["T"][1]).all() and (got["index"][1] == -1).all() and np.isnan(got["dist"][1]).all() and np.isnan(got["sums"][1]).all()
    assert np.isnan(got["rmse"][1]).all() and (got["inliers"][1] == 0).all() and got["iterations"][1] == 0
    assert same(got["T"][2], inits[2]) and (got["index"][2] == -1).all() and (got["inliers"][2] == 0).all() and got["iterations"][2] == 0
    with pytest.raises(ValueError, match="slot 1 of 3"):
        icp(cuda(src), cuda(dst), iters=3, max_dist=0.5)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        T = icp(cuda(src[[0, 2]]), cuda(dst[[0, 2]]), iters=3, max_dist=0.5)
    assert any("slot 1 of 2 is degenerate" in str(w.message) for w in seen)
    assert same(T.R[1].cpu().numpy(), np.eye(3)) and float(T.s[1]) == 1.0                    # the transform it kept: the identity
    big = src.copy()
    big[1, 100, 2] = np.float32(2.0 ** 30 * 1.5)                                              # finite, above the bound: an invalid VALUE
    assert raw_icp(cuda(big), cuda(dst), 1, 0.25, init=inits)["status"].tolist() == [0, A.REFUSED, A.DEGENERATE]
    bad = inits.copy()
    bad[0, 3] = np.inf
    assert raw_icp(cuda(src), cuda(dst), 1, 0.25, init=bad)["status"].tolist() == [A.REFUSED, A.REFUSED, A.DEGENERATE]


def test_more_slots_than_one_launch_takes():
    B = 32769
    rng = np.random.default_rng(3)
    src = rng.standard_normal((B, 4, 3)).astype(np.float32)
    dst = (src[:, ::-1] + 0.05 * rng.standard_normal((B, 4, 3))).astype(np.float32)
    got = raw_icp(cuda(src), cuda(dst), 2, 0.0)
    for b in (0, B - 1):
        alone = raw_icp(cuda(src[b:b + 1]), cuda(dst[b:b + 1]), 2, 0.0)
        for key in alone:
            assert same(got[key][b:b + 1], alone[key]), (b, key)
    assert (got["status"] >= 0).all() and (got["inliers"] == 4).all()
