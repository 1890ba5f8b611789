"""dpf_icp_plane (csrc/align.hip) on the device against tests/align_plane_ref.py, the numpy restatement of include/dpf_hip.h.
Everything is compared for EQUALITY: the match and the thirty-one sums are bit-defined, and the solve uses only + - * / sqrt in a
stated order, so the transform, the steps and the iteration counts are the restatement's too.  The C ABI is called directly, with
sentinel guards around every output and a dirty workspace.  Failing without the feature: the parent commit exports no dpf_icp_plane."""
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
import align_plane_ref as P                                                                  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16
KEYS = ("R", "t", "s", "index", "dist", "rmse", "rmse_plane", "step", "inliers", "iterations", "sums", "status")


def _dev():
    return torch.device("cuda", 0)


class Guarded:
    """an output with GUARD sentinel elements on either side, itself filled with the sentinel (a dirty buffer)"""

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


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def raw(src, dst, normals, iters=0, max_dist2=0.0, tol=1e-7, init=None, channels_first=False, with_sums=True):
    """src, dst: float32 CUDA tensors (any strides), normals a numpy (B, m, 3) float64 -> dict of numpy outputs, guards checked"""
    from dpf_nets_amd._lib import lib, check, current_stream
    B = src.shape[0]
    n, m = (src.shape[2], dst.shape[2]) if channels_first else (src.shape[1], dst.shape[1])
    K1 = iters + 1
    o = dict(R=Guarded((B, 3, 3), torch.float64), t=Guarded((B, 3), torch.float64), s=Guarded((B,), torch.float64),
             index=Guarded((B, n), torch.int32), dist=Guarded((B, n), torch.float32), rmse=Guarded((B, K1), torch.float64),
             rmse_plane=Guarded((B, K1), torch.float64), step=Guarded((B, K1), torch.float64), inliers=Guarded((B, K1), torch.int32),
             iterations=Guarded((B,), torch.int32), sums=Guarded((B, 31), torch.float64), status=Guarded((B,), torch.int32))
    nbytes = lib().dpf_icp_plane_workspace_bytes(B, n)
    ws = Guarded(((nbytes + 7) // 8,), torch.float64)                                        # (dirty: every word holds the sentinel)
    nrm = cuda(np.asarray(normals, dtype=np.float64))
    T0 = None if init is None else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64).reshape(B, 13)).to(_dev())
    check(lib().dpf_icp_plane(B, n, src.data_ptr(), *_strides(src, channels_first), m, dst.data_ptr(), *_strides(dst, channels_first),
                              nrm.data_ptr(), iters, float(max_dist2), float(tol), None if T0 is None else T0.data_ptr(), o["R"].ptr(),
                              o["t"].ptr(), o["s"].ptr(), o["index"].ptr(), o["dist"].ptr(), o["rmse"].ptr(), o["rmse_plane"].ptr(),
                              o["step"].ptr(), o["inliers"].ptr(), o["iterations"].ptr(), o["sums"].ptr() if with_sums else None,
                              o["status"].ptr(), ws.ptr(), nbytes, current_stream()), "icp_plane")
    torch.cuda.synchronize()
    ws.take()
    out = {k: v.take() for k, v in o.items()}
    if not with_sums:
        assert (out["sums"] == o["sums"].sentinel).all()                                     # NULL sums: nothing written
    out["T"] = np.concatenate([out["R"].reshape(B, 9), out["t"], out["s"][:, None]], axis=1)
    return out


def check_slot(got, ref, b, what=""):
    """every output of slot b against the restatement's dict, for equality"""
    for key in ("index", "dist", "rmse", "rmse_plane", "step", "inliers", "sums", "T"):
        assert same(got[key][b], ref[key]), (what, b, key, got[key][b], ref[key])
    assert got["iterations"][b] == ref["iterations"] and got["status"][b] == ref["status"], (what, b)


KINDS = ("gauss", "lattice", "far")


def batch(kinds, n, m, seed):
    pairs = [A.make_pair(kind, n, m, seed + 10 * b) for b, kind in enumerate(kinds)]
    src, dst = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return src, dst, np.stack([P.pair_normals(dst[b], seed + b) for b in range(len(kinds))])


@pytest.mark.parametrize("trim", [0.0, 0.75])
@pytest.mark.parametrize("n,m", [(1, 1), (3, 3), (6, 6), (255, 257), (257, 255), (600, 513)])
def test_match_sums_and_iteration_counts_are_the_restatements(n, m, trim):
    """iters = 0: the match under an init and its thirty-one sums; iters = 3: the changed-driven iteration counts.  lattice: integer
    coordinates under the identity, full of ties and duplicated targets."""
    src, dst, nrm = batch(KINDS, n, m, 1000 + n)
    inits = np.stack([A.make_init(b) if b != 1 else A.IDENTITY for b in range(3)])
    got0 = raw(cuda(src), cuda(dst), nrm, 0, trim, init=inits)
    got3 = raw(cuda(src), cuda(dst), nrm, 3, trim, tol=1e-3, init=inits)
    for b in range(3):
        check_slot(got0, P.icp_plane(src[b], dst[b], nrm[b], 0, trim, init=inits[b]), b, "iters 0")
        check_slot(got3, P.icp_plane(src[b], dst[b], nrm[b], 3, trim, tol=1e-3, init=inits[b]), b, "iters 3")
    if n < 6:
        assert (got3["status"] == A.DEGENERATE).all() and same(got3["T"], inits)
    if n >= 255:
        d = A.distances(src[1], dst[1])
        assert (np.sort(d, axis=1)[:, 0] == np.sort(d, axis=1)[:, 1]).mean() > 0.5            # the tie rule was exercised
        if trim:
            assert (got0["index"][2] == -1).sum() >= n // 3 and 0 < got0["inliers"][2, 0] < n


def ellipsoids(n, m, seeds=(0, 1, 2)):
    e = [P.make_ellipsoid_pair(n, m, s) for s in seeds]
    return np.stack([x[0] for x in e]), np.stack([x[1] for x in e]), np.stack([x[2] for x in e])


def test_one_solve_from_the_kernels_own_sums_is_the_restatements():
    src, dst, nrm = ellipsoids(600, 513)
    inits = np.stack([A.make_init(60 + b, 3.0) for b in range(3)])
    first = raw(cuda(src), cuda(dst), nrm, 0, init=inits)
    got = raw(cuda(src), cuda(dst), nrm, 1, init=inits)
    for b in range(3):
        want, step2 = P.solve(first["sums"][b], int(first["inliers"][b, 0]), dst[b, 0], inits[b])
        assert same(got["T"][b], want), (b, got["T"][b] - want)
        assert got["step"][b, 0] == np.sqrt(step2) and got["step"][b, 1] == 0.0 and got["iterations"][b] == 1 and got["s"][b] == 1.0
        again = P.match(src[b], dst[b], nrm[b], got["T"][b])                                 # the reported match belongs to what is returned
        assert same(got["index"][b], again[0]) and same(got["dist"][b], again[1])
        assert np.abs(got["R"][b].T @ got["R"][b] - np.eye(3)).max() <= P.ortho_bound(1, np.abs(A.unpack(inits[b])[0].T @ A.unpack(inits[b])[0] - np.eye(3)).max())


def test_a_full_run_chained_calls_repeats_and_a_batch_of_seventy_give_the_same_bits():
    src, dst, nrm = ellipsoids(257, 255)
    s, d = cuda(src), cuda(dst)
    whole = raw(s, d, nrm, 10, 0.3, tol=1e-9)
    for b in range(3):
        check_slot(whole, P.icp_plane(src[b], dst[b], nrm[b], 10, 0.3, tol=1e-9), b, "ten iterations")
        assert np.abs(whole["R"][b].T @ whole["R"][b] - np.eye(3)).max() <= P.ortho_bound(10)
    again = raw(s, d, nrm, 10, 0.3, tol=1e-9)
    for key in KEYS:
        assert same(whole[key], again[key]), key
    # T chained single iterations from the transform before; tol = 0 so that neither stops on its own
    T = 4
    whole = raw(s, d, nrm, T, 0.3, tol=0.0)
    step, cur = None, None
    for _ in range(T):
        step = raw(s, d, nrm, 1, 0.3, tol=0.0, init=cur)
        cur = step["T"]
    assert (whole["iterations"] == T).all()
    for key in ("R", "t", "s", "index", "dist", "sums", "status"):
        assert same(whole[key], step[key]), key
    for key in ("rmse", "rmse_plane", "inliers"):
        assert same(whole[key][:, -1], step[key][:, -1]) and same(whole[key][:, -2], step[key][:, 0]), key
    assert same(whole["step"][:, -2], step["step"][:, 0])
    # flipped normals: equal bits on the device too
    rng = np.random.default_rng(1)
    flipped = np.where((rng.random((3, 255)) < 0.5)[:, :, None], -nrm, nrm)
    other = raw(s, d, flipped, T, 0.3, tol=0.0)
    for key in KEYS:
        assert same(whole[key], other[key]) and same(np.signbit(whole[key]), np.signbit(other[key])), key
    # slot 1 alone against slot 1 in a batch of 70
    reps = np.arange(70) % 3
    many = raw(cuda(src[reps]), cuda(dst[reps]), nrm[reps], T, 0.3, tol=0.0)
    for key in KEYS:
        assert same(many[key][43:44], whole[key][1:2]) and same(many[key][69:70], whole[key][0:1]), key


def test_a_broadcast_target_channels_first_odd_strides_and_the_package():
    from dpf_nets_amd.metrics import icp_plane
    n, m = 257, 255
    src, dst, nrm = batch(KINDS, n, m, 77)
    dst, nrm = np.repeat(dst[:1], 3, axis=0), np.repeat(nrm[:1], 3, axis=0)
    inits = np.stack([A.make_init(40 + b) for b in range(3)])
    refs = [P.icp_plane(src[b], dst[b], nrm[b], 2, 0.75, init=inits[b]) for b in range(3)]
    one = cuda(dst[:1])
    assert one.expand(3, m, 3).stride(0) == 0
    got = raw(cuda(src), one.expand(3, m, 3), nrm, 2, 0.75, init=inits)                      # cloud stride 0
    wide_s = torch.zeros((3, 3, 2 * n + 1), device=_dev())
    wide_s[:, :, 1::2] = cuda(src).transpose(1, 2)
    cf_src, cf_dst = wide_s[:, :, 1::2], cuda(dst).transpose(1, 2).contiguous()              # (B, 3, n): point stride 2
    got_cf = raw(cf_src, cf_dst, nrm, 2, 0.75, init=inits, channels_first=True)
    wide_d = torch.zeros((3, 5, m, 3), device=_dev())
    wide_d[:, 2] = cuda(dst)
    got_w = raw(cuda(src), wide_d[:, 2], nrm, 2, 0.75, init=inits)                           # cloud stride 5 m 3
    for b in range(3):
        check_slot(got, refs[b], b, "broadcast")
        check_slot(got_cf, refs[b], b, "channels first")
        check_slot(got_w, refs[b], b, "wide")
    init = (cuda(inits[:, :9].reshape(3, 3, 3)), cuda(inits[:, 9:12]), cuda(inits[:, 12]))
    T, info = icp_plane(cf_src, cf_dst, cuda(nrm).float().double(), iters=2, max_dist=0.75 ** 0.5, init=init, return_info=True,
                        channels_first=True)
    want = raw(cf_src, cf_dst, nrm.astype(np.float32).astype(np.float64), 2, float(0.75 ** 0.5) ** 2, init=inits, channels_first=True)
    assert same(T.R.cpu().numpy(), want["R"]) and same(T.t.cpu().numpy(), want["t"]) and same(T.s.cpu().numpy(), np.ones(3))
    assert same(info.index.cpu().numpy(), want["index"]) and same(info.rmse_plane.cpu().numpy(), want["rmse_plane"])
    assert same(info.step.cpu().numpy(), want["step"]) and same(info.inliers.cpu().numpy(), want["inliers"])
    assert T.R.dtype == torch.float64 and info.index.dtype == torch.int64 and not T.R.requires_grad
    # a float32 normals tensor is converted, not refused
    T32 = icp_plane(cf_src, cf_dst, cuda(nrm).float(), iters=2, max_dist=0.75 ** 0.5, init=init, channels_first=True)
    assert same(T32.R.cpu().numpy(), want["R"])


def test_null_sums_and_return_codes():
    from dpf_nets_amd._lib import lib, current_stream
    src, dst, nrm = ellipsoids(40, 50)
    s, d = cuda(src), cuda(dst)
    with_sums, without = raw(s, d, nrm, 2), raw(s, d, nrm, 2, with_sums=False)
    for key in KEYS:
        assert key == "sums" or same(with_sums[key], without[key]), key
    L = lib()
    assert L.dpf_icp_plane_workspace_bytes(3, 40) == 3 * 31 * 8 + 3 * 8 + 3 * 2 * 4 + 3 * 2 * 4
    assert L.dpf_icp_plane_workspace_bytes(2, 600) == 2 * 3 * 31 * 8 + 2 * 8 + 2 * 3 * 2 * 4 + 2 * 2 * 4
    assert L.dpf_icp_plane_workspace_bytes(0, 40) == 0 and L.dpf_icp_plane_workspace_bytes(3, 0) == 0
    nbytes = L.dpf_icp_plane_workspace_bytes(3, 40)
    buf = torch.zeros(4096, dtype=torch.float64, device=_dev())
    nd = cuda(nrm)
    ptr = buf.data_ptr()

    def call(B=3, n=40, m=50, iters=2, tol=1e-7, normals=nd.data_ptr(), step=ptr + 8192, ws=ptr + 2048 * 8, wbytes=nbytes):
        return L.dpf_icp_plane(B, n, s.data_ptr(), *s.stride(), m, d.data_ptr(), *d.stride(), normals, iters, 0.0, tol, None, ptr, ptr + 512,
                               ptr + 1024, ptr + 1536, ptr + 4096, ptr + 6144, ptr + 7168, step, ptr + 9216, ptr + 10240, None, ptr + 11264,
                               ws, wbytes, current_stream())
    assert call() == 0
    torch.cuda.synchronize()
    einval = call(B=-1)
    assert einval != 0
    for bad in (dict(n=0), dict(m=0), dict(iters=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(normals=None), dict(step=None),
                dict(ws=None), dict(ws=ptr + 2048 * 8 + 4), dict(wbytes=nbytes - 1)):
        assert call(**bad) == einval, bad
    assert call(B=0) == 0
    torch.cuda.synchronize()


def test_a_nan_normal_at_a_matched_point_keeps_the_index_and_touches_nothing_else():
    src, dst, nrm = ellipsoids(257, 255)
    first = raw(cuda(src), cuda(dst), nrm, 0)
    bad = nrm.copy()
    hit = int(first["index"][0, 0])
    bad[0, hit, 1] = np.nan
    bad[1, int(first["index"][1, 5]), 0] = np.inf
    got = raw(cuda(src), cuda(dst), bad, 0)
    assert same(got["index"], first["index"]) and same(got["dist"], first["dist"]) and (got["status"] == 0).all()
    lost = int((first["index"][0] == hit).sum())
    assert got["inliers"][0, 0] == 257 - lost and got["sums"][0, 0] == 257 - lost and np.isfinite(got["sums"]).all()
    for key in KEYS:
        assert same(got[key][2], first[key][2]), key                                         # no other slot
    for b in range(2):
        check_slot(got, P.icp_plane(src[b], dst[b], bad[b], 0), b, "nan normal")
    run = raw(cuda(src), cuda(dst), bad, 3)
    for b in range(3):
        check_slot(run, P.icp_plane(src[b], dst[b], bad[b], 3), b, "nan normal, three iterations")


def test_a_refused_and_a_degenerate_slot_leave_the_served_one_alone():
    from dpf_nets_amd.metrics import icp_plane
    src, dst, nrm = ellipsoids(257, 255)
    bad = nrm.copy()
    bad[1, 200, 2] = 2.0 ** 30 * 1.5                                                         # finite, above the bound: refused
    keep = np.zeros(257, dtype=bool)
    keep[:5] = True
    src[2, ~keep] += np.float32(500.0)                                                       # five points within the trim: degenerate
    inits = np.stack([A.make_init(70 + b, 2.0) for b in range(3)])
    got = raw(cuda(src), cuda(dst), bad, 3, 0.25, init=inits)
    alone = raw(cuda(src[:1]), cuda(dst[:1]), bad[:1], 3, 0.25, init=inits[:1])
    assert got["status"].tolist() == [0, A.REFUSED, A.DEGENERATE]
    for key in alone:
        assert same(got[key][:1], alone[key]), key
    for b in range(3):
        check_slot(got, P.icp_plane(src[b], dst[b], bad[b], 3, 0.25, init=inits[b]), b, "refused / degenerate")
    assert np.isnan(got["T"][1]).all() and (got["index"][1] == -1).all() and np.isnan(got["dist"][1]).all() and np.isnan(got["sums"][1]).all()
    assert np.isnan(got["rmse_plane"][1]).all() and np.isnan(got["step"][1]).all() and (got["inliers"][1] == 0).all()
    assert same(got["T"][2], inits[2]) and (got["inliers"][2] == 5).all() and got["iterations"][2] == 0 and (got["step"][2] == 0).all()
    with pytest.raises(ValueError, match="slot 1 of 3"):
        icp_plane(cuda(src), cuda(dst), cuda(bad), iters=3, max_dist=0.5)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        T = icp_plane(cuda(src[[0, 2]]), cuda(dst[[0, 2]]), cuda(bad[[0, 2]]), iters=3, max_dist=0.5)
    assert any("slot 1 of 2 is degenerate" in str(w.message) for w in seen)
    assert same(T.R[1].cpu().numpy(), np.eye(3)) and float(T.s[1]) == 1.0
    scaled = inits.copy()
    scaled[0, 12] = 1.25                                                                     # no scale is fitted: an init with one is refused
    assert raw(cuda(src), cuda(dst), bad, 1, 0.25, init=scaled)["status"].tolist() == [A.REFUSED, A.REFUSED, A.DEGENERATE]
    nans = src.copy()
    nans[0, 100, 2] = np.nan
    assert raw(cuda(nans), cuda(dst), bad, 1, 0.25, init=inits)["status"].tolist() == [A.REFUSED, A.REFUSED, A.DEGENERATE]


def test_a_planar_target_is_served_by_the_pivot_rule():
    cases = [P.make_planar_target(200, 220, s) for s in (1, 2, 3)]
    src, dst, nrm = (np.stack([c[i] for c in cases]) for i in range(3))
    got = raw(cuda(src), cuda(dst), nrm, 8, tol=1e-12)
    for b in range(3):
        check_slot(got, P.icp_plane(src[b], dst[b], nrm[b], 8, tol=1e-12), b, "planar")
        _, ok = P.ldl_solve(raw(cuda(src[b:b + 1]), cuda(dst[b:b + 1]), nrm[b:b + 1], 0)["sums"][0])
        assert ok.count(False) == 3                                                          # three unknowns without data
    assert (got["status"] == 0).all() and (got["rmse_plane"][:, -1] < 1e-6).all() and (got["rmse_plane"][:, 0] > 1e-3).all()
    assert np.abs(got["t"]).max() < 1.0


def test_normals_none_is_estimate_normals_of_the_target():
    from dpf_nets_amd.metrics import icp_plane, estimate_normals
    src, dst, _ = ellipsoids(300, 280)
    s, d = cuda(src), cuda(dst)
    nrm = estimate_normals(d, 16, double=True)[0]
    a, ia = icp_plane(s, d, iters=6, return_info=True)
    b, ib = icp_plane(s, d, nrm, iters=6, return_info=True)
    for x, y in zip(tuple(a) + tuple(ia), tuple(b) + tuple(ib)):
        assert torch.equal(x, y) or same(x.cpu().numpy(), y.cpu().numpy())
    c = icp_plane(s, d, k=8, iters=6)
    assert same(c.R.cpu().numpy(), icp_plane(s, d, estimate_normals(d, 8, double=True)[0], iters=6).R.cpu().numpy())
    assert float(ia.rmse_plane[:, -1].max()) < float(ia.rmse_plane[:, 0].min())


def test_more_slots_than_one_launch_takes():
    B = 32769
    rng = np.random.default_rng(3)
    src = rng.standard_normal((B, 2, 3)).astype(np.float32)
    dst = rng.standard_normal((B, 7, 3)).astype(np.float32)
    nrm = rng.standard_normal((B, 7, 3))
    got = raw(cuda(src), cuda(dst), nrm, 2)
    for b in (0, 32767, 32768):
        alone = raw(cuda(src[b:b + 1]), cuda(dst[b:b + 1]), nrm[b:b + 1], 2)
        for key in KEYS:
            assert same(got[key][b:b + 1], alone[key]), (b, key)
        check_slot(got, P.icp_plane(src[b], dst[b], nrm[b], 2), b, "past the cut")
    assert (got["status"] == A.DEGENERATE).all() and (got["inliers"] == 2).all() and (got["index"] >= 0).all()
