"""Rigid alignment on the device (dpf_rigid_fit, dpf_icp, dpf_icp_plane: include/dpf_hip.h; csrc/align.hip): the weighted Procrustes
fit of given correspondences, trimmed point-to-point ICP and point-to-plane ICP -- what brings two clouds into one frame before Chamfer, F1 or an EMD compares them, so
that those measure the shape and not the pose.  No (B, n, m) tensor, no host round trip per iteration, every output bit-identical
from run to run.  Nothing the two searches return carries a gradient; a loss differentiates through apply_transform alone.  There is
no CPU path."""
import warnings
from collections import namedtuple

import torch

from .._lib import lib, check, current_stream
from .knn import _strides

ALIGN_DEGENERATE, ALIGN_REFUSED = 1, -1

RigidTransform = namedtuple("RigidTransform", ["R", "t", "s"])         # float64: (B, 3, 3), (B, 3), (B); y = s R p + t
ICPInfo = namedtuple("ICPInfo", ["index", "dist", "rmse", "inliers", "iterations", "status"])
PlaneICPInfo = namedtuple("PlaneICPInfo", ICPInfo._fields + ("rmse_plane", "step"))


def _readable(points, channels_first, what, who):
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3):
        raise RuntimeError("%s needs float32 CUDA tensors of shape (B, n, 3), or (B, 3, N) with channels_first (the %s is not); "
                           "there is no CPU path" % (who, what))
    pts = points.detach()
    if min(_strides(pts, channels_first, what)[2:]) < 0:
        pts = pts.contiguous()
    return (pts,) + _strides(pts, channels_first, what)


def _pack(T, B, device, who):
    """(B, 13) float64: R row-major, t, s"""
    R, t, s = T
    R = torch.as_tensor(R, dtype=torch.float64, device=device)
    t = torch.as_tensor(t, dtype=torch.float64, device=device)
    s = torch.as_tensor(s, dtype=torch.float64, device=device)
    if R.dim() == 2:
        R, t, s = R.expand(B, 3, 3), t.expand(B, 3), s.expand(B)
    if R.shape != (B, 3, 3) or t.shape != (B, 3) or s.shape != (B,):
        raise RuntimeError("%s: a transform is (R (B, 3, 3), t (B, 3), s (B,)) with B = %d, got %s, %s, %s"
                           % (who, B, tuple(R.shape), tuple(t.shape), tuple(s.shape)))
    return torch.cat([R.reshape(B, 9), t, s[:, None]], dim=1).contiguous()


def _report(status, who, refused="a coordinate, a weight or an entry of the initial transform is not finite or exceeds 2^30, or a weight "
            "is negative", degenerate="fewer than 3 matched points, no weight or no spread"):
    """the one synchronisation: a refused slot raises, a degenerate one warns"""
    st = status.cpu()
    bad = torch.nonzero(st == ALIGN_REFUSED)
    if bad.numel():
        raise ValueError("%s: slot %d of %d refused (%s); %d refused in all" % (who, int(bad[0, 0]), st.numel(), refused, bad.shape[0]))
    deg = torch.nonzero(st == ALIGN_DEGENERATE)
    if deg.numel():
        warnings.warn("%s: slot %d of %d is degenerate (%s); it keeps the transform it "
                      "had; %d degenerate in all" % (who, int(deg[0, 0]), st.numel(), degenerate, deg.shape[0]), RuntimeWarning, stacklevel=3)


def rigid_fit_raw(src, dst, weights=None, with_scale=False, channels_first=False, return_sums=False):
    """(R, t, s, rmse (B,), sums (B, 18) or None, status (B,) int32) of dpf_rigid_fit: no look at the statuses, no synchronisation."""
    p, B, n, psc, psp, psa = _readable(src, channels_first, "source", "rigid_fit")
    q, Bq, nq, qsc, qsp, qsa = _readable(dst, channels_first, "target", "rigid_fit")
    if Bq != B or nq != n or q.device != p.device:
        raise RuntimeError("rigid_fit: source and target must correspond point by point on one device, got %s and %s"
                           % (tuple(src.shape), tuple(dst.shape)))
    if n < 1:
        raise ValueError("rigid_fit: no points")
    dev = p.device
    w = None
    if weights is not None:
        if not (torch.is_tensor(weights) and weights.is_cuda and weights.shape == (B, n)):
            raise RuntimeError("rigid_fit: weights must be a CUDA tensor of shape (B, n) = (%d, %d)" % (B, n))
        w = weights.detach().to(torch.float32).contiguous()
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((B, 3), dtype=torch.float64, device=dev)
    s = torch.empty((B,), dtype=torch.float64, device=dev)
    rmse = torch.empty((B,), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 18), dtype=torch.float64, device=dev) if return_sums else None
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            nbytes = lib().dpf_align_workspace_bytes(B, n)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            check(lib().dpf_rigid_fit(B, n, p.data_ptr(), psc, psp, psa, q.data_ptr(), qsc, qsp, qsa, w.data_ptr() if w is not None else None,
                                      int(bool(with_scale)), R.data_ptr(), t.data_ptr(), s.data_ptr(), rmse.data_ptr(),
                                      sums.data_ptr() if return_sums else None, status.data_ptr(), ws.data_ptr(), nbytes, current_stream()),
                  "rigid_fit")
    return R, t, s, rmse, sums, status


def rigid_fit(src, dst, weights=None, with_scale=False, channels_first=False):
    """RigidTransform(R, t, s) minimising sum_i w_i |s R src_i + t - dst_i|^2 per slot: R (B, 3, 3) a proper rotation (det = +1, also
    where the unconstrained optimum is a reflection), t (B, 3), s (B,) -- 1 unless with_scale -- all float64.

    src and dst (B, n, 3), or (B, 3, N) with channels_first: float32 CUDA tensors, any strides (read in place; an expanded batch
    dimension broadcasts one set), point i of one belonging to point i of the other; a CPU tensor raises RuntimeError.  weights (B, n),
    optional, >= 0.  A slot with a coordinate or weight that is not finite or exceeds 2^30, or a negative weight, raises ValueError
    naming the slot -- reading the statuses is the one synchronisation.  A degenerate slot (fewer than 3 points of positive weight, or
    no spread under with_scale) warns and returns the identity.  One accumulate launch and one solve launch; the sums and their order
    are stated in include/dpf_hip.h.  NO GRADIENT: the result is a constant; differentiate through apply_transform."""
    R, t, s, _, _, status = rigid_fit_raw(src, dst, weights, with_scale, channels_first)
    _report(status, "rigid_fit")
    return RigidTransform(R, t, s)


def icp_raw(src, dst, iters=30, max_dist=None, with_scale=False, init=None, channels_first=False, return_sums=False):
    """dict of dpf_icp's outputs (R, t, s, index int32, dist, rmse, inliers, iterations, sums or None, status): no look at the statuses,
    no synchronisation."""
    p, B, n, psc, psp, psa = _readable(src, channels_first, "source", "icp")
    q, Bq, m, qsc, qsp, qsa = _readable(dst, channels_first, "target", "icp")
    if Bq != B or q.device != p.device:
        raise RuntimeError("icp: source and target must share the batch size and the device, got %s and %s" % (tuple(src.shape), tuple(dst.shape)))
    iters = int(iters)
    if iters < 0:
        raise ValueError("icp: iters must be >= 0, got %d" % iters)
    if n < 1 or m < 1:
        raise ValueError("icp: no points")
    if max_dist is not None and not float(max_dist) > 0:
        raise ValueError("icp: max_dist must be positive (None: no trim), got %r" % (max_dist,))
    max_dist2 = 0.0 if max_dist is None else float(max_dist) ** 2
    dev = p.device
    T0 = _pack(init, B, dev, "icp") if init is not None else None
    out = dict(R=torch.empty((B, 3, 3), dtype=torch.float64, device=dev), t=torch.empty((B, 3), dtype=torch.float64, device=dev),
               s=torch.empty((B,), dtype=torch.float64, device=dev), index=torch.empty((B, n), dtype=torch.int32, device=dev),
               dist=torch.empty((B, n), dtype=torch.float32, device=dev), rmse=torch.empty((B, iters + 1), dtype=torch.float64, device=dev),
               inliers=torch.empty((B, iters + 1), dtype=torch.int32, device=dev), iterations=torch.empty((B,), dtype=torch.int32, device=dev),
               sums=torch.empty((B, 18), dtype=torch.float64, device=dev) if return_sums else None,
               status=torch.empty((B,), dtype=torch.int32, device=dev))
    if B > 0:
        with torch.cuda.device(dev):
            nbytes = lib().dpf_align_workspace_bytes(B, n)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            check(lib().dpf_icp(B, n, p.data_ptr(), psc, psp, psa, m, q.data_ptr(), qsc, qsp, qsa, iters, max_dist2, int(bool(with_scale)),
                                T0.data_ptr() if T0 is not None else None, out["R"].data_ptr(), out["t"].data_ptr(), out["s"].data_ptr(),
                                out["index"].data_ptr(), out["dist"].data_ptr(), out["rmse"].data_ptr(), out["inliers"].data_ptr(),
                                out["iterations"].data_ptr(), out["sums"].data_ptr() if return_sums else None, out["status"].data_ptr(),
                                ws.data_ptr(), nbytes, current_stream()), "icp")
    return out


def icp(src, dst, iters=30, max_dist=None, with_scale=False, init=None, return_info=False, channels_first=False):
    """Point-to-point ICP of src onto dst: RigidTransform(R, t, s), float64, with apply_transform(T, src) lying on dst.

    src (B, n, 3) and dst (B, m, 3), or (B, 3, N) and (B, 3, M) with channels_first: float32 CUDA tensors, any strides; a CPU tensor
    raises RuntimeError.  Every iteration matches each source point, under the current transform, to its nearest target point (the
    Chamfer kernels' distance bits, the lowest index among equal distances) and solves for the ABSOLUTE transform from the original
    source points to their matches -- increments are never composed.  max_dist: matches farther than it are left out of the fit
    (trimmed ICP); None keeps all.  with_scale also fits a scale.  init: a RigidTransform, or any (R, t, s), per slot or one for all,
    to start from (the identity without one).  A slot stops when no match changes; 2 (iters + 1) launches, no synchronisation until the
    statuses are read.  A refused slot (a coordinate or init entry that is not finite or exceeds 2^30) raises ValueError naming it; a
    degenerate one (fewer than 3 matches) warns and returns the transform it kept.
    return_info: also ICPInfo(index (B, n) int64, -1 where a point has no match; dist (B, n) fp32 squared distances; rmse (B, iters
    + 1) float64 per match; inliers (B, iters + 1); iterations (B,); status (B,)) -- index, dist and the last rmse belong to the
    returned transform.  NO GRADIENT: everything returned is a constant; after icp a loss differentiates through apply_transform."""
    out = icp_raw(src, dst, iters, max_dist, with_scale, init, channels_first)
    _report(out["status"], "icp")
    T = RigidTransform(out["R"], out["t"], out["s"])
    if not return_info:
        return T
    return T, ICPInfo(out["index"].long(), out["dist"], out["rmse"], out["inliers"], out["iterations"], out["status"])


def icp_plane_raw(src, dst, normals, iters=30, max_dist=None, tol=1e-7, init=None, channels_first=False, return_sums=False):
    """dict of dpf_icp_plane's outputs (R, t, s, index int32, dist, rmse, rmse_plane, step, inliers, iterations, sums (B, 31) or None,
    status): no look at the statuses, no synchronisation.  normals: a float CUDA tensor of shape (B, m, 3), always points-major."""
    p, B, n, psc, psp, psa = _readable(src, channels_first, "source", "icp_plane")
    q, Bq, m, qsc, qsp, qsa = _readable(dst, channels_first, "target", "icp_plane")
    if Bq != B or q.device != p.device:
        raise RuntimeError("icp_plane: source and target must share the batch size and the device, got %s and %s"
                           % (tuple(src.shape), tuple(dst.shape)))
    if not (torch.is_tensor(normals) and normals.is_cuda and normals.is_floating_point() and normals.device == p.device
            and tuple(normals.shape) == (B, m, 3)):
        raise RuntimeError("icp_plane: normals must be a floating-point CUDA tensor of shape (B, m, 3) = (%d, %d, 3) on the clouds' "
                           "device; there is no CPU path" % (B, m))
    iters = int(iters)
    if iters < 0:
        raise ValueError("icp_plane: iters must be >= 0, got %d" % iters)
    if n < 1 or m < 1:
        raise ValueError("icp_plane: no points")
    if max_dist is not None and not float(max_dist) > 0:
        raise ValueError("icp_plane: max_dist must be positive (None: no trim), got %r" % (max_dist,))
    if not float(tol) >= 0:
        raise ValueError("icp_plane: tol must be >= 0, got %r" % (tol,))
    max_dist2 = 0.0 if max_dist is None else float(max_dist) ** 2
    dev = p.device
    nrm = normals.detach().to(torch.float64).contiguous()
    T0 = _pack(init, B, dev, "icp_plane") if init is not None else None
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    out = dict(R=f64(B, 3, 3), t=f64(B, 3), s=f64(B), index=i32(B, n), dist=torch.empty((B, n), dtype=torch.float32, device=dev),
               rmse=f64(B, iters + 1), rmse_plane=f64(B, iters + 1), step=f64(B, iters + 1), inliers=i32(B, iters + 1),
               iterations=i32(B), sums=f64(B, 31) if return_sums else None, status=i32(B))
    if B > 0:
        with torch.cuda.device(dev):
            nbytes = lib().dpf_icp_plane_workspace_bytes(B, n)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            check(lib().dpf_icp_plane(B, n, p.data_ptr(), psc, psp, psa, m, q.data_ptr(), qsc, qsp, qsa, nrm.data_ptr(), iters, max_dist2,
                                      float(tol), T0.data_ptr() if T0 is not None else None, out["R"].data_ptr(), out["t"].data_ptr(),
                                      out["s"].data_ptr(), out["index"].data_ptr(), out["dist"].data_ptr(), out["rmse"].data_ptr(),
                                      out["rmse_plane"].data_ptr(), out["step"].data_ptr(), out["inliers"].data_ptr(),
                                      out["iterations"].data_ptr(), out["sums"].data_ptr() if return_sums else None,
                                      out["status"].data_ptr(), ws.data_ptr(), nbytes, current_stream()), "icp_plane")
    return out


def icp_plane(src, dst, normals=None, k=16, iters=30, max_dist=None, tol=1e-7, init=None, return_info=False, channels_first=False):
    """Point-to-plane ICP of src onto dst: RigidTransform(R, t, s) with s = 1, float64.  For two samplings of ONE surface -- a
    decoder's samples against a ground-truth cloud -- where icp pulls every point toward a sample and stalls at a pose error set by
    the sampling density, this pulls every point toward the target's tangent plane at its match.

    src, dst, max_dist, init, channels_first and the match are icp's (init's scale must be 1).  normals (B, m, 3): one per target
    point, any float dtype (converted to dense float64), used as given -- not normalised; their SIGN IS IRRELEVANT, bit for bit, so
    estimate_normals' unoriented normals serve; None computes estimate_normals(dst, k) first (which synchronises once).  A normal with
    a NaN takes its target point's matches out of the fit.  Every iteration solves the damped 6 x 6 normal equations of the linearised
    distances and COMPOSES the increment (a proper rotation by construction) onto the transform.  A slot stops when no match changes
    and the step before was at most tol (|omega|^2 + |tau|^2 / the mean squared extent, rooted); tol = 0 stops on an exactly zero
    step only.  2 (iters + 1) launches, no synchronisation until the statuses are read.  A refused slot raises ValueError naming it;
    a degenerate one (fewer than 6 matches) warns and keeps its transform.  A rank-deficient geometry (a planar target) is served:
    the unknowns the data do not fix stay put.
    return_info: also PlaneICPInfo -- ICPInfo's fields, then rmse_plane (B, iters + 1), the root mean square point-to-plane
    residual per match, and step (B, iters + 1), the step taken from each match (0 where none was).  NO GRADIENT."""
    if normals is None:
        from .normals import estimate_normals
        normals = estimate_normals(dst, k, channels_first=channels_first, double=True)[0]
    out = icp_plane_raw(src, dst, normals, iters, max_dist, tol, init, channels_first)
    _report(out["status"], "icp_plane",
            "a coordinate or an entry of the initial transform is not finite or exceeds 2^30, the initial scale is not 1, or a finite "
            "normal component exceeds 2^30", "fewer than 6 matched points with a finite normal")
    T = RigidTransform(out["R"], out["t"], out["s"])
    if not return_info:
        return T
    return T, PlaneICPInfo(out["index"].long(), out["dist"], out["rmse"], out["inliers"], out["iterations"], out["status"],
                           out["rmse_plane"], out["step"])


def apply_transform(T, clouds, channels_first=False):
    """s R p + t for every point: clouds (B, n, 3), or (B, 3, N) with channels_first, any device; the result has the cloud's shape and
    dtype.  Plain tensor arithmetic in float64: differentiable with respect to the cloud, T a constant."""
    R, t, s = (x.detach() for x in T)
    x = clouds.to(torch.float64)
    if channels_first:
        y = s[:, None, None] * torch.matmul(R, x) + t[:, :, None]
    else:
        y = s[:, None, None] * torch.matmul(x, R.transpose(1, 2)) + t[:, None, :]
    return y.to(clouds.dtype)
