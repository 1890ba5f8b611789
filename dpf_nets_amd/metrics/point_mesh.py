"""Exact point-to-mesh distance on the device (csrc/point_mesh.hip) over a datasets.MeshStore: the squared distance from every
point of a predicted cloud to the surface it was sampled from -- Chamfer's predicted-to-truth half without the sampling noise
of a target cloud -- as a metric and as a loss with a gradient with respect to the points.

  point_mesh_distance -- dist (B, N), face (B, N)[, closest (B, N, 3)]
  surface_accuracy    -- dist.mean(1) (B,)[, the percentage of points nearer than a threshold]

and the other direction (csrc/mesh_point.hip), per face of the mesh the nearest point of the cloud -- what the prediction left
uncovered:

  mesh_point_distance  -- dist (B, W), point (B, W)[, closest (B, W, 3)][, area (B, W)]
  surface_completeness -- the area-weighted mean of dist over each mesh's faces (B,)[, the weighted percentage of faces reached]
  surface_chamfer      -- surface_accuracy + surface_completeness (B,)

The mesh is data: no gradient flows to its vertices.  The arithmetic and the tie rule are in include/dpf_hip.h."""
import numpy as np
import torch

from .._lib import lib, check, current_stream
from ..datasets.sampling import MeshStore, CloudTransform

__all__ = ["point_mesh_distance", "surface_accuracy", "mesh_point_distance", "surface_completeness", "surface_chamfer"]


def _launch(points, store, slots, max_faces, form, want_closest):
    B, N = int(points.shape[0]), int(points.shape[1])
    dev = points.device
    dist = torch.empty((B, N), dtype=torch.float32, device=dev)
    face = torch.empty((B, N), dtype=torch.int32, device=dev)
    closest = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if want_closest else None
    if B and N:
        L = lib()
        with torch.cuda.device(dev):
            nbytes = L.dpf_point_mesh_workspace_bytes(B, N)
            ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
            check(L.dpf_point_mesh_distance(*store.abi_args(), B, N, points.data_ptr(), slots.data_ptr(), max_faces, form,
                                            dist.data_ptr(), face.data_ptr(), None if closest is None else closest.data_ptr(),
                                            ws.data_ptr(), nbytes, current_stream()), "point_mesh_distance")
    return dist, face, closest


class _PointMeshDistance(torch.autograd.Function):
    """One node: the forward search saves the closest points, the backward is one launch of 2 * g * (p - closest)."""

    @staticmethod
    def forward(ctx, points, store, slots, max_faces, form, return_closest):
        wants_grad = bool(ctx.needs_input_grad[0])
        dist, face, closest = _launch(points, store, slots, max_faces, form, bool(return_closest) or wants_grad)
        if wants_grad:
            ctx.save_for_backward(points, closest)
        if closest is None:
            closest = points.new_empty((0,))
        ctx.mark_non_differentiable(face, closest)
        return dist, face, closest

    @staticmethod
    def backward(ctx, grad_dist, _grad_face, _grad_closest):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        points, closest = ctx.saved_tensors
        B, N = int(points.shape[0]), int(points.shape[1])
        grad = torch.empty_like(points)
        if B and N:
            g = grad_dist.contiguous()
            with torch.cuda.device(points.device):
                check(lib().dpf_point_mesh_distance_grad(B, N, points.data_ptr(), closest.data_ptr(), g.data_ptr(), grad.data_ptr(),
                                                         current_stream()), "point_mesh_distance_grad")
        return (grad,) + (None,) * 5


def _slots(mesh_indices, store, B):
    """(the int32 device tensor of mesh indices, the largest face count among them as far as the host knows)"""
    counts = store.face_counts
    if isinstance(mesh_indices, torch.Tensor):
        if mesh_indices.dim() != 1 or mesh_indices.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise RuntimeError("point_mesh_distance: mesh_indices must be a 1-D integer tensor, got %s %s"
                               % (mesh_indices.dtype, tuple(mesh_indices.shape)))
        if len(mesh_indices) != B:
            raise RuntimeError("point_mesh_distance: %d mesh indices for %d clouds" % (len(mesh_indices), B))
        if mesh_indices.is_cuda:
            if mesh_indices.device != store.device:
                raise RuntimeError("point_mesh_distance: mesh_indices are on %s, the store on %s" % (mesh_indices.device, store.device))
            return mesh_indices.to(torch.int32).contiguous(), int(counts.max())        # (no read-back: the largest mesh of the store)
        idx = mesh_indices.numpy()
    else:
        try:
            idx = np.asarray(mesh_indices)
        except Exception:
            raise RuntimeError("point_mesh_distance: mesh_indices must be a sequence of integers")
        if idx.size == 0:
            idx = idx.reshape(0).astype(np.int64)
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise RuntimeError("point_mesh_distance: mesh_indices must be a 1-D sequence of integers, got %s %s" % (idx.dtype, idx.shape))
    if len(idx) != B:
        raise RuntimeError("point_mesh_distance: %d mesh indices for %d clouds" % (len(idx), B))
    idx = idx.astype(np.int64)
    known = idx[(idx >= 0) & (idx < store.num_meshes)]
    most = int(counts[known].max()) if known.size else 1
    return torch.from_numpy(np.clip(idx, -1, store.num_meshes).astype(np.int32)).to(store.device), most


def _frame(store, transform, slots):
    """The similarity x' = ((orig_s * x + orig_c) - shift) / scale of the transform's fused steps, per slot: (mask, orig_s (B, 1, 1),
    orig_c (B, 1, 3), shift (3,), scale)."""
    if not isinstance(transform, CloudTransform):
        raise RuntimeError("point_mesh_distance: transform must be a datasets.CloudTransform or None")
    if transform.noise or transform.center:
        raise RuntimeError("point_mesh_distance: a transform with noise or centring cannot be undone from the cloud alone (%s)"
                           % ", ".join(transform.order()))
    mask, shift, scale = transform.fused()
    if (mask & 1 and store.orig_s is None) or (mask & 2 and store.orig_c is None):
        raise RuntimeError("point_mesh_distance: the transform rescales / recentres to the original frame but the store has no "
                           "orig_s / orig_c")
    at = slots.long().clamp(0, store.num_meshes - 1)                                   # (slots outside the store give NaN anyway)
    os_ = store.orig_s.index_select(0, at).view(-1, 1, 1) if mask & 1 else None
    oc = store.orig_c.index_select(0, at).view(-1, 1, 3) if mask & 2 else None
    return mask, os_, oc, torch.from_numpy(np.asarray(shift, np.float32)).to(store.device), float(scale)


def _checked(name, points, store, form):
    if not isinstance(store, MeshStore):
        raise RuntimeError("%s: store must be a datasets.MeshStore" % name)
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("%s needs a CUDA tensor of points (there is no CPU fallback)" % name)
    if points.dtype != torch.float32:
        raise RuntimeError("%s: points must be float32, got %s" % (name, points.dtype))
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("%s: points must be (B, N, 3), got %s" % (name, tuple(points.shape)))
    if points.device != store.device:
        raise RuntimeError("%s: points are on %s, the store on %s" % (name, points.device, store.device))
    if not points.is_contiguous():
        raise RuntimeError("%s: points must be contiguous (point-major, as nn_distance takes them)" % name)
    if form not in (0, 1, 2):
        raise RuntimeError("%s: form must be 0, 1 or 2" % name)


def _to_mesh_frame(points, store, transform, slots):
    """(the points mapped back into the meshes' frame by the transform's inverse steps, the factor (B, 1) or None that takes
    squared lengths of that frame to the clouds', the frame for _to_cloud_frame)"""
    if transform is None:
        return points, None, None
    mask, os_, oc, shift, scale = frame = _frame(store, transform, slots)
    local, factor = points, None
    if mask & 8:
        local = local * scale
    if mask & 4:
        local = local + shift
    if mask & 2:
        local = local - oc
    if mask & 1:
        local = local / os_
    if mask & 9:                                                                       # dist' = dist * (orig_s / scale)^2
        factor = (os_.view(-1, 1) if mask & 1 else 1.0) / (scale if mask & 8 else 1.0)
        factor = factor * factor
    return local.contiguous(), factor, frame


def _to_cloud_frame(closest, frame):
    if frame is None:
        return closest
    mask, os_, oc, shift, scale = frame
    if mask & 1:
        closest = closest * os_
    if mask & 2:
        closest = closest + oc
    if mask & 4:
        closest = closest - shift
    if mask & 8:
        closest = closest / scale
    return closest


def point_mesh_distance(points, store, mesh_indices, return_closest=False, transform=None, form=0):
    """dist (B, N) float32: the squared distance from points[b, i] to the nearest point of mesh mesh_indices[b] of `store`;
    face (B, N) int32: a face of that mesh attaining it (the lowest index among equals); with return_closest also closest
    (B, N, 3): the nearest point itself.  points: (B, N, 3) contiguous float32 CUDA tensor on the store's device; mesh_indices:
    a sequence of integers or a 1-D integer tensor of length B.  Anything else raises RuntimeError -- there is no CPU path.

    A slot whose mesh index is outside the store or whose mesh is flagged (a store built with strict=False), and a non-finite
    point, give dist NaN, face -1, closest NaN.  The results are bit-identical from run to run and do not depend on the batch.

    Autograd: one node.  d dist / d points = 2 * (points - closest), one launch in the backward, and none unless points needs a
    gradient; 0 where dist is NaN.  face and closest carry no gradient, and the mesh is data: nothing flows to its vertices.

    transform: the datasets.CloudTransform the clouds were sampled with (sample_clouds(..., transform=)), whose fused steps put
    them into the frame x' = ((orig_s * x + orig_c) - shift) / scale, each step present iff its flag is (rescale2orig,
    recenter2orig, translate, scale).  The points are mapped back by the inverse steps -- out-of-place float32 tensor ops, which
    autograd follows -- and, the map being a similarity, the squared distances are returned in the clouds' frame:
    dist' = dist * (orig_s / scale)^2 per mesh; closest is returned in the clouds' frame too.  A transform with noise or centring
    raises: those cannot be undone from the cloud alone.

    form: 0 lets csrc/dispatch.h choose the kernel form; 1 / 2 force one (tests)."""
    _checked("point_mesh_distance", points, store, form)
    slots, most = _slots(mesh_indices, store, int(points.shape[0]))
    local, factor, frame = _to_mesh_frame(points, store, transform, slots)
    dist, face, closest = _PointMeshDistance.apply(local, store, slots, most, int(form), bool(return_closest))
    if factor is not None:
        dist = dist * factor
    if not return_closest:
        return dist, face
    return dist, face, _to_cloud_frame(closest, frame)


def surface_accuracy(points, store, mesh_indices, threshold=None, transform=None):
    """(B,) mean squared distance from each cloud's points to its mesh: the predicted-to-surface half of Chamfer, exact.  With
    `threshold` also the (B,) percentage of points with dist < threshold -- f_score's precision term against the true surface.
    Arguments as point_mesh_distance; differentiable with respect to points through it."""
    dist, _ = point_mesh_distance(points, store, mesh_indices, transform=transform)
    if threshold is None:
        return dist.mean(1)
    return dist.mean(1), 100.0 * (dist < threshold).to(dist.dtype).mean(1)


# ---- the other direction: per face the nearest point ----------------------------------------------------------------------------
def _launch_faces(points, store, slots, width, form, want_closest, want_area):
    B, N = int(points.shape[0]), int(points.shape[1])
    dev = points.device
    dist = torch.empty((B, width), dtype=torch.float32, device=dev)
    point = torch.empty((B, width), dtype=torch.int32, device=dev)
    closest = torch.empty((B, width, 3), dtype=torch.float32, device=dev) if want_closest else None
    area = torch.empty((B, width), dtype=torch.float32, device=dev) if want_area else None
    if B and width:
        L = lib()
        with torch.cuda.device(dev):
            nbytes = L.dpf_mesh_point_workspace_bytes(B, width)
            ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
            check(L.dpf_mesh_point_distance(*store.abi_args(), B, N, points.data_ptr() if N else None, slots.data_ptr(), width, form,
                                            dist.data_ptr(), point.data_ptr(), None if closest is None else closest.data_ptr(),
                                            None if area is None else area.data_ptr(), ws.data_ptr(), nbytes, current_stream()),
                  "mesh_point_distance")
    return dist, point, closest, area


class _MeshPointDistance(torch.autograd.Function):
    """One node: the forward search saves the nearest points' indices and the closest points on the faces, the backward is one
    launch that gathers 2 * g * (p - closest) per point in face order."""

    @staticmethod
    def forward(ctx, points, store, slots, width, form, return_closest, return_area):
        wants_grad = bool(ctx.needs_input_grad[0])
        dist, point, closest, area = _launch_faces(points, store, slots, width, form, bool(return_closest) or wants_grad, bool(return_area))
        if wants_grad:
            ctx.save_for_backward(points, point, closest)
        if closest is None:
            closest = points.new_empty((0,))
        if area is None:
            area = points.new_empty((0,))
        ctx.mark_non_differentiable(point, closest, area)
        return dist, point, closest, area

    @staticmethod
    def backward(ctx, grad_dist, _grad_point, _grad_closest, _grad_area):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        points, point, closest = ctx.saved_tensors
        B, N, W = int(points.shape[0]), int(points.shape[1]), int(point.shape[1])
        grad = torch.empty_like(points)
        if B and N:
            g = grad_dist.contiguous()
            with torch.cuda.device(points.device):
                check(lib().dpf_mesh_point_distance_grad(B, N, W, points.data_ptr(), point.data_ptr(), closest.data_ptr(), g.data_ptr(),
                                                         grad.data_ptr(), current_stream()), "mesh_point_distance_grad")
        return (grad,) + (None,) * 6


def mesh_point_distance(points, store, mesh_indices, return_closest=False, return_area=False, transform=None, form=0):
    """The other direction of point_mesh_distance: for every face of mesh mesh_indices[b] the nearest of cloud b's points.
    dist (B, W) float32: the smallest squared distance from a point of the cloud to the closed triangle; point (B, W) int32: the
    index of a point attaining it (the lowest among equals); with return_closest also closest (B, W, 3): the point of the face
    nearest to that point; with return_area also area (B, W): the face's area as the store's sampler forms it.  W is the largest
    face count among the meshes asked for (of the store, when mesh_indices is a device tensor).  Arguments and refusals as
    point_mesh_distance: anything but a contiguous float32 (B, N, 3) CUDA tensor on the store's device raises RuntimeError --
    there is no CPU path.

    Columns past a mesh's own face count, and every column of a slot whose mesh index is outside the store, whose mesh is
    flagged or whose cloud has no finite point (N = 0 included), hold dist NaN, point -1, closest NaN, area 0.  A non-finite
    point is skipped.  The results are bit-identical from run to run and do not depend on the batch or the form.

    Autograd: one node.  d dist[b, f] / d points[b, point[b, f]] = 2 * (point - closest), gathered per point over the faces that
    name it in face order -- one launch in the backward, no atomics, and none unless points needs a gradient.  A point no face
    names gets 0.  point, closest and area carry no gradient, and the mesh is data: nothing flows to its vertices.

    transform: as in point_mesh_distance -- the points are mapped back by the inverse steps; dist and area are returned in the
    clouds' frame, dist' = dist * (orig_s / scale)^2 and area likewise, closest in the clouds' frame too.  A transform with noise
    or centring raises.

    form: 0 lets csrc/dispatch.h choose the kernel form; 1 / 2 force one (tests)."""
    _checked("mesh_point_distance", points, store, form)
    slots, width = _slots(mesh_indices, store, int(points.shape[0]))
    local, factor, frame = _to_mesh_frame(points, store, transform, slots)
    dist, point, closest, area = _MeshPointDistance.apply(local, store, slots, width, int(form), bool(return_closest), bool(return_area))
    if factor is not None:
        dist = dist * factor
        if return_area:
            area = area * factor
    out = (dist, point)
    if return_closest:
        out += (_to_cloud_frame(closest, frame),)
    if return_area:
        out += (area,)
    return out


def surface_completeness(points, store, mesh_indices, threshold=None, transform=None, weights="area"):
    """(B,) weighted mean over each mesh's faces of the squared distance from the face to the nearest point of its cloud: the
    surface-to-predicted half of Chamfer, which sees the geometry a cloud leaves uncovered (a cloud collapsed onto one corner
    scores a perfect surface_accuracy and a poor completeness).  weights: "area" -- each face's area over its mesh's total --
    or "uniform" -- 1 / F_b.  With `threshold` also the (B,) weighted percentage of faces with dist < threshold.  A bad slot (see
    mesh_point_distance) gives NaN.  Arguments as mesh_point_distance; differentiable with respect to points through it.

    What the number is: a face counts as reached when ONE point is near ANY part of it, so this is a lower bound on the
    surface-to-cloud distance an integral over the surface would give.  It is sharp for meshes whose faces are small against the
    spacing of the points and loose for a table top made of two triangles, which a single point on its diagonal covers.  For a
    sampled estimate of the integral use datasets.sample_clouds + nn_distance."""
    if weights not in ("area", "uniform"):
        raise RuntimeError("surface_completeness: weights must be 'area' or 'uniform'")
    dist, point, area = mesh_point_distance(points, store, mesh_indices, return_area=True, transform=transform)
    real = point >= 0
    w = area if weights == "area" else real.to(dist.dtype)
    w = w / w.sum(1, keepdim=True)                                                     # (0 / 0 = NaN: a bad slot)
    mean = (torch.where(real, dist, torch.zeros_like(dist)) * w).sum(1)
    if threshold is None:
        return mean
    return mean, 100.0 * ((real & (dist < threshold)).to(dist.dtype) * w).sum(1)


def surface_chamfer(points, store, mesh_indices, transform=None):
    """(B,) surface_accuracy + surface_completeness: both directions of the squared distance between a cloud and the surface it
    should lie on.  Arguments as point_mesh_distance; differentiable with respect to points."""
    return surface_accuracy(points, store, mesh_indices, transform=transform) + surface_completeness(points, store, mesh_indices,
                                                                                                       transform=transform)
