"""Exact point-to-mesh distance on the device (csrc/point_mesh.hip) over a datasets.MeshStore: the squared distance from every
point of a predicted cloud to the surface it was sampled from -- Chamfer's predicted-to-truth half without the sampling noise
of a target cloud -- as a metric and as a loss with a gradient with respect to the points.

  point_mesh_distance -- dist (B, N), face (B, N)[, closest (B, N, 3)]
  surface_accuracy    -- dist.mean(1) (B,)[, the percentage of points nearer than a threshold]

The mesh is data: no gradient flows to its vertices.  The arithmetic and the tie rule are in include/dpf_hip.h."""
import numpy as np
import torch

from .._lib import lib, check, current_stream
from ..datasets.sampling import MeshStore, CloudTransform

__all__ = ["point_mesh_distance", "surface_accuracy"]


def _store_args(store):
    return (store.num_meshes, store.vertices.data_ptr(), store.vertex_bounds.data_ptr(), store.faces.data_ptr(),
            store.face_bounds.data_ptr(), store.flags.data_ptr())


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
            check(L.dpf_point_mesh_distance(*_store_args(store), B, N, points.data_ptr(), slots.data_ptr(), max_faces, form,
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
    if not isinstance(store, MeshStore):
        raise RuntimeError("point_mesh_distance: store must be a datasets.MeshStore")
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("point_mesh_distance needs a CUDA tensor of points (there is no CPU fallback)")
    if points.dtype != torch.float32:
        raise RuntimeError("point_mesh_distance: points must be float32, got %s" % points.dtype)
    if points.dim() != 3 or points.shape[2] != 3:
        raise RuntimeError("point_mesh_distance: points must be (B, N, 3), got %s" % (tuple(points.shape),))
    if points.device != store.device:
        raise RuntimeError("point_mesh_distance: points are on %s, the store on %s" % (points.device, store.device))
    if not points.is_contiguous():
        raise RuntimeError("point_mesh_distance: points must be contiguous (point-major, as nn_distance takes them)")
    if form not in (0, 1, 2):
        raise RuntimeError("point_mesh_distance: form must be 0, 1 or 2")
    slots, most = _slots(mesh_indices, store, int(points.shape[0]))
    local, factor = points, None
    if transform is not None:
        mask, os_, oc, shift, scale = _frame(store, transform, slots)
        if mask & 8:
            local = local * scale
        if mask & 4:
            local = local + shift
        if mask & 2:
            local = local - oc
        if mask & 1:
            local = local / os_
        if mask & 9:                                                                   # dist' = dist * (orig_s / scale)^2
            factor = (os_.view(-1, 1) if mask & 1 else 1.0) / (scale if mask & 8 else 1.0)
            factor = factor * factor
        local = local.contiguous()
    dist, face, closest = _PointMeshDistance.apply(local, store, slots, most, int(form), bool(return_closest))
    if factor is not None:
        dist = dist * factor
    if not return_closest:
        return dist, face
    if transform is not None:
        if mask & 1:
            closest = closest * os_
        if mask & 2:
            closest = closest + oc
        if mask & 4:
            closest = closest - shift
        if mask & 8:
            closest = closest / scale
    return dist, face, closest


def surface_accuracy(points, store, mesh_indices, threshold=None, transform=None):
    """(B,) mean squared distance from each cloud's points to its mesh: the predicted-to-surface half of Chamfer, exact.  With
    `threshold` also the (B,) percentage of points with dist < threshold -- f_score's precision term against the true surface.
    Arguments as point_mesh_distance; differentiable with respect to points through it."""
    dist, _ = point_mesh_distance(points, store, mesh_indices, transform=transform)
    if threshold is None:
        return dist.mean(1)
    return dist.mean(1), 100.0 * (dist < threshold).to(dist.dtype).mean(1)
