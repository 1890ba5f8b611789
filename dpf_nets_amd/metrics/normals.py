"""Point-cloud normals on the device (dpf_normals, include/dpf_hip.h; csrc/normals.hip): per point the covariance of its k nearest
points, the eigenvalues of that 3 x 3 matrix and the unit eigenvector of the smallest one, by a fixed number of Jacobi sweeps in
float64 -- the local feature that says which way a surface FACES, and with it the normal-consistency score reported beside Chamfer
and F1.  A k-nearest-neighbour launch (metrics/knn.py) and one dpf_normals launch; no (B, n, k, 3) tensor.  Nothing here has a
gradient: the outputs are detached.  There is no CPU path."""
import torch

from .._lib import lib, check, current_stream
from .knn import _readable, knn_index
from .StructuralLosses import StructuralLossesBackend as _backend

MIN_K, MAX_K = 3, 32


def _viewpoint(viewpoint, B, device):
    """(tensor or None, slot stride in floats): (3,) broadcasts, (B, 3) gives every slot its own (an expanded one broadcasts too)"""
    if viewpoint is None:
        return None, 0
    w = torch.as_tensor(viewpoint, dtype=torch.float32, device=device).detach()
    if w.dim() == 1 and w.shape[0] == 3:
        return w.contiguous(), 0
    if w.dim() == 2 and w.shape == (B, 3):
        if w.stride(0) == 0 and w.stride(1) == 1:
            return w, 0
        return w.contiguous(), 3
    raise RuntimeError("normals: the viewpoint must have shape (3,) or (B, 3) = (%d, 3), got %s" % (B, tuple(w.shape)))


def normals_from_index(cloud, index, viewpoint=None, channels_first=False, return_cov=False):
    """The raw call: (normal (B, n, 3), eigenvalues (B, n, 3) ascending, flag (B, n) int32), with cov (B, n, 6) -- xx, xy, xz, yy, yz,
    zz -- in front of flag under return_cov; float64, no look at the flags and no synchronisation.

    cloud (B, m, 3), or (B, 3, M) with channels_first: a float32 CUDA tensor, any strides (read in place).  index (B, n, k), 3 <= k <=
    32, int32 or int64 (an int64 table is converted with one .to(torch.int32)): row (b, i) lists the neighbourhood of point i, as
    knn_index writes it.  viewpoint: None, (3,) or (B, 3) -- the normals are turned towards it; without one the component of
    largest magnitude is positive.  A point whose list holds an index outside [0, m), or reaches a coordinate that is not finite or
    exceeds 2^61, gets flag 1 and NaN; no other point is touched.  No gradient."""
    c, B, m, csc, csp, csa = _readable(cloud, channels_first, "cloud")
    if not (torch.is_tensor(index) and index.is_cuda and index.dim() == 3 and index.dtype in (torch.int32, torch.int64)
            and index.shape[0] == B and index.device == c.device):
        raise RuntimeError("normals_from_index needs an int32 or int64 CUDA index of shape (B, n, k) = (%d, n, k) on the cloud's device" % B)
    idx = index.detach()
    idx = (idx.to(torch.int32) if idx.dtype == torch.int64 else idx).contiguous()
    n, k = idx.shape[1], idx.shape[2]
    if not MIN_K <= k <= MAX_K:
        raise ValueError("normals: k must be in %d..%d, got %d" % (MIN_K, MAX_K, k))
    if n < 1:
        raise ValueError("normals: no query points")
    dev = c.device
    w, wss = _viewpoint(viewpoint, B, dev)
    normal = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
    lam = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
    cov = torch.empty((B, n, 6), dtype=torch.float64, device=dev) if return_cov else None
    flag = torch.empty((B, n), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(lib().dpf_normals(B, n, m, c.data_ptr(), csc, csp, csa, idx.data_ptr(), k, w.data_ptr() if w is not None else None, wss,
                                    normal.data_ptr(), lam.data_ptr(), cov.data_ptr() if return_cov else None, flag.data_ptr(),
                                    current_stream()), "normals")
    return (normal, lam, cov, flag) if return_cov else (normal, lam, flag)


def estimate_normals(clouds, k=16, viewpoint=None, channels_first=False, double=False):
    """(normals (B, n, 3), eigenvalues (B, n, 3) float64, ascending) of every point of `clouds`, from the k nearest points of its own
    cloud INCLUDING the point itself: knn_index(clouds, clouds, k, exclude_self=False), then one dpf_normals launch.

    clouds (B, n, 3), or (B, 3, N) with channels_first: float32 CUDA, any strides; a CPU tensor raises RuntimeError.  3 <= k <=
    min(32, n), else ValueError.  normals has the cloud's dtype, float64 under double; it is always (B, n, 3).  The sign: towards the
    viewpoint ((3,) or (B, 3)) where one is given, else the component of largest magnitude is positive.  The eigenvalues are those of
    the UNNORMALISED covariance sum_s (p_s - c)(p_s - c)^T (surface_variation is a ratio of them).  A point that reaches a coordinate
    which is not finite or exceeds 2^61 raises ValueError naming the first (slot, point) -- reading the flags is the one
    synchronisation.  NO GRADIENT: both outputs are detached; the derivative of an eigenvector is out of scope on purpose."""
    if not (torch.is_tensor(clouds) and clouds.dim() == 3):
        raise RuntimeError("estimate_normals needs a float32 CUDA tensor of shape (B, n, 3), or (B, 3, N) with channels_first; there is no CPU path")
    k = int(k)
    n = clouds.shape[2] if channels_first else clouds.shape[1]
    if not MIN_K <= k <= min(MAX_K, n):
        raise ValueError("estimate_normals: k must be in %d..%d (at most %d neighbours, %d points in a cloud), got %d"
                         % (MIN_K, min(MAX_K, n), MAX_K, n, k))
    _, index, _ = knn_index(clouds, clouds, k, False, channels_first)          # (a refused slot's rows are -1: every point of it is flagged)
    normal, lam, flag = normals_from_index(clouds, index, viewpoint, channels_first)
    bad = torch.nonzero(flag)                                                  # (reads the flags: a synchronisation)
    if bad.numel():
        raise ValueError("estimate_normals: point (%d, %d) reaches a coordinate that is not finite or exceeds 2^61; %d points flagged in all"
                         % (int(bad[0, 0]), int(bad[0, 1]), bad.shape[0]))
    return (normal if double else normal.to(clouds.dtype)), lam


def surface_variation(eigenvalues):
    """lambda_0 / (lambda_0 + lambda_1 + lambda_2) of (..., 3) ascending eigenvalues, float64: 0 on a plane, 1/3 where the
    neighbourhood has no preferred direction; 0 where the sum is 0."""
    lam = eigenvalues.detach().double()
    total = (lam[..., 0] + lam[..., 1]) + lam[..., 2]
    return torch.where(total == 0, torch.zeros_like(total), lam[..., 0] / torch.where(total == 0, torch.ones_like(total), total))


def normal_consistency(a, b, k=16, normals_a=None, normals_b=None):
    """(a_to_b, b_to_a), each (B,) float64: for every point i of a the |n_a[i] . n_b[j]| with j its nearest point of b, averaged over
    i -- and the same from b.  Unoriented (the absolute value): 1 where the two surfaces face the same way wherever they are close.

    a (B, n, 3) and b (B, m, 3): contiguous float32 CUDA clouds.  The nearest points are the Chamfer kernels' (one NNDistance call,
    both index rows).  normals_a (B, n, 3) / normals_b (B, m, 3): the clouds' normals where the caller has them (true normals of a
    mesh sample, say); estimated with estimate_normals(., k, double=True) where not passed in.  Float64 arithmetic; no gradient."""
    with torch.no_grad():
        a, b = a.detach(), b.detach()
        _, i1, _, i2 = _backend.NNDistance(a, b)
        na = estimate_normals(a, k, double=True)[0] if normals_a is None else normals_a.detach().double()
        nb = estimate_normals(b, k, double=True)[0] if normals_b is None else normals_b.detach().double()
        if na.shape != a.shape or nb.shape != b.shape:
            raise RuntimeError("normal_consistency: normals must have their cloud's shape, got %s for %s and %s for %s"
                               % (tuple(na.shape), tuple(a.shape), tuple(nb.shape), tuple(b.shape)))

        def score(n_from, n_to, nearest):
            near = torch.gather(n_to, 1, nearest.long()[:, :, None].expand(-1, -1, 3))
            return (n_from * near).sum(-1).abs().mean(1)

        return score(na, nb, i1), score(nb, na, i2)
