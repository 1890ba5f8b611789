"""k nearest neighbours on the device (dpf_knn, include/dpf_hip.h; csrc/knn.hip): for every query point the k nearest points of a
cloud and their squared distances, ascending, the lowest index first among equal distances -- the neighbourhood that a spacing
statistic, a repulsion or uniformity term or a local feature needs, without ever writing the (B, n, m) distance tensor.  One launch
per call, every output bit-identical from run to run, the distances those of nn_distance's kernels.  There is no CPU path."""
import torch

from .._lib import lib, check, current_stream

KNN_REFUSED = -1


def _strides(points, channels_first, what):
    """(B, n, the three strides in floats) of a 3-d tensor: any strided (B, n, 3) or (B, 3, N) view is read in place"""
    if channels_first:
        B, c, n = points.shape
        sc, sa, sp = points.stride()
    else:
        B, n, c = points.shape
        sc, sp, sa = points.stride()
    if c != 3:
        raise RuntimeError("knn_points needs a %s %s, got %s" % ("(B, 3, N)" if channels_first else "(B, n, 3)", what, tuple(points.shape)))
    return B, n, sc, sp, sa


def _readable(points, channels_first, what):
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3):
        raise RuntimeError("knn_points needs float32 CUDA tensors of shape (B, n, 3), or (B, 3, N) with channels_first (the %s is not); "
                           "there is no CPU path" % what)
    src = points.detach()
    if min(_strides(src, channels_first, what)[2:]) < 0:        # (no torch view has one; the three-stride form could not say "reversed")
        src = src.contiguous()
    return (src,) + _strides(src, channels_first, what)


def knn_index(query, cloud, k, exclude_self=False, channels_first=False, form=0):
    """(dist (B, n, k) fp32, index (B, n, k) int32, status (B,) int32) of dpf_knn, no check of the statuses and no synchronisation.
    form: 0 by k, 1..4 force the list capacity 4, 8, 16, 32 (tests and tools)."""
    q, B, n, qsc, qsp, qsa = _readable(query, channels_first, "query")
    c, Bc, m, csc, csp, csa = _readable(cloud, channels_first, "cloud")
    if Bc != B or c.device != q.device:
        raise RuntimeError("knn_points: query and cloud must share the batch size and the device, got %s and %s"
                           % (tuple(query.shape), tuple(cloud.shape)))
    k = int(k)
    limit = lib().dpf_knn_max_k()
    eligible = m - 1 if exclude_self else m
    if not 1 <= k <= min(limit, eligible):
        raise ValueError("knn_points: k must be in 1..%d (at most %d neighbours a call, %d eligible points), got %d"
                         % (min(limit, eligible), limit, eligible, k))
    if n < 1:
        raise ValueError("knn_points: no query points")
    dev = q.device
    dist = torch.empty((B, n, k), dtype=torch.float32, device=dev)
    index = torch.empty((B, n, k), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(lib().dpf_knn(B, n, q.data_ptr(), qsc, qsp, qsa, m, c.data_ptr(), csc, csp, csa, k, int(bool(exclude_self)), int(form),
                                dist.data_ptr(), index.data_ptr(), status.data_ptr(), current_stream()), "knn")
    return dist, index, status


class _KNN(torch.autograd.Function):
    """dist as one node; the indices are constants.  d = |q_i - c_j|^2, so the gradient of a listed pair is 2 g (q_i - c_j) for the
    query and its negative for the cloud point."""

    @staticmethod
    def forward(ctx, query, cloud, k, exclude_self, channels_first, form):
        dist, index, status = knn_index(query, cloud, k, exclude_self, channels_first, form)
        bad = torch.nonzero(status < 0)                                                      # (reads the statuses: a synchronisation)
        if bad.numel():
            raise ValueError("knn_points: slot %d of %d refused (a coordinate of its query or its cloud is not finite or exceeds 2^61); "
                             "%d refused in all" % (int(bad[0, 0]), status.numel(), bad.shape[0]))
        index = index.long()
        ctx.save_for_backward(query, cloud, index)
        ctx.channels_first = channels_first
        ctx.mark_non_differentiable(index)
        return dist, index

    @staticmethod
    def backward(ctx, g, _):
        query, cloud, index = ctx.saved_tensors
        cf = ctx.channels_first
        q = query.detach().transpose(1, 2) if cf else query.detach()                         # (B, n, 3) views
        c = cloud.detach().transpose(1, 2) if cf else cloud.detach()
        B, n, k = index.shape
        flat = index.reshape(B, n * k)
        nb = torch.gather(c, 1, flat[:, :, None].expand(-1, -1, 3)).reshape(B, n, k, 3)
        term = (2.0 * g)[..., None] * (q[:, :, None, :] - nb)                                # (B, n, k, 3) fp32
        gq = gc = None
        if ctx.needs_input_grad[0]:
            gq = term[:, :, 0]
            for s in range(1, k):                                                            # ascending s, whatever a reduction would do
                gq = gq + term[:, :, s]
            gq = gq.transpose(1, 2) if cf else gq
        if ctx.needs_input_grad[1]:
            m = c.shape[1]
            rows = (flat + torch.arange(B, device=flat.device)[:, None] * m).reshape(-1)      # row of (b, j) in a (B * m, 3) table
            gc = torch.zeros((B * m, 3), dtype=term.dtype, device=term.device).index_add_(0, rows, -term.reshape(-1, 3)).view(B, m, 3)
            gc = gc.transpose(1, 2) if cf else gc
        return gq, gc, None, None, None, None


def knn_points(query, cloud, k, exclude_self=False, channels_first=False, return_index=True, form=0):
    """The k nearest points of `cloud` for every point of `query`: dist (B, n, k) fp32, the squared distances in ascending order,
    and index (B, n, k) int64 (dist alone with return_index=False).

    query (B, n, 3) and cloud (B, m, 3), or (B, 3, N) and (B, 3, M) with channels_first (the networks' layout): float32 CUDA
    tensors, any strides -- every 3-d view is read in place through dpf_knn's strides (an expanded batch dimension broadcasts one
    set; only a negative stride, which no torch view has, would be copied); a CPU tensor raises RuntimeError.  The two may be the
    same tensor.  k in 1..32 and at most the number of eligible points (ValueError).  exclude_self: candidate i is not a neighbour of
    query i -- by index, for a self-search; a duplicate of the query elsewhere in the cloud stays a neighbour at distance 0.  Equal
    distances are ordered by the lowest index (include/dpf_hip.h states the arithmetic and the order).
    dist is one autograd node, the indices are constants: grad_query[i] = sum_s 2 g[i, s] (q_i - c_index[i, s]), added in ascending
    s; grad_cloud[j] = the matching negative sum over every (i, s) with index[i, s] == j.  The backward is tensor arithmetic
    (a gather and index_add_): it repeats bit for bit ONLY under torch.use_deterministic_algorithms(True) -- without it index_add_
    adds in an order that changes from run to run.
    A slot with a non-finite coordinate, or one above 2^61 in magnitude, in either set is refused: ValueError naming the first such
    slot (looking at the statuses synchronises with the device)."""
    dist, index = _KNN.apply(query, cloud, int(k), bool(exclude_self), bool(channels_first), int(form))
    return (dist, index) if return_index else dist


def knn_gather(values, index):
    """values (B, m, C) gathered by index (B, n, k) -> (B, n, k, C): out[b, i, s] = values[b, index[b, i, s]].  Differentiable with
    respect to values."""
    B, n, k = index.shape
    C = values.shape[2]
    return torch.gather(values, 1, index.reshape(B, n * k, 1).expand(-1, -1, C)).reshape(B, n, k, C)


def neighbour_spacing(clouds, k=1):
    """How evenly a cloud covers its surface: per point the DISTANCE (the square root of the kernel's squared distance) to its k-th
    nearest other point, then (mean, cv) over the cloud, each (B,) float64.  cv is the coefficient of variation -- the population
    standard deviation over the mean -- the uniformity number: 0 where every point has the same k-th spacing (the interior of a
    lattice), larger for clumped clouds.  clouds (B, n, 3) float32 CUDA, 1 <= k <= min(32, n - 1).  Float64 arithmetic on dist; no
    gradient."""
    with torch.no_grad():
        dist = knn_points(clouds, clouds, k, exclude_self=True, return_index=False)
        s = dist[:, :, k - 1].double().sqrt()
        mean = s.mean(1)
        return mean, ((s - mean[:, None]) ** 2).mean(1).sqrt() / mean
