"""Farthest-point sampling on the device (dpf_fps, include/dpf_hip.h; csrc/fps.hip): the k points of a cloud that cover it best for
their number, chosen greedily -- each selection is the point farthest from those already taken, the lowest index among equals.
It is what brings clouds of any size to the common size that emd_exact, emd_approx, EMD_CD and the EMD halves of
compute_all_metrics need, without the uneven thinning of a random subset.  One launch per call, one workgroup per cloud, every
output bit-identical from run to run.  There is no CPU path."""
import torch

from .._lib import lib, check, current_stream

FPS_REFUSED = -1


def _strides(clouds, channels_first):
    """(B, n, the three strides in floats) of a 3-d tensor: any strided (B, n, 3) or (B, 3, N) view is read in place"""
    if channels_first:
        B, c, n = clouds.shape
        sc, sa, sp = clouds.stride()
    else:
        B, n, c = clouds.shape
        sc, sp, sa = clouds.stride()
    if c != 3:
        raise RuntimeError("farthest_point_sample needs %s clouds, got %s"
                           % ("(B, 3, N)" if channels_first else "(B, n, 3)", tuple(clouds.shape)))
    return B, n, sc, sp, sa


def farthest_point_index(clouds, k, start=None, channels_first=False, form=0):
    """(index (B, k) int32, radius2 (B, k) fp32, status (B,) int32) of dpf_fps, no check of the statuses and no synchronisation.
    form: 0 by size, 1, 2, ... force a kernel form (tests and tools)."""
    if not (torch.is_tensor(clouds) and clouds.is_cuda and clouds.dtype == torch.float32 and clouds.dim() == 3):
        raise RuntimeError("farthest_point_sample needs a float32 CUDA tensor of shape (B, n, 3), or (B, 3, N) with channels_first; "
                           "there is no CPU path")
    B, n, sc, sp, sa = _strides(clouds, channels_first)
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError("farthest_point_sample: k must be in 1..%d (the cloud's size), got %d" % (n, k))
    limit = lib().dpf_fps_max_points()
    if n > limit:
        raise RuntimeError("farthest_point_sample serves clouds of up to %d points, got %d" % (limit, n))
    dev = clouds.device
    src = clouds.detach()
    if min(sc, sp, sa) < 0:                                     # (no torch view has one; the three-stride form could not say "reversed")
        src = src.contiguous()
        B, n, sc, sp, sa = _strides(src, channels_first)
    if start is not None:
        start = torch.as_tensor(start, device=dev).to(torch.int32).reshape(-1).contiguous()
        if start.numel() == 1 and B != 1:
            start = start.expand(B).contiguous()
        if start.numel() != B:
            raise ValueError("farthest_point_sample: start must hold one index per cloud (%d), got %d" % (B, start.numel()))
    index = torch.empty((B, k), dtype=torch.int32, device=dev)
    radius2 = torch.empty((B, k), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(lib().dpf_fps(B, n, src.data_ptr(), sc, sp, sa, k, start.data_ptr() if start is not None else None, int(form),
                                index.data_ptr(), radius2.data_ptr(), status.data_ptr(), current_stream()), "fps")
    return index, radius2, status


def _fps_check(status, what):
    """ValueError naming the first refused cloud (reads the statuses: a device synchronisation)"""
    bad = torch.nonzero(status < 0)
    if bad.numel():
        raise ValueError("%s: cloud %d of %d refused (a non-finite coordinate or a start index outside the cloud); %d refused in all"
                         % (what, int(bad[0, 0]), status.numel(), bad.shape[0]))


def farthest_point_sample(clouds, k, start=None, channels_first=False, return_index=False, return_radius=False, form=0):
    """The k farthest-point samples of every cloud, in the input's layout: (B, k, 3) from (B, n, 3), or (B, 3, k) from (B, 3, N)
    with channels_first (the networks' layout).

    clouds: float32 CUDA tensor, any strides (every 3-d view is read in place through dpf_fps's three strides; only a negative
    stride, which no torch view has, would be copied); a CPU tensor raises RuntimeError.  k in 1..n, n <= 8192.  start: the first
    selection -- None (index 0 of every cloud), an int, or (B,) integers.  Selection t + 1 is the point whose squared distance
    to the nearest of selections 0..t is largest, the LOWEST index among equals (include/dpf_hip.h states the arithmetic); once
    every distinct position is taken the rule keeps returning index 0, so asking for more points than a cloud has distinct
    positions gives repeats of point 0.
    The subset is torch.gather by the selected indices: differentiable with respect to `clouds` (ones at the selected points), the
    indices are constants.
    return_index: also index (B, k) int64.  return_radius: also the covering radius (B, k) fp32 -- radius[:, t] is the largest
    DISTANCE (the square root of the kernel's radius2, not the squared value) from any point of the cloud to its nearest of the
    first t + 1 selections; it never increases, and radius[:, k-1] is the one-sided Hausdorff distance from the cloud to the
    subset.  Returns the subset alone, or a tuple (subset[, index][, radius]).
    A cloud with a non-finite coordinate or a start outside [0, n) is refused: ValueError naming the first such cloud (looking at
    the statuses synchronises with the device)."""
    index, radius2, status = farthest_point_index(clouds, k, start, channels_first, form)
    _fps_check(status, "farthest_point_sample")
    index = index.long()
    if channels_first:
        subset = torch.gather(clouds, 2, index[:, None, :].expand(-1, 3, -1))
    else:
        subset = torch.gather(clouds, 1, index[:, :, None].expand(-1, -1, 3))
    out = (subset,) + ((index,) if return_index else ()) + ((radius2.sqrt(),) if return_radius else ())
    return out if len(out) > 1 else subset
