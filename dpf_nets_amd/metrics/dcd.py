"""Density-aware Chamfer distance on the device (dpf_dcd: include/dpf_hip.h; csrc/dcd.hip): DCD of Wu et al., "Balanced Chamfer
Distance as a Comprehensive Metric for Point Cloud Completion" (NeurIPS 2021) -- Chamfer's search, every nearest-neighbour term bounded
(1 - exp(-alpha d)) and divided by the number of queries that chose the same target point, so a prediction that piles its points onto
a few spots of the target no longer scores like a uniform one.  An evaluation number and a training loss: the counts, the per-cloud
loss and the per-point gradient coefficients are ONE launch behind the search, the backward is the deterministic Chamfer backward.
There is no CPU path."""
import math

import torch

from .._lib import lib, check, current_stream
from .StructuralLosses import StructuralLossesBackend as BK


def _scalars(alpha, n_lambda, who):
    alpha, n_lambda = float(alpha), float(n_lambda)
    if not (alpha > 0.0 and math.isfinite(alpha)):
        raise ValueError("%s: alpha must be positive and finite, got %r" % (who, alpha))
    if not (n_lambda >= 0.0 and math.isfinite(n_lambda)):
        raise ValueError("%s: n_lambda must be non-negative and finite, got %r" % (who, n_lambda))
    return alpha, n_lambda


def _need(t, dtype, shape, name, who):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.is_contiguous()):
        raise RuntimeError("%s needs contiguous CUDA tensors dist (B, n) float32 and idx (B, n) int32, as NNDistance returns them (%s is "
                           "not); there is no CPU path" % (who, name))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: %s must have shape %s, got %s" % (who, name, tuple(shape), tuple(t.shape)))


def density_aware_chamfer_raw(dist1, idx1, dist2, idx2, alpha=1000.0, n_lambda=1.0, non_reg=False, form=0):
    """(loss (B,) float64, halves (B, 2) float64, count1 (B, n) int32, count2 (B, m) int32, coef1 (B, n) fp32, coef2 (B, m) fp32,
    status (B,) int32) of dpf_dcd on one nn_distance result: no look at the statuses, no synchronisation.  form: 0 by size, 1 the
    one-workgroup form, 2 the workspace form (the same bits)."""
    who = "density_aware_chamfer_raw"
    alpha, n_lambda = _scalars(alpha, n_lambda, who)
    _need(dist1, torch.float32, None, "dist1", who)
    B, n = dist1.shape
    _need(dist2, torch.float32, None, "dist2", who)
    m = dist2.shape[1]
    _need(dist2, torch.float32, (B, m), "dist2", who)
    _need(idx1, torch.int32, (B, n), "idx1", who)
    _need(idx2, torch.int32, (B, m), "idx2", who)
    if n < 1 or m < 1:
        raise ValueError("%s: no points" % who)
    if form not in (0, 1, 2):
        raise ValueError("%s: form must be 0 (by size), 1 or 2, got %r" % (who, form))
    dev = dist1.device
    if any(t.device != dev for t in (idx1, dist2, idx2)):
        raise RuntimeError("%s: the four tensors lie on different devices" % who)
    loss = torch.empty((B,), dtype=torch.float64, device=dev)
    halves = torch.empty((B, 2), dtype=torch.float64, device=dev)
    count1 = torch.empty((B, n), dtype=torch.int32, device=dev)
    count2 = torch.empty((B, m), dtype=torch.int32, device=dev)
    coef1 = torch.empty((B, n), dtype=torch.float32, device=dev)
    coef2 = torch.empty((B, m), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            nbytes = lib().dpf_dcd_workspace_bytes(B, n, m)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            check(lib().dpf_dcd(B, n, m, dist1.data_ptr(), idx1.data_ptr(), dist2.data_ptr(), idx2.data_ptr(), alpha, n_lambda,
                                int(bool(non_reg)), int(form), loss.data_ptr(), halves.data_ptr(), count1.data_ptr(), count2.data_ptr(),
                                coef1.data_ptr(), coef2.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "dcd")
    return loss, halves, count1, count2, coef1, coef2, status


def _dcd_check(status, what):
    """ValueError naming the first refused cloud (reads the statuses: a device synchronisation)"""
    bad = torch.nonzero(status < 0)
    if bad.numel():
        raise ValueError("%s: cloud %d of %d refused (a nearest-neighbour index outside the other cloud); %d refused in all"
                         % (what, int(bad[0, 0]), status.numel(), bad.shape[0]))


def _grad(x, y, idx1, idx2, gd1, gd2, need_x, need_y):
    """NNDistanceGrad(deterministic=True) for the gradients that are asked for alone"""
    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    gx = torch.empty((b, n, 3), dtype=torch.float32, device=x.device) if need_x else None
    gy = torch.empty((b, m, 3), dtype=torch.float32, device=x.device) if need_y else None
    with torch.cuda.device(x.device):
        ws, wsp, nbytes = BK._grad_scratch(b, n, m, x.device)
        check(lib().dpf_nndistancegrad_det(b, n, x.data_ptr(), m, y.data_ptr(), gd1.data_ptr(), idx1.data_ptr(), gd2.data_ptr(),
                                           idx2.data_ptr(), gx.data_ptr() if need_x else None, gy.data_ptr() if need_y else None,
                                           wsp, nbytes, current_stream()), "nndistancegrad_det")
    return gx, gy


class _DensityAwareChamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, alpha, n_lambda, non_reg):
        dist1, idx1, dist2, idx2 = BK.NNDistance(x, y)
        loss, halves, count1, count2, coef1, coef2, status = density_aware_chamfer_raw(dist1, idx1, dist2, idx2, alpha, n_lambda, non_reg)
        _dcd_check(status, "density_aware_chamfer")
        ctx.save_for_backward(x, y, idx1, idx2, coef1, coef2)
        for t in (halves, count1, count2, idx1, idx2):
            ctx.mark_non_differentiable(t)
        return loss.to(torch.float32), halves, count1, count2, idx1, idx2

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None, None, None, None
        x, y, idx1, idx2, coef1, coef2 = ctx.saved_tensors
        g = grad_loss.to(torch.float32)
        gx, gy = _grad(x, y, idx1, idx2, (g[:, None] * coef1).contiguous(), (g[:, None] * coef2).contiguous(), need_x, need_y)
        return gx, gy, None, None, None


def density_aware_chamfer(x, y, alpha=1000.0, n_lambda=1.0, non_reg=False, return_raw=False):
    """(B,) fp32 density-aware Chamfer distance of cloud b of x (B, n, 3) against cloud b of y (B, m, 3), n != m served:
    loss = (L1 + L2) / 2 with L1 = mean_i (1 - exp(-alpha d1[i]) * (n / m) / (c1[i]^n_lambda + 1e-6)), d1[i] the squared distance of
    x's point i to its nearest point of y and c1[i] the number of x's points that share that nearest point; L2 the same with x and y
    swapped.  non_reg clamps the two size ratios at 1 from below.  Float64 sums in a fixed order, one rounding to fp32.

    x, y: contiguous float32 CUDA tensors; a CPU tensor raises RuntimeError.  One autograd node: the forward is NNDistance and one
    dpf_dcd launch, the backward NNDistanceGrad(deterministic=True) with grad_dist1 = grad[:, None] * coef1 and grad_dist2 likewise
    -- the weights are constants, as the published loss detaches them -- computing only the gradients asked for, the same bits on
    every run.  A refused cloud (an index outside the other cloud: only a search gone wrong gives one) raises ValueError naming the
    first; looking at the statuses synchronises with the device.
    return_raw: also (halves (B, 2) float64 = L1, L2; count1 (B, n), count2 (B, m) int32; idx1 (B, n), idx2 (B, m) int32)."""
    alpha, n_lambda = _scalars(alpha, n_lambda, "density_aware_chamfer")
    for t, name in ((x, "x"), (y, "y")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3):
            raise RuntimeError("density_aware_chamfer needs float32 CUDA tensors of shape (B, n, 3) (%s is not); there is no CPU path" % name)
    if x.shape[0] != y.shape[0] or x.device != y.device:
        raise RuntimeError("density_aware_chamfer pairs cloud b of x with cloud b of y on one device, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if x.shape[1] < 1 or y.shape[1] < 1:
        raise ValueError("density_aware_chamfer: no points")
    out = _DensityAwareChamfer.apply(x, y, alpha, n_lambda, bool(non_reg))
    return (out[0], out[1:]) if return_raw else out[0]


def pairwise_DCD(clouds1, clouds2, bs=2048, alpha=1000.0, n_lambda=1.0, non_reg=False):
    """(N1, N2) fp32 matrix of density_aware_chamfer of every cloud of clouds1 (N1, n, 3) against every cloud of clouds2 (N2, m, 3),
    no autograd.  The pairs are served in row-major order, at most bs of them per batched call; what is kept beyond a chunk is the
    matrix alone.  Entry (i, j) has the bits of the single call on clouds1[i], clouds2[j]."""
    bs = int(bs)
    if bs < 1:
        raise ValueError("pairwise_DCD: bs must be at least 1, got %d" % bs)
    N1, N2 = clouds1.shape[0], clouds2.shape[0]
    with torch.no_grad():
        out = torch.empty((N1 * N2,), dtype=torch.float32, device=clouds1.device)
        for p0 in range(0, N1 * N2, bs):
            pair = torch.arange(p0, min(N1 * N2, p0 + bs), device=clouds1.device)
            rows, cols = torch.div(pair, N2, rounding_mode="floor"), pair % N2
            out[p0:p0 + bs] = density_aware_chamfer(clouds1.index_select(0, rows), clouds2.index_select(0, cols), alpha, n_lambda, non_reg)
        return out.view(N1, N2)
