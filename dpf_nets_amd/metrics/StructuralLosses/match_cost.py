"""match_cost(seta (B,n,3), setb (B,m,3)) -> cost (B,): approximate EMD.
Mirror of lib/metrics/pytorch_structural_losses/match_cost.py:6-44 (the matching
is a constant in backward, :38-42).

The (B, m, n) matching is written only where something will read it: a call whose backward cannot run (grad mode off, or no
input requires grad -- the reference's only call path, evaluation_metrics.py:26-31) takes the cost-only forward, same bits of
the cost.  A call whose backward will run stores the matching as before; match_cost_lean (or the switch
StructuralLossesBackend.EMD_LEAN_GRAD / env DPF_EMD_LEAN_GRAD=1, which routes match_cost itself) never stores it: its backward
rebuilds the weights from the forward's workspace."""
import torch

from . import StructuralLossesBackend as BK
from .StructuralLossesBackend import ApproxMatch, ApproxMatchCost, MatchCost, MatchCostGrad  # noqa: F401
from .StructuralLossesBackend import ApproxMatchCostOnly, MatchCostGradRecompute  # noqa: F401


def _backward_can_run(seta, setb):
    return torch.is_grad_enabled() and (seta.requires_grad or setb.requires_grad)


def _scaled(grad, go, needed):
    return grad.mul_(go) if needed else None          # (the kernels' fresh outputs: scaled in place)


class MatchCostFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seta, setb, backward_can_run=None):
        # (inside forward grad mode is always off: match_cost looks before it calls; a direct .apply(seta, setb) falls back on
        # the inputs' flags)
        if backward_can_run is None:
            backward_can_run = any(ctx.needs_input_grad[:2])
        if not backward_can_run and not BK.EMD_RMW:
            return ApproxMatchCostOnly(seta, setb)[1]
        ctx.save_for_backward(seta, setb)
        match, _temp, cost = ApproxMatchCost(seta, setb)        # = ApproxMatch, then MatchCost (match_cost.py:20-22)
        ctx.match = match
        return cost

    @staticmethod
    def backward(ctx, grad_output):
        seta, setb = ctx.saved_tensors
        grada, gradb = MatchCostGrad(seta, setb, ctx.match)
        go = grad_output.unsqueeze(1).unsqueeze(2)
        return _scaled(grada, go, ctx.needs_input_grad[0]), _scaled(gradb, go, ctx.needs_input_grad[1]), None


class MatchCostLeanFunction(torch.autograd.Function):
    """match_cost without a stored matching, forward and backward.

    Forward: the cost-only entry; the cost has the bits of match_cost's.  Saved for backward: the two clouds and the forward's
    workspace (dpf_approxmatch_workspace_bytes: ~ 36 (n + m) + 16 (n + 2 m) + 48 m + 64 n + 350 m bytes per cloud pair), instead
    of 4 n m bytes of matching.  Backward: the materialising pass runs again with the saved state and adds every entry's term
    to both gradients in registers -- zero bytes of `match` moved in either direction; read: the workspace's records and ratio
    vectors; written and read once more: grad2's per-64-column partial sums (12 bytes per column block and row, 3 / (16 n) of the
    matching).  The weights are the stored path's bits; the gradients differ from match_cost's by fp32 summation order only
    (tests/test_gpu_emd_lean.py: rtol 1e-4, atol 1e-5).  Deterministic; the saved workspace is only read, so the graph can be
    walked twice.
    Measured on MI355X (tools/emd_lean_bench.py; forward + backward, lean / stored, best of 5, run-to-run spread
    0.03-0.10): 0.90 at B = 16, n = 8192 (3.36 vs 3.75 ms), 0.89 at B = 32, n = 2048 (1.10 vs 1.23 ms), 1.08 at B = 64, n = 8192
    (15.8 vs 14.7 ms); peak allocation 0.28 / 0.06 / 1.1 GB against 4.4 / 0.58 / 17.5 GB."""

    @staticmethod
    def forward(ctx, seta, setb, backward_can_run=None):
        if backward_can_run is None:
            backward_can_run = any(ctx.needs_input_grad[:2])
        _temp, cost, saved = ApproxMatchCostOnly(seta, setb)
        if backward_can_run:
            ctx.save_for_backward(seta, setb, saved)
        return cost

    @staticmethod
    def backward(ctx, grad_output):
        seta, setb, saved = ctx.saved_tensors
        grada, gradb = MatchCostGradRecompute(seta, setb, saved)
        go = grad_output.unsqueeze(1).unsqueeze(2)
        return _scaled(grada, go, ctx.needs_input_grad[0]), _scaled(gradb, go, ctx.needs_input_grad[1]), None


def match_cost_lean(seta, setb):
    """match_cost that never stores the matching (MatchCostLeanFunction)."""
    return MatchCostLeanFunction.apply(seta, setb, _backward_can_run(seta, setb))


def match_cost(seta, setb):
    can = _backward_can_run(seta, setb)
    if BK.EMD_LEAN_GRAD and not BK.EMD_RMW:
        return MatchCostLeanFunction.apply(seta, setb, can)
    return MatchCostFunction.apply(seta, setb, can)
