"""Host driver of the eval-mode (frozen BatchNorm) autograd path of the latent prior flow (csrc/gprior_frozen.hip).

Under model.eval() the reference's GlobalRNVPDecoder / RealNVPFlowCouple / RealNVPFlow (lib/networks/flows.py:198-243,
decoders.py:21-38) are differentiable with respect to g and every parameter.  With `eval_autograd = "hip"` such a call is ONE
autograd node for the whole stack (`_GPriorFrozen` / `_GPriorFrozenFlat`, modelled on prior_flows' training nodes):

  forward   the fused eval launch itself (GPriorStack.run: dpf_gprior_forward, csrc/gprior.hip) -- the outputs are those of a
            no_grad call, bit for bit; nothing else is saved, the backward recomputes the hidden activations;
  backward  dpf_gprior_frozen_backward: two launches whatever the number of steps (a row-parallel walk of the steps in reverse,
            then every parameter gradient as a fixed-order sum over the rows).

The BatchNorm buffers are read, never written.  B = 1 is legal."""
import torch

from .._lib import lib, check, current_stream, MODE
from .layers import scatter_param_grads


def _forward(stack, g, mode):
    with torch.no_grad():
        _, sum_lv, gs, mus, lvs = stack.run(g, mode)
    return gs, mus, lvs, sum_lv


def _backward(cfg, canon, params_only, stats, g, gs, mus, lvs, grads):
    """-> (dL/dg, the gradient block in the layout of `canon`)."""
    mode, codes, (S, G, nf), bn_eps, eps = cfg
    d_gs, d_mus, d_lvs, d_sum = grads
    B, dev, L_ = g.shape[0], g.device, lib()
    if B == 0:
        return torch.zeros_like(g), torch.zeros_like(canon)
    if d_sum is not None:                                        # d/d(layer-sum) reaches every step's log-variances
        d_lvs = d_sum.expand(S, B, G) if d_lvs is None else d_lvs + d_sum
    cg = [t.contiguous() if t is not None else None for t in (d_gs, d_mus, d_lvs)]      # alive across the call
    with torch.cuda.device(dev):
        dg, dcanon = torch.empty_like(g), torch.empty_like(canon)
        ws = torch.empty(L_.dpf_gprior_frozen_workspace_floats(S, B, G, nf), dtype=torch.float32, device=dev)
        check(L_.dpf_gprior_frozen_backward(S, B, G, nf, MODE[mode], codes, params_only, canon.data_ptr(),
                                            stats.data_ptr() if stats is not None else None, bn_eps, eps, g.data_ptr(), gs.data_ptr(),
                                            mus.data_ptr(), lvs.data_ptr(), *[t.data_ptr() if t is not None else None for t in cg],
                                            dg.data_ptr(), dcanon.data_ptr(), ws.data_ptr(), current_stream()),
              "gprior_frozen_backward")
    return dg, dcanon


class _GPriorFrozen(torch.autograd.Function):
    """The whole eval-mode stack as one node: inputs g and every parameter, outputs the three (S,B,G) blocks and the layer-sum of
    the log-variances.  The backward reads the canonical block the forward's weights were packed from."""

    @staticmethod
    def forward(ctx, g, stack, cfg, slots, *params):
        g = g.contiguous()
        gs, mus, lvs, sum_lv = _forward(stack, g, cfg[0])
        ctx.save_for_backward(g, stack.canon, gs, mus, lvs, *params)
        ctx.cfg, ctx.slots = cfg, slots
        ctx.set_materialize_grads(False)
        return gs, mus, lvs, sum_lv

    @staticmethod
    def backward(ctx, *grads):
        g, canon, gs, mus, lvs = ctx.saved_tensors[:5]
        params = ctx.saved_tensors[5:]
        dg, dcanon = _backward(ctx.cfg, canon, 0, None, g, gs, mus, lvs, grads)
        pgrads = scatter_param_grads(dcanon, ctx.slots, params, ctx.needs_input_grad[4:])
        return (dg if ctx.needs_input_grad[0] else None, None, None, None, *pgrads)


class _GPriorFrozenFlat(torch.autograd.Function):
    """The same over a PriorFlatStore: autograd sees g and a token; the kernels read flat_p in place (the parameters-only layout)
    and the running statistics as a block of their own; the parameter gradients are added to flat_g."""

    @staticmethod
    def forward(ctx, g, token, store, stack, cfg):
        g = g.contiguous()
        gs, mus, lvs, sum_lv = _forward(stack, g, cfg[0])
        S, G, nf = cfg[2]
        at = nf * (G // 2) + 2 * nf                              # running_mean | running_var of a net inside the canonical block
        stats = stack.canon.view(2 * S, -1)[:, at:at + 2 * nf].contiguous()
        ctx.save_for_backward(g, stats, gs, mus, lvs)
        ctx.cfg = (store, cfg, store.flat_p._version)
        ctx.set_materialize_grads(False)
        return gs, mus, lvs, sum_lv

    @staticmethod
    def backward(ctx, *grads):
        g, stats, gs, mus, lvs = ctx.saved_tensors
        store, cfg, version = ctx.cfg
        if store.flat_p._version != version:
            raise RuntimeError("the flattened parameters were modified in place between forward and backward")
        dg, dcanon = _backward(cfg, store.flat_p, 1, stats, g, gs, mus, lvs, grads)
        store.accumulate(dcanon)
        return (dg if ctx.needs_input_grad[0] else None, None, None, None, None)


def run_frozen_prior(stack, store, params, slots, cfg, g):
    """Eval-mode forward of the steps of `stack` attached to autograd through the HIP backward: (gs, mus, lvs) blocks (S,B,G) in
    DIRECT order and the layer-sum of the log-variances (B,G).  store: the attached PriorFlatStore whose parameters are being
    trained, or None."""
    with torch.cuda.device(g.device):
        if store is not None:
            return _GPriorFrozenFlat.apply(g, store.token, store, stack, cfg)
        return _GPriorFrozen.apply(g, stack, cfg, slots, *params)
