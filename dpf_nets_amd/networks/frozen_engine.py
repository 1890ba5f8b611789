"""Host driver of the eval-mode (frozen BatchNorm) autograd path of the coupling stack (csrc/flow_frozen.hip).

Under model.eval() the reference's CondRealNVPFlow3D.forward (lib/networks/flows.py:95-117) is differentiable with respect to
p, g and every parameter.  With `eval_autograd = "hip"` on the module such a call is ONE autograd node for the whole stack
(`_FlowStackFrozen` / `_FlowStackFrozenFlat`, modelled on train_engine's training nodes):

  forward   the fused eval stack itself (engine.FlowStack.run with the per-layer lists: one launch, csrc/flow.hip) -- the
            outputs are those of a no_grad call, bit for bit; next to it the K = 4 L per-cloud FiLM nets once more with the running
            statistics, whose activations the backward needs: one launch of dpf_film_frozen_forward (csrc/film_train.hip; B > 64
            or G % 4 != 0: batched tensor ops);
  backward  dpf_flow_frozen_backward_lists: per layer, in reverse order, one recompute-and-differentiate launch over the points
            and one reduction of its per-workgroup partial rows (no statistic pass: with frozen statistics a layer is a
            per-point map); then the FiLM nets' backward, one launch of dpf_film_frozen_backward (du = rstd * gamma * dy: no mean
            terms; d g summed over the K nets in a fixed order inside the launch), or batched tensor ops outside its limits.

The BatchNorm buffers are read, never written.  B = 1 is legal."""
import torch

from .._lib import lib, check, current_stream, PREC, MODE
from .flowlist import tag_layer_sum
from .layers import scatter_param_grads
from .train_engine import F, _T_BR, _grad_table

def cuda_fp32(*tensors):                      # what the kernels of this path serve (backend.frozen_asked: what the call asks for)
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def film_frozen_ok(B, G, *blocks):
    """The fused frozen FiLM kernels take 1 <= B <= 64 clouds, G % 4 == 0 and contiguous fp32 blocks."""
    return 1 <= B <= lib().dpf_film_train_max_batch() and G % 4 == 0 and \
        all(t.is_contiguous() and t.dtype == torch.float32 for t in blocks)


def _film_forward(g, W0, gam, bet, W1, b1, rm, rstd):
    """The K conditioner nets with frozen BatchNorm: Lin(G -> F), (u - running_mean) * rstd * gamma + beta, swish, Lin(F -> F) + b."""
    u = torch.matmul(g.unsqueeze(0), W0.transpose(1, 2))               # (K, B, F)
    xhat = (u - rm) * rstd
    y = xhat * gam + bet
    sig = torch.sigmoid(y)
    sw = y * sig
    return torch.baddbmm(b1, sw, W1.transpose(1, 2)), xhat, y, sig, sw


def _film_backward(dfm, g, W0, gam, W1, rstd, xhat, y, sig, sw, need_dg):
    dout = dfm
    db1 = dout.sum(1)
    dW1 = torch.matmul(dout.transpose(1, 2), sw)                       # (K, F, F)
    dy = torch.matmul(dout, W1) * (sig * (1.0 + y * (1.0 - sig)))
    dgam = (dy * xhat).sum(1)
    dbet = dy.sum(1)
    du = dy * (gam * rstd)                                             # frozen statistics: no mean-correction terms
    dW0 = torch.matmul(du.transpose(1, 2), g.unsqueeze(0))             # (K, F, G)
    dg = torch.bmm(du, W0).sum(0) if need_dg else None                 # K small products and one sum over K (train_engine)
    return dW0, dgam, dbet, dW1, db1, dg


def _frozen_stats(spec, dev):
    """(L, 2, 4, F) running_mean0 | running_var0 | running_mean1 | running_var1 of the conditioner stacks, and the FiLM nets'
    (K, 1, F) running mean and 1 / sqrt(running_var + eps)."""
    L = spec.L
    bns = spec.flow_bns()
    rm = torch.stack([b.running_mean for b in bns]).view(L, 2, 2, F)
    rv = torch.stack([b.running_var for b in bns]).view(L, 2, 2, F)
    fstats = torch.stack([rm[:, :, 0], rv[:, :, 0], rm[:, :, 1], rv[:, :, 1]], dim=2).to(device=dev, dtype=torch.float32).contiguous()
    fbns = [m[1] for m in spec.film_modules()]
    frm = torch.stack([b.running_mean for b in fbns]).unsqueeze(1).float()
    frv = torch.stack([b.running_var for b in fbns]).unsqueeze(1).float()
    return fstats, frm, frv, float(fbns[0].eps)


def _forward_core(stack, spec, p, g, mode, precision, tcanon, W0, gam, bet, W1, b1):
    L = spec.L
    B = p.shape[0]
    # (detached: at::matmul folds its batch dimensions differently for an operand that requires grad -- other GEMM shapes, other
    # roundings; the FiLM vectors must not depend on WHICH input the caller differentiates)
    p, g = p.detach(), g.detach()
    K, G, dev = 4 * L, spec.G, p.device
    with torch.no_grad():
        fstats, frm, frv, bn_eps = _frozen_stats(spec, dev)
        if film_frozen_ok(B, G, g, W0, gam, bet, W1, b1, frm, frv):
            fm = torch.empty((L, 2, 2, B, F), dtype=torch.float32, device=dev)
            xhat = torch.empty((K, B, F), dtype=torch.float32, device=dev)
            frstd = torch.empty((K, 1, F), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                check(lib().dpf_film_frozen_forward(K, B, G, g.data_ptr(), W0.data_ptr(), gam.data_ptr(), bet.data_ptr(), W1.data_ptr(),
                                                    b1.data_ptr(), frm.data_ptr(), frv.data_ptr(), bn_eps, fm.data_ptr(), xhat.data_ptr(),
                                                    frstd.data_ptr(), current_stream()), "film_frozen_forward")
            y = sig = sw = None
        else:                                                          # batched tensor ops (B > 64, G % 4 != 0)
            frstd = torch.rsqrt(frv + bn_eps)
            fm, xhat, y, sig, sw = _film_forward(g, W0, gam, bet, W1, b1, frm, frstd)
            fm = fm.view(L, 2, 2, B, F).contiguous()
        p_out, sum_lv, ps, mus, lvs = stack.run(p, g, mode, precision, want_lists=True, n_layers=L)
        if stack.last_precision != "f16x3":
            raise RuntimeError("eval_autograd='hip' differentiates the f16x3 stack only (got %s)" % stack.last_precision)
    outs = ps.unbind(0) + mus.unbind(0) + lvs.unbind(0) + (sum_lv,)
    saved = (p, g, tcanon, fstats, stack.last_packed, stack.last_film, fm, ps, mus, lvs, W0, gam, bet, W1, frstd, xhat, y, sig, sw)
    return outs, saved


N_SAVED = 19


def _backward_core(spec, mode, saved, grads, need_dg, into_flat=False):
    """-> (dL/dp, dL/dg, d canon block, dW0, dgamma, dbeta, dW1, db1); the last five are None when the fused FiLM backward has
    added them to the flat store's gradient blocks itself (into_flat)."""
    p_in, g, tcanon, fstats, packed, film, fm, ps, mus, lvs, W0, gam, bet, W1, frstd, xhat, y, sig, sw = saved
    L = spec.L
    B, _, N = p_in.shape
    dev = p_in.device
    g = g.detach()
    L_ = lib()
    with torch.cuda.device(dev):
        ws = torch.empty(L_.dpf_flow_frozen_workspace_bytes(B, N), dtype=torch.uint8, device=dev)
        dcanon = torch.empty_like(tcanon)
        dfm = torch.empty((L, 2, 2, B, F), dtype=torch.float32, device=dev)
        keep = {}
        g_lvs = grads[2 * L:3 * L]
        if grads[3 * L] is not None:                            # d/d(layer-sum) reaches every layer's log-variances
            dtot = grads[3 * L]
            g_lvs = [dtot if t is None else t + dtot for t in g_lvs]
        t_ps, t_mus = (_grad_table(grads[i * L:(i + 1) * L], tuple(p_in.shape), keep) for i in range(2))
        t_lvs = _grad_table(g_lvs, tuple(p_in.shape), keep)
        chain, dp_tmp = torch.empty_like(p_in), torch.empty_like(p_in)
        check(L_.dpf_flow_frozen_backward_lists(L, B, N, MODE[mode], PREC["f16x3"], spec.meta_host, tcanon.data_ptr(),
                                                fstats.data_ptr(), packed.data_ptr(), film.data_ptr(), fm.data_ptr(),
                                                p_in.data_ptr(), ps.data_ptr(), mus.data_ptr(), lvs.data_ptr(), t_ps, t_mus, t_lvs,
                                                chain.data_ptr(), dp_tmp.data_ptr(), dcanon.data_ptr(), dfm.data_ptr(), spec.eps,
                                                ws.data_ptr(), current_stream()), "flow_frozen_backward_lists")
        del keep
        K, G = 4 * L, spec.G
        if y is None:                                                  # the forward took the fused kernel: so does the backward
            into = spec.flat.film_grad_blocks() if into_flat else None
            if into is None:
                dW0, dW1 = torch.empty_like(W0), torch.empty_like(W1)
                dgam, dbet, db1 = (torch.empty((K, F), dtype=torch.float32, device=dev) for _ in range(3))
            else:
                dW0, dgam, dbet, dW1, db1 = into
            dg = work = None
            ticket = spec._dev_cache.get(("film_ticket", dev))
            if ticket is None:                                         # one word, zero between calls (the kernel leaves it zero)
                ticket = spec._dev_cache[("film_ticket", dev)] = torch.zeros(1, dtype=torch.int32, device=dev)
            if need_dg:
                dg = torch.empty((B, G), dtype=torch.float32, device=dev)
                work = torch.empty(L_.dpf_film_frozen_workspace_floats(K, B, G), dtype=torch.float32, device=dev)
            check(L_.dpf_film_frozen_backward(K, B, G, g.data_ptr(), W0.data_ptr(), gam.data_ptr(), bet.data_ptr(), W1.data_ptr(),
                                              xhat.data_ptr(), frstd.data_ptr(), dfm.data_ptr(), dW0.data_ptr(), dgam.data_ptr(),
                                              dbet.data_ptr(), dW1.data_ptr(), db1.data_ptr(), dg.data_ptr() if need_dg else None,
                                              work.data_ptr() if need_dg else None, ticket.data_ptr(), 1 if into is not None else 0,
                                              current_stream()), "film_frozen_backward")
            if into is not None:
                return chain, dg, dcanon, None, None, None, None, None
            return chain, dg, dcanon, dW0, dgam, dbet, dW1, db1
        dW0, dgam, dbet, dW1, db1, dg = _film_backward(dfm.view(K, B, F), g, W0, gam, W1, frstd, xhat, y, sig, sw, need_dg)
    return chain, dg, dcanon, dW0, dgam, dbet, dW1, db1


class _FlowStackFrozen(torch.autograd.Function):
    """The eval-mode stack as one node whose inputs are p, g and all 32 * L parameters."""

    @staticmethod
    def forward(ctx, p, g, stack, spec, mode, precision, *params):
        L, G = spec.L, spec.G
        p, g = p.contiguous(), g.contiguous()
        ncanon = len(spec.canon_slots)
        cparams, fparams = params[:ncanon], params[ncanon:]
        zeros = spec.zeros_on(p.device)
        tcanon = torch.cat([cparams[i].reshape(-1) if kind == "p" else zeros[:i] for kind, i in spec.cat_plan]).view(L, 2 * _T_BR)
        K = 4 * L
        W0 = torch.cat([t.reshape(-1) for t in fparams[0::5]]).view(K, F, G)
        gam = torch.cat(fparams[1::5]).view(K, 1, F)
        bet = torch.cat(fparams[2::5]).view(K, 1, F)
        W1 = torch.cat([t.reshape(-1) for t in fparams[3::5]]).view(K, F, F)
        b1 = torch.cat(fparams[4::5]).view(K, 1, F)
        outs, saved = _forward_core(stack, spec, p, g, mode, precision, tcanon, W0, gam, bet, W1, b1)
        ctx.save_for_backward(*saved, *params)
        ctx.spec, ctx.mode = spec, mode
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        saved, params = ctx.saved_tensors[:N_SAVED], ctx.saved_tensors[N_SAVED:]
        spec = ctx.spec
        chain, dg, dcanon, dW0, dgam, dbet, dW1, db1 = _backward_core(spec, ctx.mode, saved, grads, ctx.needs_input_grad[1])
        flat = dcanon.view(-1)
        views = [flat[o:o + n] for o, n in spec.canon_slots]
        for k in range(4 * spec.L):
            views += [dW0[k], dgam[k], dbet[k], dW1[k], db1[k]]
        pgrads = scatter_param_grads(views, None, params, ctx.needs_input_grad[6:])
        return (chain if ctx.needs_input_grad[0] else None, dg, None, None, None, None, *pgrads)


class _FlowStackFrozenFlat(torch.autograd.Function):
    """The same over a FlatStore: autograd sees p, g and a token; the parameter gradients are added to the store's twin buffer."""

    @staticmethod
    def forward(ctx, p, g, token, stack, spec, mode, precision):
        outs, saved = _forward_core(stack, spec, p.contiguous(), g.contiguous(), mode, precision, *spec.flat.blocks)
        ctx.save_for_backward(*saved)
        ctx.spec, ctx.mode = spec, mode
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        spec = ctx.spec
        chain, dg, *dparams = _backward_core(spec, ctx.mode, ctx.saved_tensors, grads, ctx.needs_input_grad[1], into_flat=True)
        spec.flat.accumulate(*dparams)
        return (chain if ctx.needs_input_grad[0] else None, dg, None, None, None, None, None)


def run_frozen_stack(stack, spec, p, g, mode, precision=None):
    """Eval-mode forward of the layers of `spec` (= those of the FlowStack `stack`, DIRECT order), attached to autograd through
    the HIP backward.
    Returns (ps, mus, lvs): three lists of L (B,3,N) tensors in DIRECT order."""
    if p.dim() != 3 or p.shape[1] != 3 or g.dim() != 2 or g.shape[0] != p.shape[0]:
        raise RuntimeError("expected p (B,3,N) and g (B,G)")
    if g.shape[1] != spec.G:
        raise RuntimeError("g has %d features, the layers expect %d" % (g.shape[1], spec.G))
    with torch.cuda.device(p.device):
        # the flat node adds to flat_g whatever requires grad (its token always does): with every parameter frozen (latent
        # optimisation over a flattened decoder) the per-parameter node is taken, which forms no parameter gradient -- flat_g and
        # grad_written stay as they are, as in the prior flow (prior_flows._frozen_prior)
        if spec.flat is not None and spec.flat.attached() and any(t.requires_grad for t in spec.flat.params):
            outs = _FlowStackFrozenFlat.apply(p, g, spec.flat.token, stack, spec, mode, precision)
        else:
            outs = _FlowStackFrozen.apply(p, g, stack, spec, mode, precision, *spec.all_params())
    L = spec.L
    return list(outs[:L]), list(outs[L:2 * L]), tag_layer_sum(list(outs[2 * L:3 * L]), outs[3 * L])


def frozen_precision_ok(stack, spec, precision, device):
    """The frozen backward recomputes the f16x3 stack (the default); any other operand format, or weights outside f16x3's exact
    range, is served by tensor operations.  When parameters require grad (fine-tuning) the packed weights AND the range verdict
    are refreshed first, on every call: an optimizer may move the parameters behind the version counters' back (updates through
    .data), and a stack that has drifted out of range must fall back here, not run.  The verdict costs a host round trip."""
    from .engine import DEFAULT_PRECISION
    if (precision or DEFAULT_PRECISION) != "f16x3":
        return False
    if any(t.requires_grad for t in spec.all_params()):
        stack.invalidate()
    with torch.cuda.device(device):
        return stack._ensure("f16x3", device, spec.L)[4] == "f16x3"
