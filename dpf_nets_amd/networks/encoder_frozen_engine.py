"""Host driver of the eval-mode (frozen BatchNorm) autograd path of the PointNet cloud encoder (csrc/encoder_frozen.hip).

Under model.eval() the reference's PointNetCloudEncoder followed by the max over the points (lib/networks/encoders.py:15-28,
models.py:106,124) is differentiable with respect to the cloud and the twelve parameters.  With `eval_autograd = "hip"` such a call
is ONE autograd node (`_FrozenPool`; the glue it shares with the two flow paths is in networks/layers.py):

  forward   the fused eval launch with the argmax switched on (dpf_encoder_forward_arg, csrc/encoder.hip) -- pooled has the bits
            of a no_grad call; saved: x, the canonical block, pooled and the (B,512) argmax, nothing per point;
  backward  dpf_encoder_frozen_backward: four launches for the parameter gradients, six with dx, whatever B and N are -- the
            B * 512 argmax points are recomputed through layers 0-2 with the forward's fragments and differentiated from there.

The BatchNorm buffers are read, never written.  B = 1 and N = 1 are legal."""
import torch

from .._lib import lib, check, current_stream, PREC
from .layers import scatter_param_grads

FROZEN_PRECISIONS = ("bf16x3", "bf16x6")


def frozen_params(enc):
    """W, gamma, beta of the four layers, in the order of the canonical block"""
    out = []
    for name in ("init_sd", "sd0", "sd1", "sd2"):
        sd, bn = getattr(enc.features, name), getattr(enc.features, name + "_bn")
        out += [sd.weight, bn.weight, bn.bias]
    return out


def frozen_slots(enc):
    """(offset, numel) of frozen_params in the canonical block (per layer W | gamma | beta | running_mean | running_var), once per module"""
    slots = enc.__dict__.get("_frozen_slots")
    if slots is None:
        slots, off, cin = enc.__dict__.setdefault("_frozen_slots", []), 0, enc.init_n_channels
        for cout in (enc.init_n_features, *enc.n_features):
            for n in (cout * cin, cout, cout):
                slots.append((off, n))
                off += n
            off += 2 * cout                                               # the running-statistics slots
            cin = cout
        assert off == lib().dpf_encoder_canon_floats(), off
    return slots


def frozen_hip_serves(enc, x):
    """What the kernels serve (backend.frozen_asked: what the call asks for): the 3 -> 64 -> [128, 256, 512] architecture, CUDA fp32 (B,3,N), bf16x3 or bf16x6."""
    ts = enc._layer_tensors()
    return enc.hip_supported() and enc.precision in FROZEN_PRECISIONS and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 \
        and x.shape[1] == 3 and x.shape[2] >= 1 and x.shape[0] <= 65535 \
        and all(t is not None and t.dtype == torch.float32 and t.device == x.device for t in ts)


class _FrozenPool(torch.autograd.Function):
    """pooled = max over the points of the eval-mode encoder; inputs x and W, gamma, beta of the four layers."""

    @staticmethod
    def forward(ctx, enc, x, *params):
        B, _, N = x.shape
        dev, L_, prec = x.device, lib(), PREC[enc.precision]
        with torch.cuda.device(dev):
            canon = torch.cat([t.detach().reshape(-1) for t in enc._layer_tensors()]).contiguous()
            if any(p.requires_grad for p in params):
                # optimizers write through .data, which moves no version counter: parameters in training are packed per call
                packed = torch.empty(L_.dpf_encoder_packed_bytes(prec), dtype=torch.uint8, device=dev)
                check(L_.dpf_encoder_pack(prec, canon.data_ptr(), packed.data_ptr(), current_stream()), "encoder_pack")
            else:
                packed = enc._packed(dev)
            pooled = torch.empty((B, enc.n_features[-1]), dtype=torch.float32, device=dev)
            arg = torch.empty((B, enc.n_features[-1]), dtype=torch.int32, device=dev)
            if B > 0:
                scratch = torch.empty(L_.dpf_encoder_arg_scratch_bytes(B), dtype=torch.uint8, device=dev)
                check(L_.dpf_encoder_forward_arg(B, N, prec, packed.data_ptr(), x.data_ptr(), pooled.data_ptr(), arg.data_ptr(),
                                                 scratch.data_ptr(), current_stream()), "encoder_forward_arg")
        ctx.save_for_backward(x, canon, packed, pooled, arg)
        ctx.prec, ctx.shapes, ctx.slots = prec, [p.shape for p in params], frozen_slots(enc)
        ctx.set_materialize_grads(False)
        return pooled

    @staticmethod
    def backward(ctx, g):
        n_in = len(ctx.needs_input_grad)
        if g is None:
            return (None,) * n_in
        x, canon, packed, pooled, arg = ctx.saved_tensors
        B, _, N = x.shape
        needs_p = ctx.needs_input_grad[2:]
        dev, L_ = x.device, lib()
        with torch.cuda.device(dev):
            g32 = g.contiguous().to(torch.float32)                        # a local: it must outlive the launch's enqueue
            dcanon = torch.empty_like(canon) if any(needs_p) else None
            dx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
            if B > 0 and (dcanon is not None or dx is not None):
                ws = torch.empty(L_.dpf_encoder_frozen_workspace_bytes(B), dtype=torch.uint8, device=dev)
                check(L_.dpf_encoder_frozen_backward(B, N, ctx.prec, canon.data_ptr(), packed.data_ptr(), x.data_ptr(),
                                                     pooled.data_ptr(), arg.data_ptr(), g32.data_ptr(),
                                                     dcanon.data_ptr() if dcanon is not None else None,
                                                     dx.data_ptr() if dx is not None else None, ws.data_ptr(), current_stream()),
                      "encoder_frozen_backward")
            elif dcanon is not None:
                dcanon.zero_()
            pgrads = scatter_param_grads(dcanon, ctx.slots, ctx.shapes, needs_p)
        return (None, dx, *pgrads)


def run_frozen_pool(enc, x):
    """(B,512) max over the points of the eval-mode encoder, attached to autograd through the HIP backward"""
    return _FrozenPool.apply(enc, x, *frozen_params(enc))
