"""LocalCondRNVPDecoder with the reference's constructor and forward() contract
(lib/networks/decoders.py:41-72): forward(p, g, mode) -> (ps, mus, logvars), three
list-likes of 3*n_flows (B,3,N) tensors in DIRECT order for both modes.

The whole stack is ONE fused launch (FlowLists over three (L,B,3,N) buffers the kernel fills), one training node or one
frozen-statistics node; `forward_torch` chains the layers' tensor-op path (decoders.py:58-70).  Who serves a call:
networks/backend.py (point_flow, sample_and_decode)."""
import torch
import torch.nn as nn

from . import backend as B
from .backend import Backend
from .flows import CondRealNVPFlow3DTriple, EvalAutograd, choose, train_stack, stack_spec, cuda_fp32, run_frozen_stack
from .flowlist import FlowList
from .layers import PackedWeights, warn_eval_autograd
from .engine import FlowStack


class LocalCondRNVPDecoder(EvalAutograd, PackedWeights, nn.Module):
    def __init__(self, n_flows, f_n_features, g_n_features, weight_std=0.01):
        super().__init__()
        self.n_flows, self.f_n_features, self.g_n_features = n_flows, f_n_features, g_n_features
        self.weight_std = weight_std
        self.flows = nn.ModuleList([
            CondRealNVPFlow3DTriple(f_n_features, g_n_features, weight_std=weight_std, pattern=i % 2)
            for i in range(n_flows)])
        self.precision = None          # None -> engine.DEFAULT_PRECISION ("f16x3")
        self.materialize_lists = True  # False: skip the 3 x L per-layer tensors (lists then hold the final layer only)
        # eval_autograd (layers.EvalAutograd): "torch" (default) | "hip" = eval()-mode calls under autograd on the HIP kernels

    def coupling_layers(self):
        """All 3*n_flows CondRealNVPFlow3D modules in DIRECT order."""
        return [lyr for tri in self.flows for lyr in tri.layers()]

    def _layers(self, n_layers):
        layers = self.coupling_layers()
        return layers if n_layers is None else layers[:int(n_layers)]

    def _all_params(self):
        return stack_spec(self, self.coupling_layers()).all_params()

    def stack(self):
        return self.packed_stack(lambda: FlowStack(self.coupling_layers()))

    def flatten_parameters(self):
        """Opt-in (extension; DPF_TRAIN_FLAT=1 does it on the first training step): move every parameter and
        BatchNorm buffer of the coupling layers into ONE flat buffer laid out as the HIP training path consumes it,
        with `.grad` as views of a twin gradient buffer (train_engine.FlatStore).  Names, shapes, state dicts and
        optimizers are unaffected; the training step loses the per-parameter gather, scatter and AccumulateGrad
        work (2016 tensors at n_flows=21).  Call it after the module is on its GPU.  Returns the store
        (`.flat_p`, `.flat_g`, `.zero_grad()`); data-parallel runs reduce `.flat_g` with
        dpf_nets_amd.distributed.allreduce_flat_gradients instead of DistributedDataParallel hooks."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("flatten_parameters: move the decoder to its GPU first")
        return stack_spec(self, self.coupling_layers()).flatten(dev)

    def flat_store(self):
        """The FlatStore of the full stack, or None."""
        spec = self.__dict__.get("_train_specs", {}).get(len(self.coupling_layers()))
        return None if spec is None else spec.flat

    def forward_torch(self, p, g, mode="direct"):
        ps, mus, lvs = [], [], []
        for i in range(self.n_flows):                               # decoders.py:58-70
            if mode == "direct":
                buf = self.flows[i].forward_torch(p if i == 0 else ps[-1], g, mode=mode)
                ps, mus, lvs = ps + buf[0], mus + buf[1], lvs + buf[2]
            else:
                buf = self.flows[-(i + 1)].forward_torch(p if i == 0 else ps[0], g, mode=mode)
                ps, mus, lvs = buf[0] + ps, buf[1] + mus, buf[2] + lvs
        return ps, mus, lvs

    def sample_and_decode(self, mu0, logvar0, g, noise=None):
        """`reparameterize` + `forward(z, g, mode='direct')` of lib/networks/models.py:211-213 (and :118-119, :250-253) as
        ONE call (extension): returns (z, ps, mus, logvars) with z = noise * exp(0.5 * logvar0) + mu0 =
        what the models store as p_prior_samples[0].  mu0 / logvar0 are the models' (B,3,S) stride-0 expansions, read in
        place; `noise` defaults to torch.randn_like(logvar0) -- drawn by torch, so the generator stream is the caller's.
        In eval mode on CUDA the sample is formed in the fused kernel's prologue (no exp / mul / add launches, no
        materialised z round trip); otherwise this is exactly the two reference calls."""
        if noise is None:
            noise = torch.randn_like(logvar0)                                      # models.py:78
        training, ea, grad = self.training, self.eval_autograd, torch.is_grad_enabled()
        # sample_and_decode's leading arguments in its order: training, eval_autograd, grad, input_rg, noise_cuda, base_fp32
        cheap = (training, ea, grad, any([t.requires_grad for t in (noise, mu0, logvar0, g)]), noise.is_cuda,
                 noise.dtype == torch.float32 and mu0.dtype == torch.float32 and logvar0.dtype == torch.float32)
        out = B.sample_and_decode(*cheap) if not B.frozen_candidate(training, ea, grad) else B.ask(lambda **node: B.sample_and_decode(*cheap, **node), [
            ("cuda_fp32", lambda: cuda_fp32(noise, mu0, logvar0, g)),
            ("param_rg", lambda: any(t.requires_grad for t in self._all_params()))])
        warn_eval_autograd(out.warning, 2)
        if out.backend is Backend.FROZEN_HIP:
            # the gradient must reach mu0 / logvar0 / noise: z by tensor ops in front of the node
            z = noise * torch.exp(0.5 * logvar0) + mu0
            return (z,) + tuple(self.forward(z, g, mode="direct"))
        if out.backend is Backend.TENSOR_OPS:
            z = noise.mul(torch.exp(0.5 * logvar0)).add_(mu0)                      # models.py:77-79
            return (z,) + tuple(self.forward(z, g, mode="direct"))
        stack = self.stack()
        p_out, sum_lv, ps, mus, lvs = stack.run(noise, g, "direct", self.precision, want_lists=self.materialize_lists,
                                                base=(mu0, logvar0))
        z = stack.last_base_sample
        if ps is None:
            return z, FlowList(p_out.unsqueeze(0)), None, FlowList(sum_lv.unsqueeze(0), sum_lv)
        return z, FlowList(ps), FlowList(mus), FlowList(lvs, sum_lv)

    def forward(self, p, g, mode="direct", n_layers=None):
        """n_layers (extension, default all): run only the first n_layers DIRECT-order layers
        (the BASELINE metric's 14-layer stack = first 14 layers of n_flows=5)."""
        if mode not in ("direct", "inverse"):
            raise ValueError(mode)
        out, spec = choose(self, self.stack, lambda: self._layers(n_layers), self.precision, p, g, n_layers is not None)
        warn_eval_autograd(out.warning, 2)
        if out.backend is Backend.TRAIN_HIP:
            return train_stack(self, self._layers(n_layers), p, g, mode, full_stack=n_layers is None)
        if out.backend is Backend.FROZEN_HIP:
            return run_frozen_stack(self.stack(), spec(), p, g, mode, self.precision)
        if out.backend is Backend.ERROR:
            raise ValueError("n_layers is only supported on the fused eval path")
        if out.backend is Backend.TENSOR_OPS:
            return self.forward_torch(p, g, mode)
        p_out, sum_lv, ps, mus, lvs = self.stack().run(p, g, mode, self.precision,
                                                       want_lists=self.materialize_lists, n_layers=n_layers)
        if ps is None:
            return FlowList(p_out.unsqueeze(0)), None, FlowList(sum_lv.unsqueeze(0), sum_lv)
        return FlowList(ps), FlowList(mus), FlowList(lvs, sum_lv)
