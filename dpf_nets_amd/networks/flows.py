"""CondRealNVPFlow3D / CondRealNVPFlow3DTriple with the reference's constructor
signatures, sub-module and parameter names (lib/networks/flows.py:10-160), so
reference checkpoints load unchanged.

forward(p, g, mode) -> (p_out, mu, logvar), p (B,3,N), g (B,G).  Which backend serves a call -- the fused HIP stack
(csrc/flow.hip), the HIP training kernels (networks/train_engine.py), the frozen-statistics HIP node (networks/frozen_engine.py) or
the tensor-op restatement of flows.py:95-117 (`forward_torch`, the reference-shaped module the CPU tests check against the golden
vectors) -- is networks/backend.py's point_flow.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from . import backend as B
from .backend import Backend, TRAIN_IMPL, TRAIN_FLAT   # noqa: F401  (re-exported; the call sites read B.TRAIN_IMPL, B.TRAIN_FLAT)
from .layers import SharedDot, Swish, PackedWeights, EvalAutograd, EvalModeAutogradWarning, warn_eval_autograd   # noqa: F401  (re-exported)
from .engine import FlowStack
from .frozen_engine import cuda_fp32, run_frozen_stack, frozen_precision_ok
from .train_engine import StackSpec, run_training_stack


def stack_spec(owner, layers):
    """The static layout description of `layers`, cached on `owner` per number of layers."""
    cache = owner.__dict__.setdefault("_train_specs", {})
    spec = cache.get(len(layers))
    if spec is None:
        spec = cache[len(layers)] = StackSpec(layers)
    return spec


def choose(owner, stack, layers, precision, p, g, n_layers_given=False):
    """(backend.point_flow's outcome for a forward(p, g) call of `owner` over `layers()`, whose fused stack is `stack()`; the
    layers' spec where the frozen node can be asked for, built at most once per call).  B.ask reads the node's facts where they decide."""
    training, ea, grad = owner.training, owner.eval_autograd, torch.is_grad_enabled()
    # point_flow's leading arguments in its order: training, eval_autograd, grad, input_rg, p_cuda, train_impl, n_layers_given
    cheap = (training, ea, grad, p.requires_grad or g.requires_grad, p.is_cuda, B.TRAIN_IMPL, n_layers_given)
    if not B.frozen_candidate(training, ea, grad):                 # the hot paths: one question, one positional call
        return B.point_flow(*cheap), None
    memo = []
    spec = lambda: memo[0] if memo else memo.append(stack_spec(owner, layers())) or memo[0]     # noqa: E731
    return B.ask(lambda **node: B.point_flow(*cheap, **node), [
                          ("cuda_fp32", lambda: cuda_fp32(p, g)),
                          ("param_rg", lambda: any(t.requires_grad for t in spec().all_params())),
                          ("precision_ok", lambda: frozen_precision_ok(stack(), spec(), precision, p.device))]), spec


def train_stack(owner, layers, p, g, mode, full_stack=False):
    """Run `layers` (DIRECT order) through the HIP training path.  full_stack: the decoder's whole stack (backend.flattens)."""
    spec = stack_spec(owner, layers)
    if B.flattens(B.TRAIN_FLAT, full_stack) and spec.flat is None:
        spec.flatten(p.device)
    return run_training_stack(spec, p, g, mode)


class CondRealNVPFlow3D(EvalAutograd, PackedWeights, nn.Module):
    def __init__(self, f_n_features, g_n_features, weight_std=0.01, warp_inds=[0],
                 centered_translation=False, eps=1e-6):
        super().__init__()
        self.f_n_features, self.g_n_features = f_n_features, g_n_features
        self.weight_std = weight_std
        self.warp_inds = list(warp_inds)
        self.keep_inds = [c for c in (0, 1, 2) if c not in self.warp_inds]
        self.centered_translation = centered_translation          # stored, never used (flows.py:20)
        self.eps_value = float(eps)
        self.register_buffer("eps", torch.tensor([eps], dtype=torch.float32))
        Fh, G, nk, nw = f_n_features, g_n_features, len(self.keep_inds), len(self.warp_inds)
        for br in ("mu", "logvar"):                                # registration order = state-dict order
            setattr(self, "T_%s_0" % br, nn.Sequential(OrderedDict([
                ("%s_sd0" % br, SharedDot(nk, Fh, 1)),
                ("%s_sd0_bn" % br, nn.BatchNorm1d(Fh)),
                ("%s_sd0_relu" % br, nn.ReLU(inplace=True)),
                ("%s_sd1" % br, SharedDot(Fh, Fh, 1)),
                ("%s_sd1_bn" % br, nn.BatchNorm1d(Fh, affine=False)),
            ])))
            for s in ("w", "b"):
                film = nn.Sequential(OrderedDict([
                    ("%s_sd1_film_%s0" % (br, s), nn.Linear(G, Fh, bias=False)),
                    ("%s_sd1_film_%s0_bn" % (br, s), nn.BatchNorm1d(Fh)),
                    ("%s_sd1_film_%s0_swish" % (br, s), Swish()),
                    ("%s_sd1_film_%s1" % (br, s), nn.Linear(Fh, Fh, bias=True)),
                ]))
                setattr(self, "T_%s_0_cond_%s" % (br, s), film)
            setattr(self, "T_%s_1" % br, nn.Sequential(OrderedDict([
                ("%s_sd1_relu" % br, nn.ReLU(inplace=True)),
                ("%s_sd2" % br, SharedDot(Fh, nw, 1, bias=True)),
            ])))
            with torch.no_grad():                                  # flows.py:52-58 / 87-93
                for last in (getattr(self, "T_%s_0_cond_w" % br)[-1], getattr(self, "T_%s_0_cond_b" % br)[-1],
                             getattr(self, "T_%s_1" % br)[-1]):
                    last.weight.normal_(std=weight_std)
                    last.bias.zero_()
        self.precision = None                                      # None -> engine.DEFAULT_PRECISION

    # -- the two paths -----------------------------------------------------------
    def _conditioner(self, br, x, g):
        h = getattr(self, "T_%s_0" % br)(x)
        a = self.eps + torch.exp(getattr(self, "T_%s_0_cond_w" % br)(g).unsqueeze(2))
        return getattr(self, "T_%s_1" % br)(a * h + getattr(self, "T_%s_0_cond_b" % br)(g).unsqueeze(2))

    def forward_torch(self, p, g, mode="direct"):
        """flows.py:95-117 on tensor ops (training-mode BatchNorm, differentiable)."""
        x = p[:, self.keep_inds, :].contiguous()
        logvar = torch.zeros_like(p)
        mu = torch.zeros_like(p)
        logvar[:, self.warp_inds, :] = nn.functional.softsign(self._conditioner("logvar", x, g))
        mu[:, self.warp_inds, :] = self._conditioner("mu", x, g)
        scale = torch.sqrt(self.eps + torch.exp(logvar))
        if mode == "direct":
            p_out = scale * p + mu
        elif mode == "inverse":
            p_out = (p - mu) / scale
        else:
            raise ValueError(mode)
        return p_out, mu, logvar

    def forward(self, p, g, mode="direct"):
        if mode not in ("direct", "inverse"):
            raise ValueError(mode)
        stack = lambda: self.packed_stack(lambda: FlowStack([self]))           # noqa: E731
        out, spec = choose(self, stack, lambda: [self], self.precision, p, g)
        warn_eval_autograd(out.warning, 2)
        if out.backend is Backend.TRAIN_HIP:
            ps, mus, lvs = train_stack(self, [self], p, g, mode)
        elif out.backend is Backend.FROZEN_HIP:
            ps, mus, lvs = run_frozen_stack(stack(), spec(), p, g, mode, self.precision)
        elif out.backend is Backend.TENSOR_OPS:
            return self.forward_torch(p, g, mode)
        else:
            p_out, _, ps, mus, lvs = stack().run(p, g, mode, self.precision, want_lists=True)
            return p_out, mus[0], lvs[0]
        return ps[0], mus[0], lvs[0]


class CondRealNVPFlow3DTriple(EvalAutograd, PackedWeights, nn.Module):
    WARPS = {0: ([0], [1], [2]), 1: ([0, 1], [0, 2], [1, 2])}     # flows.py:129-148

    def __init__(self, f_n_features, g_n_features, weight_std=0.02, pattern=0, centered_translation=False):
        super().__init__()
        self.f_n_features, self.g_n_features = f_n_features, g_n_features
        self.weight_std, self.pattern, self.centered_translation = weight_std, pattern, centered_translation
        for i, warp in enumerate(self.WARPS[pattern]):
            setattr(self, "nvp%d" % (i + 1), CondRealNVPFlow3D(
                f_n_features, g_n_features, weight_std=weight_std, warp_inds=list(warp),
                centered_translation=centered_translation))

    def layers(self):
        return [self.nvp1, self.nvp2, self.nvp3]

    def _chain(self, p, g, mode, call):                            # flows.py:151-160
        if mode == "direct":
            p1, mu1, lv1 = call(self.nvp1, p, g, mode)
            p2, mu2, lv2 = call(self.nvp2, p1, g, mode)
            p3, mu3, lv3 = call(self.nvp3, p2, g, mode)
        elif mode == "inverse":
            p3, mu3, lv3 = call(self.nvp3, p, g, mode)
            p2, mu2, lv2 = call(self.nvp2, p3, g, mode)
            p1, mu1, lv1 = call(self.nvp1, p2, g, mode)
        else:
            raise ValueError(mode)
        return [p1, p2, p3], [mu1, mu2, mu3], [lv1, lv2, lv3]

    def forward_torch(self, p, g, mode="direct"):
        return self._chain(p, g, mode, lambda lyr, pp, gg, mm: lyr.forward_torch(pp, gg, mm))

    def forward(self, p, g, mode="direct"):
        if mode not in ("direct", "inverse"):
            raise ValueError(mode)
        stack = lambda: self.packed_stack(lambda: FlowStack(self.layers()))    # noqa: E731
        out, spec = choose(self, stack, self.layers, self.nvp1.precision, p, g)
        if out.backend is Backend.TRAIN_HIP:                       # the three layers as one autograd node
            return train_stack(self, self.layers(), p, g, mode)
        if out.backend is Backend.FROZEN_HIP:                      # the three layers as one frozen-statistics node
            return run_frozen_stack(stack(), spec(), p, g, mode, self.nvp1.precision)
        # FUSED, TENSOR_OPS: layer by layer, each layer asking (and warning) for itself
        return self._chain(p, g, mode, lambda lyr, pp, gg, mm: lyr(pp, gg, mode=mm))
