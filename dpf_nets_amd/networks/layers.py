"""SharedDot / Swish with the reference's parameter names, shapes and init
(lib/networks/layers.py:5-45).  These modules carry the weights (state-dict
compatibility) and serve the training-mode path; in eval mode the coupling
layers read the weights out of them and run the fused HIP stack instead.

Also what every flow module shares around that switch: the packed-weight cache's invalidation (PackedWeights,
weight_state), the EvalModeAutogradWarning and its emission (networks/backend.py decides when), and what the three
frozen-statistics HIP paths share: EvalAutograd, scatter_param_grads."""
import warnings

import torch
import torch.nn as nn


class EvalModeAutogradWarning(RuntimeWarning):
    """An eval()-mode module was called under autograd: the call is served by PyTorch tensor operations, not by the HIP kernels."""


# The two messages of an EvalModeAutogradWarning (backend.Outcome.warning is the key).  "inputs": the fused stacks have a backward
# for training-mode BatchNorm only, so an eval-mode call that must stay differentiable with respect to its INPUTS runs the reference's
# op sequence on ATen (~30 kernels per layer) -- correct, and some 50x slower: a SECOND backend behind forward(), hence loud (VERDICT
# r05 #7).  The reference's own loops never take it (evaluating.py:58-59 runs under no_grad; training.py:37-56 in train() mode).
EVAL_AUTOGRAD_MESSAGES = {
    "inputs": "eval()-mode flow called with inputs that require grad: served by PyTorch tensor operations (differentiable, "
              "~30 ATen kernels per coupling layer), not by the fused HIP stack; call under torch.no_grad() for the HIP "
              "path, or in train() mode for the HIP training kernels",
    "unserved": "eval_autograd='hip': this call (CPU tensors, a dtype other than float32, another architecture or "
                "precision 'bf16') is served by PyTorch tensor operations, not by the HIP kernels",
}


def warn_eval_autograd(which, stacklevel):
    """Emit the warning an outcome names, if any.  stacklevel counts from the caller (1 = the caller's own frame)."""
    if which is not None:
        warnings.warn(EVAL_AUTOGRAD_MESSAGES[which], EvalModeAutogradWarning, stacklevel=stacklevel + 1)


EVAL_AUTOGRAD = ("torch", "hip")


class EvalAutograd:
    """Mixin: the `eval_autograd` attribute (extension, beside `precision`; not in the state dict).  "torch" (default): an
    eval()-mode call whose inputs require grad is served by tensor operations, with an EvalModeAutogradWarning (networks/backend.py).
    "hip": an eval()-mode call on CUDA fp32 tensors where an input or ANY parameter requires grad is one autograd node over the HIP
    kernels with frozen BatchNorm statistics (networks/*frozen_engine.py), no warning.  Setting it on a decoder or a triple reaches the layers."""
    _eval_autograd = "torch"

    @property
    def eval_autograd(self):
        return self._eval_autograd

    @eval_autograd.setter
    def eval_autograd(self, value):
        if value not in EVAL_AUTOGRAD:
            raise ValueError("eval_autograd must be one of %s, got %r" % (list(EVAL_AUTOGRAD), value))
        self.__dict__["_eval_autograd"] = value
        for child in self.children():
            for m in (child if isinstance(child, nn.ModuleList) else [child]):
                if isinstance(m, EvalAutograd):
                    m.eval_autograd = value


def scatter_param_grads(block, slots, like, needs=None):
    """Per entry of `like` (the parameters, or their shapes) a fresh tensor -- never a view: autograd takes it over without a copy
    -- filled from the (offset, numel) `slots` of the gradient `block` by ONE multi-tensor copy; None where `needs` is false.
    slots = None: `block` is the list of flat views itself (the point flow's gradients lie in several blocks)."""
    pick = range(len(like)) if needs is None else [i for i, need in enumerate(needs) if need]
    fresh = [torch.empty_like(like[i]) if torch.is_tensor(like[i]) else block.new_empty(like[i]) for i in pick]
    if fresh:
        src = [block[i] for i in pick] if slots is None else [block[slots[i][0]:slots[i][0] + slots[i][1]] for i in pick]
        torch._foreach_copy_(fresh, [v.view_as(f) for v, f in zip(src, fresh)])
    it = iter(fresh)
    return fresh if needs is None else [next(it) if need else None for need in needs]


def weight_state(tensors):
    """Fingerprint of the weights a packed copy was built from: in-place edits bump `_version`, a re-assigned `.data` moves."""
    return tuple((t._version, t.data_ptr()) for t in tensors)


class PackedWeights:
    """Mixin of the flow modules: `_stack` holds the module's fused eval-mode stack (engine.FlowStack / prior_flows.GPriorStack)
    in the instance __dict__, outside nn.Module's registries.  Its packed weights are rebuilt after anything that may have
    changed the parameters behind the version counters' back -- optimizers update through `.data` -- i.e. on every
    train()/eval() switch, load_state_dict, .to()/.cuda()/.float(); in between, the stack's sentinels (weight_state) catch
    ordinary in-place edits."""
    _stack = None

    def packed_stack(self, build):
        """The module's stack, built by `build()` on first use."""
        if self._stack is None:
            self.__dict__["_stack"] = build()
        return self._stack

    def invalidate_packed(self):
        if self._stack is not None:
            self._stack.invalidate()

    def train(self, mode=True):
        if mode != self.training:
            self.invalidate_packed()
        return super().train(mode)

    def _apply(self, fn, *a, **kw):
        self.invalidate_packed()
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        self.invalidate_packed()
        return super()._load_from_state_dict(*a, **kw)


class Swish(nn.Module):
    def forward(self, x):                       # layers.py:9-10
        return x * torch.sigmoid(x)


class SharedDot(nn.Module):
    """The same (out x in) linear map applied to every point: weight is
    (n_channels, out, in), input (B, in, N) -> (B, out, N)."""

    def __init__(self, in_features, out_features, n_channels, bias=False, init_weight=None, init_bias=None):
        super().__init__()
        self.in_features, self.out_features, self.n_channels = in_features, out_features, n_channels
        self.init_weight, self.init_bias = init_weight, init_bias
        self.weight = nn.Parameter(torch.empty(n_channels, out_features, in_features))
        if bias:
            self.bias = nn.Parameter(torch.empty(n_channels, out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):                 # layers.py:29-38
        if self.init_weight:
            nn.init.uniform_(self.weight.data, a=-self.init_weight, b=self.init_weight)
        else:
            # on the 3-D weight fan_in = out*in (n_channels is dim 0): bound sqrt(6/(out*in))
            nn.init.kaiming_uniform_(self.weight.data, a=0.0)
        if self.bias is not None:
            nn.init.constant_(self.bias.data, self.init_bias if self.init_bias else 0.0)

    def forward(self, x):                       # layers.py:40-45
        out = torch.matmul(self.weight, x.unsqueeze(1))
        if self.bias is not None:
            out = out + self.bias.unsqueeze(0).unsqueeze(3)
        return out.squeeze(1)
