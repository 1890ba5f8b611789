"""Which backend serves a forward() call of a network module, decided in ONE place: pure functions of plain values (no tensors, no
modules, no GPU, no libdpf_hip.so) -- the Python counterpart of csrc/dispatch.h.  tests/test_backend_cpu.py asserts every row; the
modules' forward() gather the facts, ask here and `switch` over the outcome (INTEGRATION.md has the table).

This file records what the modules DO, asymmetries included: a row marked `# as found` looks wrong and is kept for a later change to
argue about.  A costly fact (param_rg, precision_ok, patterns_ok, frozen_serves, train_serves) reaches a chooser
through ask(), which has the caller look only where the answer matters."""
import enum
import os
from collections import namedtuple

# ---- the two switches that pick a backend, read from the environment here and nowhere else -------------------------------
TRAIN_IMPL = os.environ.get("DPF_TRAIN_IMPL", "hip")          # "hip" | "torch": who serves a training-mode flow call on CUDA tensors
TRAIN_FLAT = os.environ.get("DPF_TRAIN_FLAT", "0") == "1"     # the first training step moves the point decoder into a flat store


class Backend(enum.Enum):
    FUSED = "the fused eval-mode launch"              # FlowStack.run, GPriorStack.run, PointFeatures
    TRAIN_HIP = "the training-mode HIP node"          # run_training_stack, run_training_prior, TrainPointFeatures
    FROZEN_HIP = "the frozen-statistics HIP node"     # run_frozen_stack, run_frozen_prior, FrozenPointFeatures
    TENSOR_OPS = "forward_torch"
    ERROR = "refused"


# warning: None | "inputs" | "unserved", the key of layers.EVAL_AUTOGRAD_MESSAGES an EvalModeAutogradWarning is emitted with (before
# an error, where both are set); error: None | "n_layers" (ValueError) | "cpu" | "layout" (the encoder's two RuntimeErrors)
Outcome = namedtuple("Outcome", "backend warning error", defaults=(None, None))
FUSED, TRAIN_HIP, FROZEN_HIP = Outcome(Backend.FUSED), Outcome(Backend.TRAIN_HIP), Outcome(Backend.FROZEN_HIP)
TENSOR_OPS, TENSOR_OPS_LOUD = Outcome(Backend.TENSOR_OPS), Outcome(Backend.TENSOR_OPS, "inputs")
TENSOR_OPS_UNSERVED = Outcome(Backend.TENSOR_OPS, "unserved")
N_LAYERS_ERROR, N_LAYERS_ERROR_LOUD = Outcome(Backend.ERROR, None, "n_layers"), Outcome(Backend.ERROR, "inputs", "n_layers")
CPU_ERROR, LAYOUT_ERROR = Outcome(Backend.ERROR, None, "cpu"), Outcome(Backend.ERROR, None, "layout")


# ---- shared by the three families -----------------------------------------------------------------------------------------
def frozen_candidate(training, eval_autograd, grad):
    """Only then can a call ask for the frozen-statistics node.  The hot paths (training steps, eval under no_grad, "torch") settle
    that with this one question; their callers then ask the chooser straight away, which takes the node's facts as False."""
    return not training and eval_autograd == "hip" and grad


def frozen_asked(training, eval_autograd, grad, input_rg, param_rg):
    """An eval()-mode call asks for the frozen-statistics node: eval_autograd == "hip", grad mode on, an input OR a parameter
    requires grad.  Whether the kernels serve it is each family's question."""
    return frozen_candidate(training, eval_autograd, grad) and (input_rg or param_rg)


def ask(chooser, costly):
    """The outcome of `chooser` -- a family's function with the call's cheap facts already in it -- for the `costly` ones, (name,
    read) pairs in the order the modules have always read them: read() is called only where that fact, with the later ones
    granted, still changes the outcome; False stands for it elsewhere.  Right only for a chooser in which a later fact being False
    never makes an earlier one matter (each family's is: a refusal only ever falls through to rows that ask less); the product test
    in tests/test_backend_cpu.py holds every table edit to that."""
    names = [name for name, _ in costly]
    out = chooser(**dict.fromkeys(names, True))
    if out is chooser(**dict.fromkeys(names, False)):
        return out
    known = {}
    for i, (name, read) in enumerate(costly):          # out: the outcome with this fact and the later ones granted
        without = chooser(**known, **dict.fromkeys(names[i + 1:], True), **{name: False})
        known[name] = out is not without and read()
        if not known[name]:
            out = without
    return out


# ---- the point flow stack: CondRealNVPFlow3D, CondRealNVPFlow3DTriple, LocalCondRNVPDecoder.forward -----------------------
# p_cuda: p is a CUDA tensor; cuda_fp32: p AND g are CUDA fp32; precision_ok: the stack is f16x3 with weights in its exact range
# (frozen_engine.frozen_precision_ok: invalidates the stack, waits for the device)
def point_flow(training, eval_autograd, grad, input_rg, p_cuda, train_impl, n_layers_given=False, cuda_fp32=False, param_rg=False, precision_ok=False):
    if training and p_cuda and train_impl == "hip":
        return TRAIN_HIP                               # (a wrong dtype or a CPU g is the engine's RuntimeError)
    if cuda_fp32 and precision_ok and frozen_asked(training, eval_autograd, grad, input_rg, param_rg):
        return FROZEN_HIP
    # from here on tensor ops or the fused launch; n_layers exists on the fused launch and the two nodes only
    # as found: n_layers raises on these two rows only -- the nodes above take it
    if training:                                       # CPU tensors, DPF_TRAIN_IMPL=torch: silent
        return N_LAYERS_ERROR if n_layers_given else TENSOR_OPS
    if grad and input_rg:                              # autograd follows the INPUTS: loud, also where "hip" was refused
        return N_LAYERS_ERROR_LOUD if n_layers_given else TENSOR_OPS_LOUD
    # as found: "hip" with only PARAMETERS requiring grad and a node that refuses (CPU, another dtype, precision) lands here: the
    # fused launch, silently detached (the encoder warns in that situation).  CPU tensors here are the stack's RuntimeError.
    return FUSED
# The triple runs its FUSED and TENSOR_OPS rows layer by layer, each layer asking again for itself (one launch, or one warning, per
# layer); the decoder hands n_layers to the two nodes and the fused launch.


def flattens(train_flat, decoder_full_stack):
    """DPF_TRAIN_FLAT=1 moves the parameters into a flat store on the first TRAIN_HIP call -- of the decoder's full stack only (not
    with n_layers, not a lone layer or triple)."""
    return train_flat and decoder_full_stack


# ---- LocalCondRNVPDecoder.sample_and_decode: who forms z = noise * exp(0.5 * logvar0) + mu0 -------------------------------
# input_rg: over noise, mu0, logvar0, g; cuda_fp32: all four; base_fp32: noise, mu0, logvar0 are fp32
def sample_and_decode(training, eval_autograd, grad, input_rg, noise_cuda, base_fp32, cuda_fp32=False, param_rg=False):
    if cuda_fp32 and frozen_asked(training, eval_autograd, grad, input_rg, param_rg):
        return FROZEN_HIP                              # z by out-of-place tensor ops in front of forward(), which asks point_flow
    if not training and noise_cuda:
        if grad and input_rg:
            return TENSOR_OPS_LOUD                     # (and forward() warns once more, from its own frame)
        if base_fp32:
            return FUSED                               # z in the fused launch's prologue
    return TENSOR_OPS                                  # z by the in-place tensor ops, then forward() by point_flow


# ---- the prior flow stack: RealNVPFlow, RealNVPFlowCouple, GlobalRNVPDecoder ----------------------------------------------
# has_steps: n_flows > 0 (always for a step or a couple); decoder: the module is a GlobalRNVPDecoder; patterns_ok: every step has
# one of the kernels' four index patterns on an even G
def prior_flow(training, eval_autograd, grad, input_rg, cuda, fp32, train_impl, has_steps, decoder, patterns_ok=False, param_rg=False):
    kernels_ok = has_steps and cuda and fp32 and patterns_ok     # what the frozen and the training node take
    if kernels_ok and frozen_asked(training, eval_autograd, grad, input_rg, param_rg):
        return FROZEN_HIP
    if training:
        # as found: only the decoder has a training node; a lone step or couple in train() mode is tensor ops.  Silent, like CPU
        # tensors, DPF_TRAIN_IMPL=torch, another dtype or pattern.
        return TRAIN_HIP if decoder and kernels_ok and train_impl == "hip" else TENSOR_OPS
    if not has_steps:
        return TENSOR_OPS                              # as found: n_flows == 0 returns its empty lists without ever warning
    if not cuda:
        # as found: a CPU g warns only when "hip" was asked for; with "torch" the same call is silent (the point flow would
        # refuse it in FlowStack.run or warn)
        return TENSOR_OPS_LOUD if eval_autograd == "hip" and grad and input_rg else TENSOR_OPS
    if grad and input_rg:
        return TENSOR_OPS_LOUD                         # as the point flow: autograd follows the INPUT
    # parameters-only grad with a refused node: as the point flow, the fused launch, silently detached (as found).  Another dtype
    # here is GPriorStack.run's RuntimeError; other patterns are tensor ops, silent.
    return FUSED if patterns_ok else TENSOR_OPS


# ---- PointNetCloudEncoder ---------------------------------------------------------------------------------------------------
# frozen_serves: encoder_frozen_engine.frozen_hip_serves; arch_ok: hip_supported(), the 3 -> 64 -> [128, 256, 512] widths with
# eps 1e-5; train_serves: hip_training_supported(input): the hip_training attribute, CUDA fp32 (B,3,N) within the launch limits,
# ordinary BatchNorm; layout_ok: input is fp32 (B,3,N)
def encoder(training, eval_autograd, grad, input_rg, cuda, layout_ok, arch_ok=False, train_serves=False, param_rg=False, frozen_serves=False):
    if frozen_asked(training, eval_autograd, grad, input_rg, param_rg):
        # refused (CPU tensors, another dtype, architecture or precision): loud with the message of its own, parameters-only included
        return FROZEN_HIP if frozen_serves else TENSOR_OPS_UNSERVED
    if not arch_ok:
        return TENSOR_OPS                              # other widths: silent in both modes
    if training:
        # silent; as found: DPF_TRAIN_IMPL is not consulted here, the module's hip_training attribute is (inside train_serves)
        return TRAIN_HIP if train_serves else TENSOR_OPS
    if grad and input_rg:
        return TENSOR_OPS                              # as found: silent, where the flows warn ("torch", a differentiable input)
    if not cuda:
        return CPU_ERROR                               # eval mode has no CPU path
    return FUSED if layout_ok else LAYOUT_ERROR
