"""networks/backend.py without a GPU: the table row by row, both sides of every condition, the rows on which a costly fact stays
unread -- and the eight call sites on CPU tensors: what a live module does is what the table says for the facts of that call, and
what it returns is forward_torch's, bit for bit."""
import copy
import itertools
import os
import subprocess
import sys
import warnings

import pytest
import torch

from dpf_nets_amd import networks as nets
from dpf_nets_amd.networks import backend as B
from dpf_nets_amd.networks.layers import EVAL_AUTOGRAD_MESSAGES, EvalModeAutogradWarning

BOOLS = (False, True)


def check_rows(chooser, base, rows):
    for name, change, want in rows:
        unknown = set(change) - set(base)
        assert not unknown, (name, unknown)
        got = chooser(**dict(base, **change))
        assert got is want, (name, got, want)


# ---- the table ----------------------------------------------------------------------------------------------------------------
# base: an eval-mode call under no particular request, on tensors every kernel takes, every costly verdict "yes"
POINT = dict(training=False, eval_autograd="torch", grad=True, input_rg=False, param_rg=False, p_cuda=True, cuda_fp32=True,
             train_impl="hip", precision_ok=True, n_layers_given=False)
FROZEN_P = dict(eval_autograd="hip", input_rg=True)              # a served frozen-node call, as a change of the base
TRAIN_P = dict(training=True)
POINT_ROWS = [
    ("eval, nothing requires grad", {}, B.FUSED),
    ("eval, grad mode off", dict(grad=False, input_rg=True, param_rg=True), B.FUSED),
    ("eval, an input requires grad", dict(input_rg=True), B.TENSOR_OPS_LOUD),
    ("eval, only parameters require grad", dict(param_rg=True), B.FUSED),
    ("eval on CPU tensors is the stack's business", dict(p_cuda=False, cuda_fp32=False), B.FUSED),
    ("eval, n_layers", dict(n_layers_given=True), B.FUSED),
    ("eval, an input requires grad, n_layers", dict(input_rg=True, n_layers_given=True), B.N_LAYERS_ERROR_LOUD),
    # the training node and each of its conditions
    ("training", TRAIN_P, B.TRAIN_HIP),
    ("training, n_layers", dict(TRAIN_P, n_layers_given=True), B.TRAIN_HIP),
    ("training, whatever autograd", dict(TRAIN_P, eval_autograd="hip", input_rg=True, param_rg=True, grad=False), B.TRAIN_HIP),
    ("training, p on the CPU", dict(TRAIN_P, p_cuda=False, cuda_fp32=False), B.TENSOR_OPS),
    ("training, g alone on the CPU or another dtype: the engine refuses", dict(TRAIN_P, cuda_fp32=False), B.TRAIN_HIP),
    ("training, DPF_TRAIN_IMPL=torch", dict(TRAIN_P, train_impl="torch"), B.TENSOR_OPS),
    ("training, DPF_TRAIN_IMPL=torch, inputs require grad: silent", dict(TRAIN_P, train_impl="torch", input_rg=True), B.TENSOR_OPS),
    ("training, DPF_TRAIN_IMPL=torch, n_layers", dict(TRAIN_P, train_impl="torch", n_layers_given=True), B.N_LAYERS_ERROR),
    ("training on the CPU with 'hip'", dict(TRAIN_P, p_cuda=False, cuda_fp32=False, eval_autograd="hip", input_rg=True), B.TENSOR_OPS),
    # the frozen node and each of its conditions
    ("frozen: an input requires grad", FROZEN_P, B.FROZEN_HIP),
    ("frozen: only parameters require grad", dict(FROZEN_P, input_rg=False, param_rg=True), B.FROZEN_HIP),
    ("frozen, n_layers", dict(FROZEN_P, n_layers_given=True), B.FROZEN_HIP),
    ("frozen, DPF_TRAIN_IMPL=torch", dict(FROZEN_P, train_impl="torch"), B.FROZEN_HIP),
    ("frozen <- 'torch'", dict(FROZEN_P, eval_autograd="torch"), B.TENSOR_OPS_LOUD),
    ("frozen <- grad mode off", dict(FROZEN_P, grad=False), B.FUSED),
    ("frozen <- nothing requires grad", dict(FROZEN_P, input_rg=False), B.FUSED),
    ("frozen <- not CUDA fp32", dict(FROZEN_P, cuda_fp32=False), B.TENSOR_OPS_LOUD),
    ("frozen <- precision or range refused", dict(FROZEN_P, precision_ok=False), B.TENSOR_OPS_LOUD),
    ("frozen <- refused, n_layers", dict(FROZEN_P, precision_ok=False, n_layers_given=True), B.N_LAYERS_ERROR_LOUD),
    ("as found: parameters only, refused: fused and detached, silent",
     dict(FROZEN_P, input_rg=False, param_rg=True, precision_ok=False), B.FUSED),
    ("as found: the same on CPU tensors", dict(FROZEN_P, input_rg=False, param_rg=True, p_cuda=False, cuda_fp32=False), B.FUSED),
]

SAMPLE = dict(training=False, eval_autograd="torch", grad=True, input_rg=False, param_rg=False, noise_cuda=True, cuda_fp32=True,
              base_fp32=True)
SAMPLE_ROWS = [
    ("eval: the fused prologue", {}, B.FUSED),
    ("eval, grad mode off", dict(grad=False, input_rg=True), B.FUSED),
    ("eval, only parameters require grad", dict(param_rg=True), B.FUSED),
    ("fused <- g on the CPU or not fp32 is the stack's business", dict(cuda_fp32=False), B.FUSED),
    ("fused <- training", dict(training=True), B.TENSOR_OPS),
    ("fused <- noise on the CPU", dict(noise_cuda=False, cuda_fp32=False), B.TENSOR_OPS),
    ("fused <- noise on the CPU, inputs require grad: silent here", dict(noise_cuda=False, cuda_fp32=False, input_rg=True), B.TENSOR_OPS),
    ("fused <- an input requires grad", dict(input_rg=True), B.TENSOR_OPS_LOUD),
    ("fused <- noise / mu0 / logvar0 not all fp32", dict(base_fp32=False, cuda_fp32=False), B.TENSOR_OPS),
    ("training, inputs require grad: silent", dict(training=True, input_rg=True), B.TENSOR_OPS),
    ("frozen: an input requires grad", dict(eval_autograd="hip", input_rg=True), B.FROZEN_HIP),
    ("frozen: only parameters require grad", dict(eval_autograd="hip", param_rg=True), B.FROZEN_HIP),
    ("frozen <- grad mode off", dict(eval_autograd="hip", input_rg=True, grad=False), B.FUSED),
    ("frozen <- training", dict(eval_autograd="hip", input_rg=True, training=True), B.TENSOR_OPS),
    ("frozen <- not all four CUDA fp32", dict(eval_autograd="hip", input_rg=True, cuda_fp32=False), B.TENSOR_OPS_LOUD),
    ("frozen <- not CUDA fp32, parameters only", dict(eval_autograd="hip", param_rg=True, cuda_fp32=False), B.FUSED),
]

PRIOR = dict(training=False, eval_autograd="torch", grad=True, input_rg=False, param_rg=False, cuda=True, fp32=True,
             train_impl="hip", has_steps=True, decoder=True, patterns_ok=True)
FROZEN_G = dict(eval_autograd="hip", input_rg=True)
TRAIN_G = dict(training=True)
PRIOR_ROWS = [
    ("eval, nothing requires grad", {}, B.FUSED),
    ("eval, a lone step or couple", dict(decoder=False), B.FUSED),
    ("eval, grad mode off", dict(grad=False, input_rg=True, param_rg=True), B.FUSED),
    ("eval, only parameters require grad", dict(param_rg=True), B.FUSED),
    ("eval, another dtype is the stack's business", dict(fp32=False), B.FUSED),
    ("fused <- g requires grad", dict(input_rg=True), B.TENSOR_OPS_LOUD),
    ("fused <- other index patterns", dict(patterns_ok=False), B.TENSOR_OPS),
    ("fused <- n_flows == 0", dict(has_steps=False, patterns_ok=False), B.TENSOR_OPS),
    ("as found: n_flows == 0 never warns", dict(has_steps=False, patterns_ok=False, input_rg=True), B.TENSOR_OPS),
    ("fused <- CPU", dict(cuda=False), B.TENSOR_OPS),
    ("as found: CPU, 'torch', g requires grad: silent", dict(cuda=False, input_rg=True), B.TENSOR_OPS),
    ("CPU, 'hip', g requires grad: loud", dict(cuda=False, eval_autograd="hip", input_rg=True), B.TENSOR_OPS_LOUD),
    ("CPU, 'hip', grad mode off", dict(cuda=False, eval_autograd="hip", input_rg=True, grad=False), B.TENSOR_OPS),
    ("CPU, 'hip', parameters only", dict(cuda=False, eval_autograd="hip", param_rg=True), B.TENSOR_OPS),
    # the training node: the decoder's alone
    ("training", TRAIN_G, B.TRAIN_HIP),
    ("training, whatever autograd", dict(TRAIN_G, eval_autograd="hip", input_rg=True, param_rg=True, grad=False), B.TRAIN_HIP),
    ("as found: training, a lone step or couple", dict(TRAIN_G, decoder=False), B.TENSOR_OPS),
    ("training <- n_flows == 0", dict(TRAIN_G, has_steps=False), B.TENSOR_OPS),
    ("training <- CPU", dict(TRAIN_G, cuda=False), B.TENSOR_OPS),
    ("training <- DPF_TRAIN_IMPL=torch", dict(TRAIN_G, train_impl="torch"), B.TENSOR_OPS),
    ("training <- another dtype", dict(TRAIN_G, fp32=False), B.TENSOR_OPS),
    ("training <- other index patterns", dict(TRAIN_G, patterns_ok=False), B.TENSOR_OPS),
    ("training, DPF_TRAIN_IMPL=torch, g requires grad: silent", dict(TRAIN_G, train_impl="torch", input_rg=True), B.TENSOR_OPS),
    # the frozen node
    ("frozen: g requires grad", FROZEN_G, B.FROZEN_HIP),
    ("frozen: only parameters require grad", dict(FROZEN_G, input_rg=False, param_rg=True), B.FROZEN_HIP),
    ("frozen: a lone step or couple", dict(FROZEN_G, decoder=False), B.FROZEN_HIP),
    ("frozen, DPF_TRAIN_IMPL=torch", dict(FROZEN_G, train_impl="torch"), B.FROZEN_HIP),
    ("frozen <- 'torch'", dict(FROZEN_G, eval_autograd="torch"), B.TENSOR_OPS_LOUD),
    ("frozen <- grad mode off", dict(FROZEN_G, grad=False), B.FUSED),
    ("frozen <- nothing requires grad", dict(FROZEN_G, input_rg=False), B.FUSED),
    ("frozen <- training", dict(FROZEN_G, training=True), B.TRAIN_HIP),
    ("frozen <- n_flows == 0", dict(FROZEN_G, has_steps=False), B.TENSOR_OPS),
    ("frozen <- CPU", dict(FROZEN_G, cuda=False), B.TENSOR_OPS_LOUD),
    ("frozen <- another dtype", dict(FROZEN_G, fp32=False), B.TENSOR_OPS_LOUD),
    ("frozen <- other index patterns", dict(FROZEN_G, patterns_ok=False), B.TENSOR_OPS_LOUD),
    ("as found: parameters only, other patterns: tensor ops, silent", dict(FROZEN_G, input_rg=False, param_rg=True, patterns_ok=False),
     B.TENSOR_OPS),
    ("as found: parameters only, another dtype: the fused stack (which refuses it)", dict(FROZEN_G, input_rg=False, param_rg=True, fp32=False),
     B.FUSED),
]

ENC = dict(training=False, eval_autograd="torch", grad=True, input_rg=False, param_rg=False, frozen_serves=False, arch_ok=True,
           train_serves=False, cuda=True, layout_ok=True)
FROZEN_E = dict(eval_autograd="hip", input_rg=True, frozen_serves=True, arch_ok=False)       # arch_ok is not read on this row
TRAIN_E = dict(training=True, train_serves=True)
ENC_ROWS = [
    ("eval", {}, B.FUSED),
    ("eval, grad mode off", dict(grad=False, input_rg=True, param_rg=True), B.FUSED),
    ("eval, only parameters require grad", dict(param_rg=True), B.FUSED),
    ("eval <- CPU", dict(cuda=False), B.CPU_ERROR),
    ("eval <- CPU and a wrong layout: the CPU error first", dict(cuda=False, layout_ok=False), B.CPU_ERROR),
    ("eval <- another dtype or shape", dict(layout_ok=False), B.LAYOUT_ERROR),
    ("eval <- other widths", dict(arch_ok=False), B.TENSOR_OPS),
    ("eval <- other widths, CPU", dict(arch_ok=False, cuda=False), B.TENSOR_OPS),
    ("as found: eval, the input requires grad: silent", dict(input_rg=True), B.TENSOR_OPS),
    ("the same on the CPU", dict(input_rg=True, cuda=False), B.TENSOR_OPS),
    ("training", TRAIN_E, B.TRAIN_HIP),
    ("training, whatever autograd", dict(TRAIN_E, eval_autograd="hip", input_rg=True, param_rg=True), B.TRAIN_HIP),
    ("training <- the kernels refuse (hip_training off, CPU, dtype, shape limits, BatchNorm): silent", dict(TRAIN_E, train_serves=False),
     B.TENSOR_OPS),
    ("training <- other widths", dict(TRAIN_E, arch_ok=False, train_serves=False), B.TENSOR_OPS),
    ("training on the CPU never raises", dict(TRAIN_E, train_serves=False, cuda=False, layout_ok=False), B.TENSOR_OPS),
    ("frozen: the input requires grad", FROZEN_E, B.FROZEN_HIP),
    ("frozen: only parameters require grad", dict(FROZEN_E, input_rg=False, param_rg=True), B.FROZEN_HIP),
    ("frozen <- the kernels refuse: loud", dict(FROZEN_E, frozen_serves=False), B.TENSOR_OPS_UNSERVED),
    ("frozen <- refused, parameters only: loud all the same", dict(FROZEN_E, frozen_serves=False, input_rg=False, param_rg=True),
     B.TENSOR_OPS_UNSERVED),
    ("frozen <- 'torch'", dict(FROZEN_E, eval_autograd="torch", arch_ok=True), B.TENSOR_OPS),
    ("frozen <- grad mode off", dict(FROZEN_E, grad=False, arch_ok=True), B.FUSED),
    ("frozen <- nothing requires grad", dict(FROZEN_E, input_rg=False, arch_ok=True), B.FUSED),
    ("frozen <- training", dict(FROZEN_E, training=True, arch_ok=True, train_serves=True), B.TRAIN_HIP),
]


@pytest.mark.parametrize("chooser,base,rows", [(B.point_flow, POINT, POINT_ROWS), (B.sample_and_decode, SAMPLE, SAMPLE_ROWS),
                                               (B.prior_flow, PRIOR, PRIOR_ROWS), (B.encoder, ENC, ENC_ROWS)],
                         ids=["point_flow", "sample_and_decode", "prior_flow", "encoder"])
def test_every_row(chooser, base, rows):
    check_rows(chooser, base, rows)
    assert len({name for name, _, _ in rows}) == len(rows)


def test_outcomes_are_plain_data():
    assert B.TENSOR_OPS_LOUD == (B.Backend.TENSOR_OPS, "inputs", None) and B.TENSOR_OPS_UNSERVED.warning == "unserved"
    assert B.N_LAYERS_ERROR_LOUD == (B.Backend.ERROR, "inputs", "n_layers") and B.N_LAYERS_ERROR.warning is None
    assert (B.CPU_ERROR.error, B.LAYOUT_ERROR.error) == ("cpu", "layout")
    assert {o.backend for o in (B.FUSED, B.TRAIN_HIP, B.FROZEN_HIP, B.TENSOR_OPS, B.CPU_ERROR)} == set(B.Backend)
    assert set(EVAL_AUTOGRAD_MESSAGES) == {"inputs", "unserved"}
    assert EVAL_AUTOGRAD_MESSAGES["inputs"].startswith("eval()-mode flow called with inputs that require grad: served by PyTorch tensor")
    assert EVAL_AUTOGRAD_MESSAGES["unserved"].startswith("eval_autograd='hip': this call (CPU tensors, a dtype other than float32")


def test_frozen_asked_and_flattens_both_sides():
    served = dict(training=False, eval_autograd="hip", grad=True, input_rg=True, param_rg=True)
    assert B.frozen_asked(**served)
    assert B.frozen_asked(**dict(served, input_rg=False)) and B.frozen_asked(**dict(served, param_rg=False))
    for change in (dict(training=True), dict(eval_autograd="torch"), dict(grad=False), dict(input_rg=False, param_rg=False)):
        assert not B.frozen_asked(**dict(served, **change)), change
    assert B.frozen_candidate(False, "hip", True) and B.frozen_candidate(training=False, eval_autograd="hip", grad=True)
    assert not (B.frozen_candidate(True, "hip", True) or B.frozen_candidate(False, "torch", True) or B.frozen_candidate(False, "hip", False))
    assert [B.flattens(f, d) for f in BOOLS for d in BOOLS] == [False, False, False, True]


def _facts(base, combo, **more):
    training, grad, input_rg, param_rg, ea = combo
    return dict(dict(base, training=training, grad=grad, input_rg=input_rg, param_rg=param_rg, eval_autograd=ea), **more)


def _product(base, fixed=()):
    keys = [k for k in base if k not in fixed]
    values = [("torch", "hip") if k in ("eval_autograd", "train_impl") else BOOLS for k in keys]
    for combo in itertools.product(*values):
        yield dict(base, **dict(zip(keys, combo)))


def _asked_with_reads(chooser, kw, costly):
    """ask() over the facts `kw`, the `costly` ones behind readers -> (outcome, the names read, in order)"""
    read = []
    cheap = {k: v for k, v in kw.items() if k not in costly}
    out = B.ask(lambda **c: chooser(**cheap, **c), [(name, lambda name=name: read.append(name) or kw[name]) for name in costly])
    return out, read


def test_ask_reads_a_costly_fact_only_where_the_modules_always_did():
    """Over every combination of the facts: ask() answers what the chooser answers with every fact known, and calls a reader on no
    row on which the ladders it replaces did not -- stated here from those ladders, not from the table."""
    for kw in _product(POINT):
        out, read = _asked_with_reads(B.point_flow, kw, ("cuda_fp32", "param_rg", "precision_ok"))
        assert out is B.point_flow(**kw), kw
        gate = not kw["training"] and kw["eval_autograd"] == "hip" and kw["grad"]
        assert gate or not read, (kw, read)                        # training steps, no_grad, "torch": nothing is looked at
        assert "param_rg" not in read or not kw["input_rg"], kw    # any(inputs) or any(parameters): the walk is short-circuited
        assert "precision_ok" not in read or (kw["cuda_fp32"] and (kw["input_rg"] or kw["param_rg"])), kw
    for base, chooser, frozen_facts in ((POINT, B.point_flow, ("cuda_fp32", "param_rg", "precision_ok")), (SAMPLE, B.sample_and_decode, ("cuda_fp32", "param_rg")),
                                        (PRIOR, B.prior_flow, ("param_rg",)), (ENC, B.encoder, ("param_rg", "frozen_serves"))):
        for kw in _product(base):                                  # no candidate: the callers ask straight away, False stands for all
            if not B.frozen_candidate(kw["training"], kw["eval_autograd"], kw["grad"]):
                assert chooser(**kw) is chooser(**{k: v for k, v in kw.items() if k not in frozen_facts}), kw
    for kw in _product(SAMPLE):
        out, read = _asked_with_reads(B.sample_and_decode, kw, ("cuda_fp32", "param_rg"))
        assert out is B.sample_and_decode(**kw), kw
        gate = not kw["training"] and kw["eval_autograd"] == "hip" and kw["grad"]
        assert gate or not read, (kw, read)
        assert "param_rg" not in read or not kw["input_rg"], kw
    for kw in _product(PRIOR):
        out, read = _asked_with_reads(B.prior_flow, kw, ("patterns_ok", "param_rg"))
        assert out is B.prior_flow(**kw), kw
        on_device = kw["has_steps"] and kw["cuda"]
        frozen_looked = kw["eval_autograd"] == "hip" and kw["fp32"]                                    # _frozen_prior
        fused_looked = not kw["training"] and not (kw["grad"] and kw["input_rg"])                      # _fusable
        train_looked = kw["training"] and kw["decoder"] and kw["train_impl"] == "hip" and kw["fp32"]   # GlobalRNVPDecoder.forward
        assert "patterns_ok" not in read or (on_device and (frozen_looked or fused_looked or train_looked)), (kw, read)
        assert "param_rg" not in read or (on_device and frozen_looked and kw["patterns_ok"] and not kw["training"] and kw["grad"]
                                          and not kw["input_rg"]), (kw, read)
    for kw in _product(ENC):
        out, read = _asked_with_reads(B.encoder, kw, ("param_rg", "frozen_serves", "arch_ok"))
        assert out is B.encoder(**kw), kw
        gate = not kw["training"] and kw["eval_autograd"] == "hip" and kw["grad"]
        asked = gate and (kw["input_rg"] or kw["param_rg"])
        assert "param_rg" not in read or (gate and not kw["input_rg"]), (kw, read)
        assert "frozen_serves" not in read or asked, (kw, read)
        assert "arch_ok" not in read or not asked, (kw, read)      # the widths are looked at once the node has declined


def test_environment_is_read_in_one_file_by_a_fresh_process():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from dpf_nets_amd.networks import backend, flows; "
            "print(backend.TRAIN_IMPL, backend.TRAIN_FLAT, flows.TRAIN_IMPL, flows.TRAIN_FLAT)")
    env = dict(os.environ, DPF_TRAIN_IMPL="torch", DPF_TRAIN_FLAT="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=here, env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["torch", "True", "torch", "True"]
    assert B.TRAIN_IMPL == nets.flows.TRAIN_IMPL == os.environ.get("DPF_TRAIN_IMPL", "hip")
    net_dir = os.path.join(here, "dpf_nets_amd", "networks")
    readers = [f for f in sorted(os.listdir(net_dir)) if f.endswith(".py")
               and any(k in open(os.path.join(net_dir, f)).read() for k in ('"DPF_TRAIN_IMPL"', '"DPF_TRAIN_FLAT"'))]
    assert readers == ["backend.py"]


# ---- the eight call sites on CPU tensors -------------------------------------------------------------------------------------
G_POINT, G_PRIOR, NF_PRIOR, BATCH, NPTS = 8, 8, 16, 2, 5
COMBOS = list(itertools.product(BOOLS, BOOLS, BOOLS, BOOLS, ("torch", "hip")))      # training, grad, input_rg, param_rg, eval_autograd
MODULE_PY = os.path.join("torch", "nn", "modules", "module.py")


def _flat(x):
    if torch.is_tensor(x):
        return [x]
    out = []
    for v in x:
        out += _flat(v)
    return out


def _observe(call):
    """-> (result or the exception, [(message, file the warning is attributed to)])"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            res = call()
        except (RuntimeError, ValueError) as e:
            res = e
    return res, [(str(w.message), w.filename) for w in caught if issubclass(w.category, EvalModeAutogradWarning)]


def _check(site, combo, outcome, res, warned, ref, n_warn, frame):
    tag = (site, combo, outcome)
    want = [EVAL_AUTOGRAD_MESSAGES[outcome.warning]] * n_warn if outcome.warning else []
    assert [m for m, _ in warned] == want, tag
    assert all(f.endswith(frame) for _, f in warned), (tag, warned)
    if outcome.backend is B.Backend.TENSOR_OPS:
        assert not isinstance(res, Exception), (tag, res)
        got, exp = _flat(res), _flat(ref())
        assert len(got) == len(exp) and all(torch.equal(a, b) and a.requires_grad == b.requires_grad for a, b in zip(got, exp)), tag
    elif outcome.backend is B.Backend.FUSED:                       # no CPU path: the stack itself refuses
        assert isinstance(res, RuntimeError) and "MI355X only" in str(res), (tag, res)
    elif outcome.error == "n_layers":
        assert isinstance(res, ValueError) and "n_layers" in str(res), (tag, res)
    elif outcome.error == "cpu":
        assert isinstance(res, RuntimeError) and "no CPU fallback" in str(res), (tag, res)
    else:
        raise AssertionError("not reachable on CPU tensors: %r" % (tag,))


def _prepared(proto, training, param_rg, eval_autograd):
    m = copy.deepcopy(proto).train(training).requires_grad_(param_rg)
    m.eval_autograd = eval_autograd
    return m


@pytest.fixture(scope="module")
def protos():
    torch.manual_seed(11)
    dec = nets.LocalCondRNVPDecoder(1, 64, G_POINT, weight_std=0.1)
    pri = nets.GlobalRNVPDecoder(1, NF_PRIOR, G_PRIOR, weight_std=0.1)
    enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512])
    for m in (dec, pri, enc):                                      # eval mode must differ from training mode
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(std=0.1)
                mod.running_var.uniform_(0.5, 1.5)
    return dict(flow=dec.flows[0].nvp2, triple=dec.flows[0], decoder=dec, step=pri.flows[0].nvp1, couple=pri.flows[0], prior=pri, encoder=enc)


@pytest.mark.parametrize("site,n_layers", [("flow", None), ("triple", None), ("decoder", None), ("decoder", 2)])
def test_point_flow_modules_on_cpu(protos, site, n_layers):
    torch.manual_seed(3)
    p0, g0 = torch.randn(BATCH, 3, NPTS) * 0.3, torch.randn(BATCH, G_POINT)
    kw = {} if n_layers is None else dict(n_layers=n_layers)
    for combo in COMBOS:
        training, grad, input_rg, param_rg, ea = combo
        m, ref = _prepared(protos[site], training, param_rg, ea), _prepared(protos[site], training, param_rg, ea)
        p, g = p0.clone().requires_grad_(input_rg), g0.clone()
        with torch.set_grad_enabled(grad):
            outcome = B.point_flow(**_facts(POINT, combo, p_cuda=False, cuda_fp32=False, train_impl=B.TRAIN_IMPL, precision_ok=False, n_layers_given=n_layers is not None))
            res, warned = _observe(lambda: m(p, g, mode="inverse", **kw))
            # the triple runs the row layer by layer: a warning per layer, every one attributed as a lone layer's
            _check(site, combo, outcome, res, warned, lambda: ref.forward_torch(p, g, mode="inverse"), 3 if site == "triple" else 1, MODULE_PY)
        if site == "decoder" and n_layers is None and outcome.backend is B.Backend.TENSOR_OPS:
            assert [s.shape for s in res[0]] == [p.shape] * 3


def test_sample_and_decode_on_cpu(protos):
    torch.manual_seed(4)
    mu0, lv0, g0 = torch.randn(BATCH, 3, 1).expand(BATCH, 3, NPTS) * 0.1, torch.randn(BATCH, 3, 1).expand(BATCH, 3, NPTS) * 0.1, torch.randn(BATCH, G_POINT)
    noise0 = torch.randn(BATCH, 3, NPTS)
    for combo in COMBOS:
        training, grad, input_rg, param_rg, ea = combo
        m, ref = _prepared(protos["decoder"], training, param_rg, ea), _prepared(protos["decoder"], training, param_rg, ea)
        noise, g = noise0.clone(), g0.clone().requires_grad_(input_rg)
        with torch.set_grad_enabled(grad):
            first = B.sample_and_decode(**_facts(SAMPLE, combo, noise_cuda=False, cuda_fp32=False))
            assert first is B.TENSOR_OPS                           # CPU noise: z by the in-place tensor ops, silently, then forward()
            outcome = B.point_flow(**_facts(POINT, combo, p_cuda=False, cuda_fp32=False, train_impl=B.TRAIN_IMPL, precision_ok=False))

            def reference():
                z = noise0.clone().mul(torch.exp(0.5 * lv0)).add_(mu0)
                return (z,) + tuple(ref.forward_torch(z, g, mode="direct"))
            res, warned = _observe(lambda: m.sample_and_decode(mu0, lv0, g, noise=noise))
            # forward() is called from sample_and_decode's own frame
            _check("sample_and_decode", combo, outcome, res, warned, reference, 1, os.path.join("networks", "decoders.py"))


@pytest.mark.parametrize("site", ["step", "couple", "prior"])
def test_prior_flow_modules_on_cpu(protos, site):
    torch.manual_seed(5)
    g0 = torch.randn(BATCH, G_PRIOR)
    for combo in COMBOS:
        training, grad, input_rg, param_rg, ea = combo
        m, ref = _prepared(protos[site], training, param_rg, ea), _prepared(protos[site], training, param_rg, ea)
        g = g0.clone().requires_grad_(input_rg)
        with torch.set_grad_enabled(grad):
            outcome = B.prior_flow(**_facts(PRIOR, combo, cuda=False, train_impl=B.TRAIN_IMPL, decoder=site == "prior"))
            assert outcome is B.prior_flow(**_facts(PRIOR, combo, cuda=False, train_impl=B.TRAIN_IMPL, decoder=site == "prior", param_rg=False, patterns_ok=False))
            res, warned = _observe(lambda: m(g, mode="direct"))
            _check(site, combo, outcome, res, warned, lambda: ref.forward_torch(g, "direct"), 1, os.path.join("networks", "prior_flows.py"))
        assert "_patterns_ok" not in m.__dict__ and "_train_plan" not in m.__dict__      # neither read on CPU tensors
    # _fusable's CPU case as found: loud with "hip", silent with "torch"
    assert B.prior_flow(**dict(PRIOR, eval_autograd="hip", input_rg=True, cuda=False, decoder=False, patterns_ok=False)) is B.TENSOR_OPS_LOUD
    assert B.prior_flow(**dict(PRIOR, input_rg=True, cuda=False, decoder=False, patterns_ok=False)) is B.TENSOR_OPS


def test_prior_flow_edge_modules_on_cpu():
    empty = nets.GlobalRNVPDecoder(0, NF_PRIOR, G_PRIOR).eval()
    empty.eval_autograd = "hip"
    g = torch.randn(BATCH, G_PRIOR, requires_grad=True)
    assert B.prior_flow(**dict(PRIOR, eval_autograd="hip", input_rg=True, cuda=False, has_steps=False, patterns_ok=False)) is B.TENSOR_OPS
    res, warned = _observe(lambda: empty(g))
    assert [list(x) for x in res] == [[], [], []] and not warned
    odd = nets.RealNVPFlowCouple(NF_PRIOR, G_PRIOR, pattern=2)       # as the reference: no sub-modules, and forward fails on them
    for call in (lambda: odd(g), lambda: odd.forward_torch(g)):
        with pytest.raises(AttributeError, match="nvp1"):
            call()
    with pytest.raises(ValueError):
        odd(g, mode="sideways")                                      # mode is validated first


@pytest.mark.parametrize("widths", [[128, 256, 512], [32, 64, 128]])
def test_encoder_on_cpu(protos, widths):
    torch.manual_seed(6)
    proto = protos["encoder"] if widths[0] == 128 else nets.PointNetCloudEncoder(3, 64, widths)
    x0 = torch.randn(BATCH, 3, NPTS)
    for combo in COMBOS:
        training, grad, input_rg, param_rg, ea = combo
        m, ref = _prepared(proto, training, param_rg, ea), _prepared(proto, training, param_rg, ea)
        x = x0.clone().requires_grad_(input_rg)
        with torch.set_grad_enabled(grad):
            outcome = B.encoder(**_facts(ENC, combo, arch_ok=m.hip_supported(), cuda=False))
            assert m.hip_supported() == (widths[0] == 128)
            res, warned = _observe(lambda: m(x))
            _check("encoder", combo, outcome, res, warned, lambda: ref.forward_torch(x), 1, MODULE_PY)


def test_mode_is_validated_first(protos):
    p, g = torch.randn(BATCH, 3, NPTS), torch.randn(BATCH, G_POINT)
    for site in ("flow", "triple", "decoder"):
        with pytest.raises(ValueError, match="sideways"):
            protos[site](p, g, mode="sideways")
    for site in ("step", "couple", "prior"):
        with pytest.raises(ValueError, match="sideways"):
            protos[site](torch.randn(BATCH, G_PRIOR), mode="sideways")
