"""eval_autograd on the latent prior flow without a GPU: the attribute reaches the couples and the steps, an invalid value is
refused, "hip" on CPU tensors is served by tensor operations with the warning; and the float64 oracle that checks the HIP path
(tests/gprior_frozen_ref.py) is itself pinned for eval-mode gradients by vectors captured from the reference's module
(tools/gen_golden_gprior_frozen.py -> tests/golden/gprior_frozen.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from dpf_nets_amd import networks as nets
from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
from tests.gprior_frozen_ref import NAMES, oracle64, rel

TOL = 1e-4


def test_eval_autograd_defaults_propagates_and_validates():
    dec = nets.GlobalRNVPDecoder(3, 8, 4).eval()
    assert dec.eval_autograd == "torch"
    assert all(c.eval_autograd == "torch" for c in dec.flows) and all(s.eval_autograd == "torch" for s in dec.coupling_layers())
    dec.eval_autograd = "hip"
    assert all(c.eval_autograd == "hip" for c in dec.flows) and all(s.eval_autograd == "hip" for s in dec.coupling_layers())
    dec.flows[1].eval_autograd = "torch"
    assert [s.eval_autograd for s in dec.flows[1].layers()] == ["torch"] * 2 and dec.flows[0].nvp2.eval_autograd == "hip"
    assert dec.eval_autograd == "hip"
    assert not any("eval_autograd" in k for k in dec.state_dict())


def test_invalid_value_raises():
    dec = nets.GlobalRNVPDecoder(1, 8, 4)
    for module in (dec, dec.flows[0], dec.flows[0].nvp1):
        with pytest.raises(ValueError):
            module.eval_autograd = "triton"
        assert module.eval_autograd == "torch"


def test_hip_on_cpu_tensors_is_tensor_ops_with_the_warning():
    torch.manual_seed(0)
    dec = nets.GlobalRNVPDecoder(2, 8, 6, weight_std=0.1).eval()
    dec.eval_autograd = "hip"
    g0 = torch.randn(3, 6)
    res = []
    for use_forward in (True, False):
        dec.zero_grad()
        g = g0.clone().requires_grad_(True)
        if use_forward:
            with pytest.warns(EvalModeAutogradWarning):
                gs, mus, lvs = dec(g, mode="inverse")
        else:
            gs, mus, lvs = dec.forward_torch(g, "inverse")
        assert isinstance(gs, list) and gs[0].grad_fn is not None
        (gs[0].square().mean() + sum(lvs).mean() + 1e-3 * (0.5 * mus[1]).sum()).backward()
        res.append((g.grad.clone(), [p.grad.clone() for p in dec.parameters()]))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    for module, call in ((dec.flows[0], lambda g: dec.flows[0](g, mode="direct")[0][-1]),
                         (dec.flows[0].nvp1, lambda g: dec.flows[0].nvp1(g, mode="direct")[0])):
        with pytest.warns(EvalModeAutogradWarning):
            assert call(g0.clone().requires_grad_(True)).grad_fn is not None


def test_float64_oracle_vs_reference_golden_gradients(golden_dir):
    """The checker of the GPU tests against the reference's own eval-mode module under autograd: lists, d/dg and the projection of
    every parameter gradient (written as tests/test_gpu_gprior.py::test_training_mode_vs_reference_golden writes it)."""
    from oracle.gen_golden import _grad_projection
    gold = np.load(os.path.join(golden_dir, "gprior_frozen.npz"))
    meta = json.load(open(os.path.join(golden_dir, "gprior_frozen.json")))
    assert sorted(tuple(v) for v in meta["cases"].values()) == [(7, 2, 16, 8, 5), (8, 1, 8, 2, 1)]
    for case, (seed, n_flows, nf, G, B) in meta["cases"].items():
        for mode in ("direct", "inverse"):
            tag = "%s_%s_" % (case, mode)
            ref = oracle64(seed, n_flows, nf, G, B, mode)
            for name in NAMES:
                assert rel(ref[name], gold[tag + name]) <= TOL, (case, mode, name)
            assert rel(ref["dg"], gold[tag + "dg"]) <= TOL, (case, mode)
            proj = _grad_projection([(k, torch.from_numpy(v)) for k, v in ref["grads"].items()], seed)
            assert len(proj) == 10 * 2 * n_flows
            for k, v in proj.items():
                r = gold[tag + "gproj_" + k]
                np.testing.assert_allclose(v, r, rtol=1e-3, atol=1e-4 * max(1.0, float(r[2])), err_msg=case + mode + k)
