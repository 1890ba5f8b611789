"""eval_autograd on the PointNet encoder without a GPU: the attribute, its validation and its absence from the state dict; "hip"
on CPU tensors is served by tensor operations with the warning; and the float64 restatement of the sparse backward that checks
the HIP path (tests/encoder_frozen_ref.py) is itself checked against float64 autograd of the module -- negative and zero
BatchNorm scales in every layer, dead features -- and pinned by vectors captured from the reference's module
(tools/gen_golden_encoder_frozen.py -> tests/golden/encoder_frozen.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from dpf_nets_amd.networks.encoders import PointNetCloudEncoder
from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
from oracle import detrng
from oracle import encoder_oracle as EO
from tests import encoder_frozen_ref as R

GOLD_TOL = 1e-4          # the fixture is the reference's float32 module
HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def test_attribute_default_validation_and_state_dict():
    enc = PointNetCloudEncoder(3, 64, [128, 256, 512])
    assert enc.eval_autograd == "torch"
    keys = set(enc.state_dict())
    enc.eval_autograd = "hip"
    assert enc.eval_autograd == "hip" and set(enc.state_dict()) == keys and not any("eval_autograd" in k for k in keys)
    with pytest.raises(ValueError):
        enc.eval_autograd = "triton"
    assert enc.eval_autograd == "hip"
    enc.eval_autograd = "torch"
    assert enc.eval_autograd == "torch"


def test_hip_on_cpu_tensors_is_tensor_ops_with_the_warning():
    torch.manual_seed(0)
    enc = PointNetCloudEncoder(3, 64, [128, 256, 512]).eval()
    enc.eval_autograd = "hip"
    x = torch.randn(2, 3, 7, requires_grad=True)
    with pytest.warns(EvalModeAutogradWarning):
        feat = enc(x)
    assert isinstance(feat, torch.Tensor) and feat.requires_grad
    assert torch.equal(feat, enc.forward_torch(x))
    x2 = torch.randn(2, 3, 7)                         # parameters only: still under autograd, still the warning
    with pytest.warns(EvalModeAutogradWarning):
        assert torch.equal(enc(x2), enc.forward_torch(x2))


@pytest.mark.parametrize("B,N", [(2, 5), (3, 33)])
def test_restatement_vs_float64_autograd(B, N):
    seed = 40 + B
    st = R.edge_state(seed)
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N)).double()
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512))).double()
    enc = R.load_state(PointNetCloudEncoder(3, 64, [128, 256, 512]), st)
    for name in R.LAYERS:                              # the state covers what it says it covers
        gam = getattr(enc.features, name + "_bn").weight
        assert (gam < 0).any() and (gam == 0).sum() >= 3
    out = R.sparse_backward(st, x, g)
    pooled, dx, grads = R.autograd_reference(enc, x, g)
    dead = pooled == 0
    assert dead[:, 2::9].all() and not dead.all()
    assert _rel(out["pooled"], pooled) < 1e-12 and _rel(out["dx"], dx) < 1e-12
    assert set(out["grads"]) == set(grads)
    for k, v in grads.items():
        assert out["grads"][k].shape == v.shape and _rel(out["grads"][k], v) < 1e-12, k
    # a dead feature: gradient exactly zero and finite
    for k in ("features.sd2.weight", "features.sd2_bn.weight", "features.sd2_bn.bias"):
        v = out["grads"][k].reshape(512, -1)
        assert torch.isfinite(v).all() and (v[2::9] == 0).all(), k
    # the same with arg handed in
    out2 = R.sparse_backward(st, x, g, arg=out["arg"])
    assert torch.equal(out2["dx"], out["dx"]) and torch.equal(out2["pooled"], out["pooled"])
    # and with another point per feature: the gradients follow the gather
    arg2 = (out["arg"] + 1) % N
    out3 = R.sparse_backward(st, x, g, arg=arg2)
    pooled3, dx3, grads3 = R.autograd_reference(enc, x, g, arg=arg2)
    assert _rel(out3["pooled"], pooled3) < 1e-12 and _rel(out3["dx"], dx3) < 1e-12
    for k, v in grads3.items():
        assert _rel(out3["grads"][k], v) < 1e-12, k


@pytest.mark.parametrize("case", ["a", "b"])
def test_restatement_vs_reference_fixture(case):
    gold = np.load(os.path.join(HERE, "golden", "encoder_frozen.npz"))
    with open(os.path.join(HERE, "golden", "encoder_frozen.json")) as f:
        seed, B, N, edge = json.load(f)["cases"][case]
    st = R.edge_state(seed) if edge else EO.make_encoder_state(seed)
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N)).double()
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512))).double()
    out = R.sparse_backward(st, x, g)
    assert _rel(out["pooled"], torch.from_numpy(gold[case + "_pooled"]).double()) < GOLD_TOL
    assert _rel(out["dx"], torch.from_numpy(gold[case + "_dx"]).double()) < GOLD_TOL
    keys = [k for k in gold.files if k.startswith(case + "_gproj_")]
    assert len(keys) == 12
    for k in keys:
        name = k[len(case + "_gproj_"):]
        want = gold[k]
        got = R.projection(out["grads"][name], name, seed)
        assert np.abs(got - want).max() <= GOLD_TOL * max(want[2], 1e-30), (name, got, want)


def test_gpu_seeds_keep_the_dx_skip_share_under_the_cap():
    """The seeds of tests/test_gpu_encoder_frozen.py, on the float64 reference alone: the argmax points with a pre-activation
    within TOL_OUT of zero are at most DX_SKIP_CAP of the argmax points of every case."""
    for (B, N, edge) in R.SEEDS:
        _, st, x, g = R.case_inputs(B, N, edge)
        out = R.sparse_backward(st, x.double(), g.double())
        skip, pts = R.near_zero_points(out["pre"], out["arg"], out["pooled"] > 0)
        share = len(skip) / len(pts)
        print("B=%d N=%d edge=%d: %d argmax points, share with a near-zero pre-activation %.3f" % (B, N, edge, len(pts), share))
        assert len(pts) > 0 and share <= R.DX_SKIP_CAP, (B, N, edge, share)
