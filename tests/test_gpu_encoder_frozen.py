"""The eval-mode PointNet encoder under autograd on HIP (`eval_autograd = "hip"`: csrc/encoder.hip with the argmax switched on,
csrc/encoder_frozen.hip for the backward, networks/encoder_frozen_engine.py) against

  * the plain launch: pooled has its bits, arg is the lowest point attaining the row maximum of its feature output;
  * the float64 module in eval() under autograd, pooled formed by gather at the kernel's own arg (a near-tie of two points is
    not a failure), at a lone point, ragged tiles, both sides of the 256-point workgroup and several workgroups per cloud, with
    negative / zero BatchNorm scales and dead features at (3, 33) and (5, 700);
  * the fixture captured from the reference's module (tools/gen_golden_encoder_frozen.py).

Bars (tests/test_gpu_encoder_train.py's): TOL_OUT = 1e-4 for pooled, TOL_GRAD = 5e-4 for every parameter gradient at both
precisions and for dx at bf16x6, relative to the tensor's largest magnitude.  dx at bf16x3 is compared per argmax point at
TOL_GRAD: the forward's 1e-5-class error can put a ReLU on the other side of zero than float64, which moves one point's dx by a
finite amount; a point is left out only if one of its 448 float64 pre-activations lies within TOL_OUT of zero relative to its
layer's largest magnitude, and at most 10 % of the argmax points of a case may be left out (the seeds are picked for that on the
float64 reference alone: tests/test_encoder_frozen_cpu.py)."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import detrng
from oracle import encoder_oracle as EO
from tests import encoder_frozen_ref as R

pytestmark = pytest.mark.gpu

PRECISIONS = ("bf16x3", "bf16x6")
GOLD_TOL = 1e-4          # tests/test_encoder_frozen_cpu.py's
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(B, N, 0) for B, N in R.GPU_SHAPES] + [(B, N, 1) for B, N in R.EDGE_SHAPES]
_cache = {}


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def _encoder(nets, st, prec, mode="hip"):
    enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512])
    R.load_state(enc, st, torch.float32)
    enc = enc.cuda().eval()
    enc.precision, enc.eval_autograd = prec, mode
    return enc


def _kernel_arg(enc, x):
    """pooled and arg straight from dpf_encoder_forward_arg"""
    from dpf_nets_amd._lib import lib, check, current_stream, PREC
    L_ = lib()
    B, _, N = x.shape
    pooled = torch.empty((B, 512), dtype=torch.float32, device=x.device)
    arg = torch.full((B, 512), -7, dtype=torch.int32, device=x.device)
    scratch = torch.empty(L_.dpf_encoder_arg_scratch_bytes(B), dtype=torch.uint8, device=x.device)
    check(L_.dpf_encoder_forward_arg(B, N, PREC[enc.precision], enc._packed(x.device).data_ptr(), x.data_ptr(), pooled.data_ptr(),
                                     arg.data_ptr(), scratch.data_ptr(), current_stream()), "encoder_forward_arg")
    torch.cuda.synchronize()
    return pooled, arg


def _backward(enc, x, g, x_grad=True, p_grad=True):
    for p in enc.parameters():
        p.requires_grad_(p_grad)
        p.grad = None
    xin = x.detach().clone().requires_grad_(x_grad)
    feats = enc(xin)
    pooled = torch.max(feats, dim=2)[0]
    (pooled * g).sum().backward()
    return feats, pooled, xin


def _run(B, N, edge, prec):
    """one HIP forward + backward of a case and its float64 reference at the kernel's arg, computed once and shared"""
    key = (B, N, edge, prec)
    if key not in _cache:
        nets = _gpu()
        seed, st, x, g = R.case_inputs(B, N, edge)
        enc = _encoder(nets, st, prec)
        x, g = x.cuda(), g.cuda()
        with warnings.catch_warnings():
            warnings.simplefilter("error", nets.flows.EvalModeAutogradWarning)
            feats, pooled, xin = _backward(enc, x, g)
        kp, arg = _kernel_arg(enc, x)
        with torch.no_grad():
            plain = enc(x)
            plain_pooled = torch.max(plain, dim=2)[0].clone()
            feat = plain.tensor().clone()
        enc64 = R.load_state(nets.PointNetCloudEncoder(3, 64, [128, 256, 512]), st)
        ref_pooled, ref_dx, ref_grads = R.autograd_reference(enc64, x.cpu(), g.cpu(), arg=arg.cpu())
        sparse = R.sparse_backward(st, x.cpu().double(), g.cpu().double(), arg=arg.cpu())
        _cache[key] = dict(enc=enc, feats=feats, pooled=pooled.detach(), kernel_pooled=kp, arg=arg, plain_pooled=plain_pooled, feat=feat,
                           dx=xin.grad, grads={k: p.grad for k, p in enc.named_parameters()}, ref_pooled=ref_pooled, ref_dx=ref_dx,
                           ref_grads=ref_grads, pre=sparse["pre"], x=x, g=g, st=st, seed=seed)
    return _cache[key]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,N,edge", CASES)
def test_forward_keeps_the_bits_and_yields_the_lowest_argmax(B, N, edge, prec):
    r = _run(B, N, edge, prec)
    assert isinstance(r["feats"], _gpu().encoders.FrozenPointFeatures)
    assert r["pooled"].dtype == torch.float32 and r["pooled"].shape == (B, 512)
    assert torch.equal(r["pooled"], r["plain_pooled"]) and torch.equal(r["kernel_pooled"], r["plain_pooled"])
    arg, feat = r["arg"].long(), r["feat"]
    assert arg.dtype == torch.int64 and int(arg.min()) >= 0 and int(arg.max()) < N
    at = torch.gather(feat, 2, arg[:, :, None])[..., 0]
    assert torch.equal(at.view(torch.int32), r["pooled"].view(torch.int32))
    lowest = (feat == feat.max(dim=2, keepdim=True)[0]).to(torch.int64).argmax(dim=2)
    live = r["pooled"] > 0
    assert bool(live.any()) and torch.equal(arg[live], lowest[live])


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("N", [33, 700])
def test_identical_points_give_arg_zero(N, prec):
    nets = _gpu()
    enc = _encoder(nets, EO.make_encoder_state(5), prec)
    x = torch.tensor([0.3, -0.2, 0.1], device="cuda").view(1, 3, 1).expand(2, 3, N).contiguous()
    pooled, arg = _kernel_arg(enc, x)
    live = pooled > 0
    assert bool(live.any()) and int(arg[live].abs().max()) == 0 and int(arg.min()) >= 0 and int(arg.max()) < N


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,N,edge", CASES)
def test_gradients_vs_float64_at_the_kernels_arg(B, N, edge, prec):
    r = _run(B, N, edge, prec)
    e = rel(r["pooled"], r["ref_pooled"])
    print("B=%d N=%d edge=%d %s: pooled %.2e" % (B, N, edge, prec, e))
    worst = {}
    for k, ref in r["ref_grads"].items():
        assert r["grads"][k] is not None and torch.isfinite(r["grads"][k]).all(), k
        worst[k] = rel(r["grads"][k], ref)
    print("   parameter gradients: worst %.2e (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    dx, ref_dx = r["dx"].double().cpu(), r["ref_dx"]
    assert torch.isfinite(dx).all()
    e_dx = rel(dx, ref_dx)
    print("   dx max-norm %.2e" % e_dx)
    assert e < R.TOL_OUT, (e, R.TOL_OUT)
    for k, v in worst.items():
        assert v < R.TOL_GRAD, (k, v)
    if edge:                                          # dead features: exactly zero, finite
        dead = (r["pooled"][:, 2::9] == 0).all().item()
        assert dead
        for k in ("features.sd2.weight", "features.sd2_bn.weight", "features.sd2_bn.bias"):
            assert (r["grads"][k].reshape(512, -1)[2::9] == 0).all(), k
    live = (r["pooled"] > 0).cpu()
    skip, pts = R.near_zero_points(r["pre"], r["arg"].cpu().long(), live)
    # away from the argmax points dx is zero, bit for bit
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b, n in pts:
        mask[b, n] = True
    assert (dx.permute(0, 2, 1)[~mask] == 0).all()
    if prec == "bf16x6":
        assert e_dx < R.TOL_GRAD, e_dx
        return
    share = len(skip) / len(pts)
    print("   bf16x3 dx: %d argmax points, %d left out (share %.3f)" % (len(pts), len(skip), share))
    assert share <= R.DX_SKIP_CAP, share
    compared = [p for p in pts if p not in skip]
    assert compared, "an empty comparison"
    bar = R.TOL_GRAD * float(ref_dx.abs().max())
    bad = [(p, float((dx[p[0], :, p[1]] - ref_dx[p[0], :, p[1]]).abs().max())) for p in compared]
    bad = [(p, d) for p, d in bad if not d < bar]
    assert not bad, (bad[:5], bar)



@pytest.mark.parametrize("prec", PRECISIONS)
def test_two_runs_and_a_second_backward_give_identical_bits(prec):
    nets = _gpu()
    B, N, edge = 5, 700, 1
    r = _run(B, N, edge, prec)
    enc, x, g = _encoder(nets, r["st"], prec), r["x"], r["g"]          # an encoder of its own: the shared runs stay as they are
    feats, pooled, xin = _backward(enc, x, g)
    _, arg2 = _kernel_arg(enc, x)
    assert torch.equal(pooled, r["pooled"]) and torch.equal(arg2, r["arg"]) and torch.equal(xin.grad, r["dx"])
    for k, p in enc.named_parameters():
        assert torch.equal(p.grad, r["grads"][k]), k
    # retain_graph and a second backward
    for p in enc.parameters():
        p.grad = None
    xin = x.detach().clone().requires_grad_(True)
    pooled = torch.max(enc(xin), dim=2)[0]
    loss = (pooled * g).sum()
    loss.backward(retain_graph=True)
    first = [xin.grad.clone()] + [p.grad.clone() for p in enc.parameters()]
    xin.grad = None
    for p in enc.parameters():
        p.grad = None
    loss.backward()
    for a, b in zip(first, [xin.grad] + [p.grad for p in enc.parameters()]):
        assert torch.equal(a, b)
    assert torch.equal(first[0], r["dx"])


def test_which_gradients_are_formed_and_the_buffers_stay():
    nets = _gpu()
    B, N = 3, 33
    seed, st, x, g = R.case_inputs(B, N, 1)
    x, g = x.cuda(), g.cuda()
    enc = _encoder(nets, st, "bf16x3")
    buffers = {k: v.clone() for k, v in enc.named_buffers()}
    full = _run(B, N, 1, "bf16x3")
    # parameters only: twelve gradients, nothing for x
    feats, pooled, xin = _backward(enc, x, g, x_grad=False)
    assert pooled.grad_fn is not None and xin.grad is None
    assert len(list(enc.parameters())) == 12
    for k, p in enc.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, full["grads"][k]), k
    # x only
    feats, pooled, xin = _backward(enc, x, g, p_grad=False)
    assert torch.equal(xin.grad, full["dx"]) and all(p.grad is None for p in enc.parameters())
    for p in enc.parameters():
        p.requires_grad_(True)
    for k, v in enc.named_buffers():
        assert torch.equal(v, buffers[k]), k
    assert all(int(getattr(enc.features, n + "_bn").num_batches_tracked) == 0 for n in R.LAYERS)
    # a step of an optimizer that writes through .data reaches the next call
    with torch.no_grad():
        enc.features.sd2_bn.bias.data.add_(0.25)
    p2 = torch.max(enc(x.clone().requires_grad_(True)), dim=2)[0]
    fresh = _encoder(nets, {k: v.cpu().numpy() for k, v in enc.state_dict().items()}, "bf16x3", mode="torch")
    with torch.no_grad():
        want = torch.max(fresh(x), dim=2)[0]
    assert torch.equal(p2.detach(), want) and not torch.equal(want, full["plain_pooled"])


def test_warnings_other_uses_and_the_default_mode():
    nets = _gpu()
    W = nets.flows.EvalModeAutogradWarning
    B, N = 2, 31
    seed, st, x, g = R.case_inputs(B, N, 0)
    x, g = x.cuda(), g.cuda()
    enc = _encoder(nets, st, "bf16x3")
    xin = x.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", W)
        feats = enc(xin)
        amax = torch.amax(feats, dim=2)
        assert amax.grad_fn is not None and torch.equal(amax, torch.max(feats, 2).values) and torch.equal(amax, feats.amax(dim=2))
        # another use of the features: a differentiable tensor
        y = enc(xin) * 1.0
    assert torch.is_tensor(y) and y.shape == (B, 512, N) and y.requires_grad
    y.sum().backward()
    assert xin.grad is not None and enc.features.init_sd.weight.grad is not None
    # under no_grad, or with nothing requiring grad, "hip" is the plain fused launch
    with torch.no_grad():
        assert type(enc(x)) is nets.encoders.PointFeatures
    # precision "bf16": tensor ops, with the warning
    enc.precision = "bf16"
    with pytest.warns(W):
        out = enc(xin)
    assert torch.is_tensor(out) and out.requires_grad
    # the default mode behaves as before: a differentiable input -> tensor ops (a plain tensor); parameters only -> the fused launch,
    # whose result carries no graph
    enc.precision, enc.eval_autograd = "bf16x3", "torch"
    out = enc(xin)
    assert torch.is_tensor(out) and out.requires_grad
    f = enc(x)
    assert type(f) is nets.encoders.PointFeatures and torch.max(f, dim=2)[0].grad_fn is None


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", ["a", "b"])
def test_reference_fixture_through_the_hip_path(case, prec):
    """pooled, dx and the projections of the twelve gradients at both precisions: the fixture's shapes and seeds keep the reference's
    argmax and ReLU decisions ten times the bf16x3 forward's error clear of a tie / of zero
    (tools/gen_golden_encoder_frozen.py)"""
    nets = _gpu()
    gold = np.load(os.path.join(HERE, "golden", "encoder_frozen.npz"))
    with open(os.path.join(HERE, "golden", "encoder_frozen.json")) as f:
        seed, B, N, edge = json.load(f)["cases"][case]
    st = R.edge_state(seed) if edge else EO.make_encoder_state(seed)
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N)).cuda()
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512))).cuda()
    enc = _encoder(nets, st, prec)
    feats, pooled, xin = _backward(enc, x, g)
    assert rel(pooled, torch.from_numpy(gold[case + "_pooled"])) < GOLD_TOL
    assert rel(xin.grad, torch.from_numpy(gold[case + "_dx"])) < GOLD_TOL
    for k, p in enc.named_parameters():
        want = gold[case + "_gproj_" + k]
        got = R.projection(p.grad, k, seed)
        assert np.abs(got - want).max() <= GOLD_TOL * max(want[2], 1e-30), (k, got, want)
