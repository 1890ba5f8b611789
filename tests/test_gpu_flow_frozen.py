"""eval_autograd = "hip": the eval-mode (frozen BatchNorm) coupling stack under autograd on the HIP kernels (csrc/flow_frozen.hip,
networks/frozen_engine.py) against the reference's goldens and against the tensor-op path in float64.

Tolerances are the project's: outputs at the fused path's bar (REL["f16x3"] of test_gpu_flow.py), gradients at the training
path's f16x3 bar (GRAD_REL["f16x3"] = 2e-4 of test_gpu_flow_train.py), parameter gradients that are cancelling sums at
max(2e-4, R32_FACTOR["f16x3"] x the fp32 tensor-op path's own error against float64 on the same inputs) with bias_floor;
grad_p through close_but_kinks (a ReLU flip is local to one point: at most max(3, 2e-4 size) elements outside, median <= tol / 10)."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import flow_oracle as FO
from oracle import golden_io
from oracle.gen_golden import layer_inputs, _grad_projection
from tests import flow_hostile as H
from tests.gradcheck import check_projections
from tests.test_gpu_flow import REL
from tests.test_gpu_flow_train import GRAD_REL, R32_FACTOR, rel, bias_floor, close_but_kinks

pytestmark = pytest.mark.gpu
OUT = REL["f16x3"]
GRAD = GRAD_REL["f16x3"]
# The ONE output of test 3 that the fused forward does not bring within OUT of float64, and the multiple of the fp32 tensor-op
# path's own error against float64 it is held to instead (the multiple of the cancelling parameter gradients): see the test.
OUT_EXCEPTION = ((2, 128, 1, 40, "inverse"), "lvs", 2)
OUT_R32_FACTOR = R32_FACTOR["f16x3"]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def _no_warning(caught):
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    assert not any(issubclass(w.category, EvalModeAutogradWarning) for w in caught)


def _layer(nets, case, F, G):
    mod = nets.CondRealNVPFlow3D(F, G, warp_inds=case["warp"])
    mod.load_state_dict(FO.to_torch(FO.make_layer_state(case["seed"], F, G, case["warp"])), strict=True)
    mod = mod.cuda().eval()
    mod.eval_autograd = "hip"
    return mod


def test_single_layer_vs_reference_golden_and_parameters_only(golden_dir):
    """1: the 12 bn == "eval" cases of tests/golden/flow_layer: outputs, grad_p, grad_g and the gproj projections of every
    parameter gradient, no EvalModeAutogradWarning.  2: the same call with only the PARAMETERS requiring grad has a grad_fn, gives
    every parameter the same (finite) gradient and leaves the BatchNorm buffers bit-identical."""
    nets = _gpu()
    gold = golden_io.load(golden_dir, "flow_layer")
    meta = json.load(open(os.path.join(golden_dir, "flow_layer.json")))
    B, N, F, G = meta["B"], meta["N"], meta["F"], meta["G"]
    seen = 0
    for case in meta["cases"]:
        if case["bn"] != "eval":
            continue
        t = case["tag"]
        mod = _layer(nets, case, F, G)
        p, g, r1, r2, r3 = layer_inputs(case["seed"], B, N, G)
        w1, w2, w3 = (torch.from_numpy(r).cuda() for r in (r1, r2, r3))
        tp = torch.from_numpy(p.copy()).cuda().requires_grad_(True)
        tg = torch.from_numpy(g.copy()).cuda().requires_grad_(True)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            po, mu, lv = mod(tp, tg, mode=case["mode"])
        _no_warning(caught)
        ((po * w1).sum() + (lv * w2).sum() + (mu * w3).sum()).backward()
        for name, got in (("p_out", po), ("mu", mu), ("logvar", lv)):
            assert rel(got, gold[t + "/" + name]) <= OUT, (t, name, rel(got, gold[t + "/" + name]))
        close_but_kinks(tp.grad, gold[t + "/grad_p"], GRAD, t + " grad_p")
        assert rel(tg.grad, gold[t + "/grad_g"]) <= GRAD, (t, rel(tg.grad, gold[t + "/grad_g"]))
        named = [(k, v.grad.cpu()) for k, v in mod.named_parameters()]
        check_projections(dict(named), _grad_projection(named, case["seed"]), lambda k: gold[t + "/gproj/" + k], GRAD, t)
        # ---- parameters only
        first = {k: v.grad.clone() for k, v in mod.named_parameters()}
        mod.zero_grad(set_to_none=True)
        bufs = {k: v.clone() for k, v in mod.named_buffers()}
        po, mu, lv = mod(tp.detach(), tg.detach(), mode=case["mode"])
        assert po.grad_fn is not None and mu.grad_fn is not None and lv.grad_fn is not None
        ((po * w1).sum() + (lv * w2).sum() + (mu * w3).sum()).backward()
        for k, v in mod.named_parameters():
            assert v.grad is not None and torch.isfinite(v.grad).all(), (t, k)
            assert torch.equal(v.grad, first[k]), (t, k)
        for k, v in mod.named_buffers():
            assert torch.equal(v, bufs[k]), (t, k)
        seen += 1
    assert seen == 12


def _loss(nets, ps, mus, lvs, tp, mode):
    B, _, N = tp.shape
    pm, pl = torch.zeros(B, 3, N).cuda().to(tp.dtype), torch.full((B, 3, N), -3.6).cuda().to(tp.dtype)
    smp = ps + [tp] if mode == "inverse" else [tp] + ps
    return nets.PointFlowNLL()(smp, [pm] + mus, [pl] + lvs) + 0.1 * (ps[2] * mus[4]).mean()


_RUNS = {}


def _run(nets, n_flows, G, B, N, mode, impl, flat=False, seed=5, mutate=None, variant=None):
    """One forward + backward of the decoder: impl "hip" (eval_autograd), "torch" (fp32 tensor ops), "torch64".  Cached.
    mutate(state, seed) (tests/flow_hostile.py) is applied to the seeded state, variant names one of its input clouds."""
    key = (n_flows, G, B, N, mode, impl, flat, seed, getattr(mutate, "__name__", None), variant)
    if key in _RUNS:
        return _RUNS[key]
    state = FO.make_decoder_state(seed, n_flows, 64, G)
    sd = FO.to_torch(state if mutate is None else mutate(state, seed))
    tgt, z, g = FO.synthetic_inputs(seed, B, N, G) if variant is None else H.hostile_inputs(seed, B, N, G, variant)
    dec = nets.LocalCondRNVPDecoder(n_flows, 64, G, weight_std=0.01)
    dec.load_state_dict(sd, strict=True)
    dec = dec.cuda().eval()
    tp = torch.from_numpy((tgt if mode == "inverse" else z).copy()).cuda()
    tg = torch.from_numpy(g.copy()).cuda()
    if impl == "torch64":
        dec, tp, tg = dec.double(), tp.double(), tg.double()
    tp.requires_grad_(True)
    tg.requires_grad_(True)
    store = dec.flatten_parameters() if flat else None
    if impl == "hip":
        dec.eval_autograd = "hip"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ps, mus, lvs = dec(tp, tg, mode=mode)
        _no_warning(caught)
    else:
        ps, mus, lvs = dec.forward_torch(tp, tg, mode=mode)
    _loss(nets, list(ps), list(mus), list(lvs), tp, mode).backward()
    res = dict(ps=[x.detach() for x in ps], mus=[x.detach() for x in mus], lvs=[x.detach() for x in lvs], gp=tp.grad, gg=tg.grad,
               grads={k: (None if v.grad is None else v.grad.clone()) for k, v in dec.named_parameters()}, store=store,
               precision=dec.stack().last_precision if impl == "hip" else None,
               grad_storage={k: v.grad.untyped_storage().data_ptr() for k, v in dec.named_parameters() if v.grad is not None})
    _RUNS[key] = res
    return res


def _compare(h, t, t32, what):
    for key in ("ps", "mus", "lvs"):
        for i, (a, b, c) in enumerate(zip(h[key], t[key], t32[key])):
            if float(b.abs().max()) == 0.0:
                assert float(a.abs().max()) == 0.0, (what, key, i)
                continue
            r, r32 = rel(a, b), rel(c, b)
            print("OUTREL", what, key, i, r, r32)
            bar = max(OUT, OUT_R32_FACTOR * r32) if (what, key, i) == OUT_EXCEPTION else OUT
            assert r <= bar, (what, key, i, r, r32)
    close_but_kinks(h["gp"], t["gp"], GRAD, "grad_p")
    assert rel(h["gg"], t["gg"]) <= GRAD, (what, rel(h["gg"], t["gg"]))
    for k in t["grads"]:
        if t["grads"][k] is None:
            assert h["grads"][k] is None or float(h["grads"][k].abs().max()) == 0.0, k
            continue
        fl = bias_floor(t["grads"], k)
        r, r32 = rel(h["grads"][k], t["grads"][k], fl), rel(t32["grads"][k], t["grads"][k], fl)
        print("GRADREL", what, k, r, r32)
        assert r <= max(GRAD, R32_FACTOR["f16x3"] * r32), (what, k, r, r32)


@pytest.mark.parametrize("n_flows,G,B,N,mode", [(2, 128, 1, 40, "inverse"), (2, 128, 3, 1000, "direct"), (2, 128, 33, 64, "direct"),
                                                (21, 128, 2, 64, "inverse"), (2, 512, 3, 100, "direct")])
def test_stack_vs_float64_tensor_ops(n_flows, G, B, N, mode):
    """3: one cloud, less than one tile, ragged tiles, more than 32 clouds, all 63 layers, G = 512; NLL + a cross term on inner
    ps[2] * mus[4], so that all three gradient tables and the layer sum are exercised, NULL entries included.

    Every output is held to REL["f16x3"] = 4e-6 of float64 but one: logvars[2] at (n_flows 2, B 1, N 40, inverse), a cancelling
    sum of O(1e-2) terms whose maximum is 4.4e-3.  Measured against float64 on the same inputs: the fused eval stack (the
    existing forward, unchanged here) 8.7e-6, the fp32 tensor-op path 5.7e-6.  Its bar is 5 x the fp32 tensor-op path's error."""
    nets = _gpu()
    h, t, t32 = (_run(nets, n_flows, G, B, N, mode, impl) for impl in ("hip", "torch64", "torch"))
    _compare(h, t, t32, (n_flows, G, B, N, mode))


@pytest.mark.parametrize("variant", H.VARIANTS)
@pytest.mark.parametrize("n_flows,G,B,N,mode", [(2, 128, 1, 40, "inverse"), (2, 128, 3, 100, "direct"), (2, 128, 33, 64, "direct"),
                                                (2, 512, 3, 100, "direct")])
def test_stack_vs_float64_tensor_ops_hostile(n_flows, G, B, N, mode, variant):
    """Test 3 on the states and clouds of tests/flow_hostile.py (gamma0 negative, zero and at the f16x3 guard, running variances
    over four decades, FiLM factors from 7e-7 to several hundred, dead / constant units, a saturated and an identity layer), through
    _compare with its bars unchanged; f16x3 is what was served.  On top, against float64 autograd: the zero-gamma0 feature's
    d gamma0 = sum dh0 xhat is live and its d W0 row exactly 0; the dead unit's dW1 column, d beta0 and d gamma0 are exactly 0; the
    identity layer's d sd2.weight and d sd2.bias are live and at GRAD.

    Measured over the twelve cases, against float64: outputs at most 1.3e-6 (OUT = 4e-6); the worst parameter gradient 6.6e-5 (GRAD =
    2e-4; a FiLM w-net's second weight at (B 1, N 40, inverse), where the fp32 tensor-op path is at 3.1e-7 of float64); the identity
    layer's d sd2 at most 2.2e-6."""
    nets = _gpu()
    h, t, t32 = (_run(nets, n_flows, G, B, N, mode, impl, seed=H.SEED, mutate=H.hostile_flow, variant=variant)
                 for impl in ("hip", "torch64", "torch"))
    _compare(h, t, t32, (n_flows, G, B, N, mode, "hostile", variant))
    assert h["precision"] == "f16x3"
    prefixes = H.layer_prefixes(t["grads"])
    assert len(prefixes) == 3 * n_flows
    G64, Gh = t["grads"], h["grads"]
    live_zero = 0
    for pre in prefixes:
        for br in FO.BRANCHES:
            t0 = "%sT_%s_0.%s_" % (pre, br, br)
            w0, g0, b0, w1 = t0 + "sd0.weight", t0 + "sd0_bn.weight", t0 + "sd0_bn.bias", t0 + "sd1.weight"
            if G64[g0] is None:                            # a net the loss does not reach (direct mode: the last layer's mu net)
                continue
            r, _ = H.roles(H.SEED, pre, br)
            z, d = r["zero"], r["dead"]
            # the project's measure: the entry's error over the TENSOR's scale.  That holds the entry itself to GRAD * scale / |ref|:
            # it is counted as checked only where it is at least 1e-2 of the scale (the entry then within 2 % of itself; a kernel
            # that divided by gamma0 or dropped the term is far outside).  In the identity layer's nets no gradient reaches the
            # conditioner: d gamma0 is an all-zero tensor there and the comparison is 0 against 0.
            got, ref, scale = float(Gh[g0][z]), float(G64[g0][z]), float(G64[g0].abs().max())
            assert math.isfinite(got) and abs(got - ref) <= GRAD * scale, (g0, "gamma0 = 0", got, ref, scale)
            if scale == 0.0:
                assert pre == prefixes[H.ID_LAYER] and got == 0.0, g0
            elif abs(ref) >= 1e-2 * scale:
                assert got != 0.0 and abs(got - ref) <= 100 * GRAD * abs(ref), (g0, got, ref)
                live_zero += 1
            assert float(G64[w0][0, z].abs().max()) == 0.0 and float(Gh[w0][0, z].abs().max()) == 0.0, (w0, "row of gamma0 = 0")
            for k, a64, a in ((w1, G64[w1][0, :, d], Gh[w1][0, :, d]), (b0, G64[b0][d], Gh[b0][d]), (g0, G64[g0][d], Gh[g0][d])):
                assert float(a64.abs().max()) == 0.0 and float(a.abs().max()) == 0.0, (k, "dead unit")
    assert live_zero >= 4, live_zero                        # d gamma0 = sum dh0 xhat does not involve gamma0 (float64: 7 to 10 of the 9 to 10 reached nets)
    for br in FO.BRANCHES:
        for leaf in ("weight", "bias"):
            k = "%sT_%s_1.%s_sd2.%s" % (prefixes[H.ID_LAYER], br, br, leaf)
            assert G64[k] is not None and float(G64[k].abs().max()) > 0.0, k
            r_ = rel(Gh[k], G64[k], bias_floor(G64, k))
            print("GRADREL identity layer", k, r_)
            assert r_ <= GRAD, (k, r_)


def test_repeated_calls_are_bit_identical():
    """4"""
    nets = _gpu()
    a = _run(nets, 2, 128, 3, 1000, "direct", "hip")
    _RUNS.pop((2, 128, 3, 1000, "direct", "hip", False, 5, None, None))
    b = _run(nets, 2, 128, 3, 1000, "direct", "hip")
    assert torch.equal(a["gp"], b["gp"]) and torch.equal(a["gg"], b["gg"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_flat_store_and_truncated_stack():
    """5: after flatten_parameters() the gradients land in the store's gradient buffer and equal the unflattened run; n_layers = 14
    of n_flows = 5 matches forward_torch restricted to those 14 layers."""
    nets = _gpu()
    a = _run(nets, 2, 128, 3, 1000, "direct", "hip")
    b = _run(nets, 2, 128, 3, 1000, "direct", "hip", flat=True)
    assert torch.equal(a["gp"], b["gp"]) and torch.equal(a["gg"], b["gg"])
    store = b["store"]
    assert float(store.flat_g.abs().max()) > 0
    for k in a["grads"]:
        assert b["grad_storage"][k] == store.flat_g.untyped_storage().data_ptr(), k
        assert torch.equal(b["grads"][k], a["grads"][k]), k
    sd = FO.to_torch(FO.make_decoder_state(7, 5, 64, 128))
    tgt, z, g = FO.synthetic_inputs(7, 2, 100, 128)
    out = {}
    for impl in ("hip", "torch64"):
        dec = nets.LocalCondRNVPDecoder(5, 64, 128, weight_std=0.01)
        dec.load_state_dict(sd, strict=True)
        dec = dec.cuda().eval()
        tp, tg = torch.from_numpy(z.copy()).cuda(), torch.from_numpy(g.copy()).cuda()
        if impl == "torch64":
            dec, tp, tg = dec.double(), tp.double(), tg.double()
        tp.requires_grad_(True)
        tg.requires_grad_(True)
        if impl == "hip":
            dec.eval_autograd = "hip"
            ps, mus, lvs = dec(tp, tg, mode="direct", n_layers=14)
            assert len(ps) == 14
        else:
            ps, cur = [], tp
            lvs = []
            for lyr in dec.coupling_layers()[:14]:
                cur, _, lv = lyr.forward_torch(cur, tg, "direct")
                ps.append(cur)
                lvs.append(lv)
        (ps[-1].square().mean() + sum(lvs).mean()).backward()
        out[impl] = (ps[-1].detach(), tp.grad, tg.grad)
    assert rel(out["hip"][0], out["torch64"][0]) <= OUT
    close_but_kinks(out["hip"][1], out["torch64"][1], GRAD, "grad_p n_layers=14")
    assert rel(out["hip"][2], out["torch64"][2]) <= GRAD


def test_through_chamfer_consumer():
    """6: dec(z, g, "direct") -> nn_distance -> mean; dL/d out is taken once from this graph and fed, as float64, into the float64
    tensor-op path, so a Chamfer argmin tie cannot enter."""
    nets = _gpu()
    from dpf_nets_amd.metrics.StructuralLosses.nn_distance import nn_distance
    B, N, G = 2, 256, 128
    sd = FO.to_torch(FO.make_decoder_state(3, 2, 64, G))
    tgt, z, g = FO.synthetic_inputs(3, B, N, G)
    dec = nets.LocalCondRNVPDecoder(2, 64, G, weight_std=0.01)
    dec.load_state_dict(sd, strict=True)
    dec = dec.cuda().eval()
    dec.eval_autograd = "hip"
    tz, tg = torch.from_numpy(z.copy()).cuda().requires_grad_(True), torch.from_numpy(g.copy()).cuda().requires_grad_(True)
    target = torch.from_numpy(tgt.copy()).cuda().transpose(1, 2).contiguous()
    ps, _, _ = dec(tz, tg, mode="direct")
    out = ps[-1]
    out.retain_grad()
    d1, d2 = nn_distance(out.transpose(1, 2).contiguous(), target)[:2]
    (d1.mean() + d2.mean()).backward()
    dout = out.grad.double()
    dec64 = nets.LocalCondRNVPDecoder(2, 64, G, weight_std=0.01)
    dec64.load_state_dict(sd, strict=True)
    dec64 = dec64.cuda().eval().double()
    z64, g64 = tz.detach().double().requires_grad_(True), tg.detach().double().requires_grad_(True)
    ps64, _, _ = dec64.forward_torch(z64, g64, mode="direct")
    ps64[-1].backward(dout)
    close_but_kinks(tz.grad, z64.grad, GRAD, "dL/dz")
    assert rel(tg.grad, g64.grad) <= GRAD, rel(tg.grad, g64.grad)


def test_sample_and_decode():
    """7: the gradient reaches mu0 and logvar0; equal to the two-call tensor-op formulation; no warning."""
    nets = _gpu()
    B, N, G = 2, 100, 128
    sd = FO.to_torch(FO.make_decoder_state(4, 2, 64, G))
    _, z, g = FO.synthetic_inputs(4, B, N, G)
    noise = torch.from_numpy(z.copy()).cuda()
    res = {}
    for impl in ("hip", "torch64"):
        dec = nets.LocalCondRNVPDecoder(2, 64, G, weight_std=0.01)
        dec.load_state_dict(sd, strict=True)
        dec = dec.cuda().eval()
        dt = torch.float64 if impl == "torch64" else torch.float32
        dec = dec.to(dt)
        mu0 = torch.full((B, 3, 1), 0.1, device="cuda", dtype=dt).requires_grad_(True)
        lv0 = torch.full((B, 3, 1), -0.5, device="cuda", dtype=dt).requires_grad_(True)
        tg = torch.from_numpy(g.copy()).cuda().to(dt)
        if impl == "hip":
            dec.eval_autograd = "hip"
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                zz, ps, mus, lvs = dec.sample_and_decode(mu0.expand(B, 3, N), lv0.expand(B, 3, N), tg, noise=noise)
            _no_warning(caught)
        else:
            zz = noise.to(dt) * torch.exp(0.5 * lv0.expand(B, 3, N)) + mu0.expand(B, 3, N)
            ps, mus, lvs = dec.forward_torch(zz, tg, mode="direct")
        (ps[-1].square().mean() + sum(lvs).mean()).backward()
        res[impl] = (mu0.grad, lv0.grad)
    assert rel(res["hip"][0], res["torch64"][0]) <= GRAD and rel(res["hip"][1], res["torch64"][1]) <= GRAD


def test_defaults_untouched():
    """8: a default-constructed module still warns and takes tensor ops; under no_grad "hip" takes the fused stack, bit for bit."""
    nets = _gpu()
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    dec = nets.LocalCondRNVPDecoder(1, 64, 128).cuda().eval()
    assert dec.eval_autograd == "torch"
    p = (torch.randn(2, 3, 64, device="cuda") * 0.3)
    g = torch.randn(2, 128, device="cuda")
    with pytest.warns(EvalModeAutogradWarning):
        ps, _, _ = dec(p.clone().requires_grad_(True), g, mode="inverse")
    assert isinstance(ps, list) and ps[0].grad_fn is not None
    with torch.no_grad():
        a = dec(p, g, mode="direct")[0][-1].clone()
        dec.eval_autograd = "hip"
        b = dec(p, g, mode="direct")[0][-1]
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,G", [(1, 128), (5, 512), (33, 128)])
def test_film_frozen_entries_vs_tensor_ops(B, G):
    """dpf_film_frozen_forward / _backward (one launch each way, B >= 1) against the batched tensor-op formulation in float64; d g
    is summed over the K nets inside the launch, the same bits on a second call; accumulate adds."""
    _gpu()
    from dpf_nets_amd._lib import lib, check, current_stream
    from dpf_nets_amd.networks.frozen_engine import _film_forward, _film_backward
    K, F = 12, 64
    gen = torch.Generator(device="cuda").manual_seed(B * 1000 + G)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    g, W0, gam, bet = rnd(B, G), rnd(K, F, G) * 0.1, 1 + 0.1 * rnd(K, 1, F), 0.1 * rnd(K, 1, F)
    W1, b1, rm, rv, dfm = rnd(K, F, F) * 0.1, 0.1 * rnd(K, 1, F), 0.1 * rnd(K, 1, F), 0.5 + torch.rand(K, 1, F, device="cuda", generator=gen), rnd(K, B, F)
    d = lambda *ts: [t.double() for t in ts]
    fm64, xhat64, y64, sig64, sw64 = _film_forward(*d(g, W0, gam, bet, W1, b1, rm), torch.rsqrt(rv.double() + 1e-5))
    ref = _film_backward(*d(dfm, g, W0, gam, W1), torch.rsqrt(rv.double() + 1e-5), xhat64, y64, sig64, sw64, True)
    L_, st = lib(), current_stream()
    fm, xhat, rstd = torch.empty(K, B, F, device="cuda"), torch.empty(K, B, F, device="cuda"), torch.empty(K, 1, F, device="cuda")
    check(L_.dpf_film_frozen_forward(K, B, G, *(t.data_ptr() for t in (g, W0, gam, bet, W1, b1, rm, rv)), 1e-5, fm.data_ptr(),
                                     xhat.data_ptr(), rstd.data_ptr(), st), "film_frozen_forward")
    assert rel(fm, fm64) <= 1e-5 and rel(xhat, xhat64) <= 1e-5
    work = torch.empty(L_.dpf_film_frozen_workspace_floats(K, B, G), device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")

    def backward(accumulate, outs=None):
        outs = outs or [torch.empty(K, F, G, device="cuda"), torch.empty(K, F, device="cuda"), torch.empty(K, F, device="cuda"),
                        torch.empty(K, F, F, device="cuda"), torch.empty(K, F, device="cuda")]
        dg = torch.empty(B, G, device="cuda")
        check(L_.dpf_film_frozen_backward(K, B, G, *(t.data_ptr() for t in (g, W0, gam, bet, W1, xhat, rstd, dfm)),
                                          *(t.data_ptr() for t in outs), dg.data_ptr(), work.data_ptr(), ticket.data_ptr(),
                                          accumulate, st), "film_frozen_backward")
        return outs + [dg]
    got = backward(0)
    for a, b, name in zip(got, ref, ("dW0", "dgamma", "dbeta", "dW1", "db1", "dg")):
        assert rel(a, b.reshape(a.shape)) <= 2e-5, (name, rel(a, b.reshape(a.shape)))
    assert int(ticket) == 0
    again = backward(0)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    twice = backward(1, [t.clone() for t in got[:5]])
    for a, b in zip(twice[:5], got[:5]):
        assert rel(a, 2 * b.double()) <= 1e-6
