"""The eval-mode autograd path of the latent prior flow on HIP (`eval_autograd = "hip"`: csrc/gprior_frozen.hip through
networks/prior_frozen_engine.py): GlobalRNVPDecoder / RealNVPFlowCouple / RealNVPFlow with FROZEN BatchNorm statistics as ONE
autograd node, against

  * float64 autograd through the pinned CPU oracle (tests/gprior_frozen_ref.py; itself pinned for gradients by
    tests/test_gprior_frozen_cpu.py), both modes, the config's shape, ragged / odd shapes, one row, K = 1,
  * the module's own tensor-op path in float64 on the GPU for a loss that uses only some outputs,
  * vectors captured from the reference's module in eval() mode (tests/golden/gprior_frozen.npz),
  * itself: parameters-only calls, accumulation, bit-reproducibility, the flat parameter store, the C ABI.

Bars (tests/test_gpu_gprior.py's): outputs and d/dg 1e-4, parameter gradients 1e-3, max-abs error over the reference's max-abs.
The fp32 tensor-op path itself is within 3.2e-6 of float64 on every tensor of the ten cases of the first test."""
import copy
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO
from tests.gprior_frozen_ref import NAMES, oracle64, projection_loss, projection_weights, rel
from tests.gprior_train_ref import hostile_bn, make_state

pytestmark = pytest.mark.gpu

TOL = 1e-4
PGRAD = 1e-3


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def _no_warning(caught):
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    assert not any(issubclass(w.category, EvalModeAutogradWarning) for w in caught)


def _warned(caught):
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    assert any(issubclass(w.category, EvalModeAutogradWarning) for w in caught)


def _decoder(nets, seed, n_flows, nf, G, impl="hip", mutate=None):
    dec = nets.GlobalRNVPDecoder(n_flows, nf, G)
    dec.load_state_dict(FO.to_torch(make_state(seed, n_flows, nf, G, mutate)), strict=True)
    dec = dec.cuda().eval()
    dec.eval_autograd = impl
    return dec


def _call(dec, g, mode):
    """One call that must be the HIP node: no warning."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = dec(g, mode=mode)
    _no_warning(caught)
    return out


def _seed(G, B):
    return 500 + G + B


_RUNS = {}


def _run(nets, n_flows, nf, G, B, mode, fresh=False, mutate=None):
    """Forward + backward of the seeded projection loss through the HIP node with g requiring grad.  Cached unless fresh."""
    key = (n_flows, nf, G, B, mode) + (() if mutate is None else (mutate.__name__,))
    if not fresh and key in _RUNS:
        return _RUNS[key]
    seed = _seed(G, B)
    dec = _decoder(nets, seed, n_flows, nf, G, mutate=mutate)
    g = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda().requires_grad_(True)
    lists = _call(dec, g, mode)
    projection_loss(lists, seed).backward()
    res = dict(dec=dec, g=g, lists=lists, outs=[torch.stack(list(lst)).detach() for lst in lists], dg=g.grad.clone(),
               grads={k: p.grad.clone() for k, p in dec.named_parameters()})
    if not fresh:
        _RUNS[key] = res
    return res


def _check_vs_oracle(outs, dg, grads, ref, what):
    for name, got in zip(NAMES, outs):
        r = rel(got, ref[name])
        print("REL", what, name, r)
        assert r <= TOL, (what, name, r)
    r = rel(dg, ref["dg"])
    print("REL", what, "dg", r)
    assert r <= TOL, (what, r)
    assert set(grads) == set(ref["grads"])
    worst = 0.0
    for k, v in grads.items():
        assert v is not None and bool(torch.isfinite(v).all()), (what, k)
        if np.abs(ref["grads"][k]).max() > 0:
            worst = max(worst, rel(v, ref["grads"][k].reshape(tuple(v.shape))))
    print("REL", what, "parameters", worst)
    assert worst <= PGRAD, (what, worst)


CASES = [(7, 128, 128, 64), (3, 40, 24, 301), (2, 256, 64, 1), (1, 8, 2, 3), (2, 16, 8, 5)]


@pytest.mark.parametrize("mode", ["direct", "inverse"])
@pytest.mark.parametrize("n_flows,nf,G,B", CASES)
def test_stack_vs_float64_oracle(n_flows, nf, G, B, mode):
    nets = _gpu()
    run = _run(nets, n_flows, nf, G, B, mode)
    assert all(isinstance(lst, list) and len(lst) == 2 * n_flows for lst in run["lists"])
    from dpf_nets_amd.networks.losses import total_logvar
    assert rel(total_logvar(run["lists"][2]), run["outs"][2].sum(0)) <= TOL       # the tagged layer sum (GaussianFlowNLL's route)
    with torch.no_grad():
        plain = run["dec"](run["g"], mode=mode)
    for got, p in zip(run["outs"], plain):
        assert torch.equal(got, p.stacked)                          # the forward IS the fused eval launch
    _check_vs_oracle(run["outs"], run["dg"], run["grads"], oracle64(_seed(G, B), n_flows, nf, G, B, mode), (n_flows, nf, G, B, mode))


@pytest.mark.parametrize("mode", ["direct", "inverse"])
@pytest.mark.parametrize("n_flows,nf,G,B", [(1, 8, 2, 3), (2, 16, 8, 5)])
def test_stack_vs_float64_oracle_hostile(n_flows, nf, G, B, mode):
    """The two smallest cases above under tests/gprior_train_ref.hostile_bn -- negative and exactly zero mlp0_bn.weight entries and a
    dead hidden unit in every net -- at the same bars: the closed-form d gamma, d W0 and d beta of csrc/gprior_frozen.hip hold for
    gamma <= 0 only if their signs do.  The zero-gamma unit's d gamma is live and its d W0 row exactly 0."""
    nets = _gpu()
    run = _run(nets, n_flows, nf, G, B, mode, mutate=hostile_bn)
    with torch.no_grad():
        plain = run["dec"](run["g"], mode=mode)
    for got, p in zip(run["outs"], plain):
        assert torch.equal(got, p.stacked)
    ref = oracle64(_seed(G, B), n_flows, nf, G, B, mode, mutate=hostile_bn)
    _check_vs_oracle(run["outs"], run["dg"], run["grads"], ref, (n_flows, nf, G, B, mode, "hostile"))
    for k, v in run["grads"].items():
        r = ref["grads"][k]
        if k.endswith("mlp0_bn.weight"):
            assert float(run["dec"].state_dict()[k][0]) == 0.0 and r[0] != 0.0 and float(v[0]) != 0.0, (k, r[0], float(v[0]))
        elif k.endswith("mlp0.weight"):
            assert not r[0].any() and not v[0].any(), k                    # gamma = 0: the d W0 row is exactly 0


@pytest.mark.parametrize("n_flows,nf,G,B,mode", [(3, 40, 24, 301, "inverse"), (2, 16, 8, 5, "direct")])
def test_parameters_only(n_flows, nf, G, B, mode):
    """Fine-tuning with frozen statistics: g does not require grad, the parameters do."""
    nets = _gpu()
    run = _run(nets, n_flows, nf, G, B, mode)
    seed = _seed(G, B)
    dec = _decoder(nets, seed, n_flows, nf, G)
    before = {k: v.clone() for k, v in dec.named_buffers()}
    lists = _call(dec, run["g"].detach(), mode)
    assert all(t.grad_fn is not None for lst in lists for t in lst)
    projection_loss(lists, seed).backward()
    for k, p in dec.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert torch.equal(p.grad, run["grads"][k]), k
    after = dict(dec.named_buffers())
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert all(int(v) == 0 for k, v in after.items() if "num_batches" in k)
    # the default keeps today's behaviour: autograd follows the input only
    dec.eval_autograd = "torch"
    lists = dec(run["g"].detach(), mode=mode)
    assert all(t.grad_fn is None for lst in lists for t in lst)


def _partial_loss(gs, mus, lvs, mode):
    first = gs[0] if mode == "inverse" else gs[-1]
    return first, first.square().mean() + sum(lvs).mean() + 1e-3 * (0.5 * mus[1]).sum()


@pytest.mark.parametrize("n_flows,nf,G,B,mode", [(7, 128, 128, 50, "direct"), (2, 24, 20, 130, "inverse")])
def test_partial_use_and_accumulation(n_flows, nf, G, B, mode):
    """A loss that leaves None gradients for most outputs and routes the layer sum through the tag, against forward_torch in
    float64 on the GPU; two backward passes without zero_grad give twice the gradient."""
    nets = _gpu()
    seed = _seed(G, B)
    dec = _decoder(nets, seed, n_flows, nf, G)
    d64 = copy.deepcopy(dec).double()
    g0 = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda()
    g64 = g0.double().requires_grad_(True)
    f64, loss = _partial_loss(*d64.forward_torch(g64, mode), mode)
    loss.backward()
    ref = [p.grad for p in d64.parameters()]
    for it in (1, 2):
        g = g0.clone().requires_grad_(True)
        first, loss = _partial_loss(*_call(dec, g, mode), mode)
        loss.backward()
        assert rel(first, f64) <= TOL and rel(g.grad, g64.grad) <= TOL
        worst = max(rel(p.grad, it * r) for p, r in zip(dec.parameters(), ref) if float(r.abs().max()) > 0)
        print("REL partial", (n_flows, nf, G, B, mode), it, rel(g.grad, g64.grad), worst)
        assert worst <= PGRAD, (it, worst)
    # the tagged layer sum is the route GaussianFlowNLL takes
    from dpf_nets_amd.networks.losses import total_logvar
    g = g0.clone().requires_grad_(True)
    total_logvar(_call(dec, g, mode)[2]).mean().backward()
    g64.grad = None
    sum(d64.forward_torch(g64, mode)[2]).mean().backward()
    assert rel(g.grad, g64.grad) <= TOL


def test_bit_reproducible():
    nets = _gpu()
    a = _run(nets, 3, 40, 24, 301, "inverse", fresh=True)
    b = _run(nets, 3, 40, 24, 301, "inverse", fresh=True)
    assert torch.equal(a["dg"], b["dg"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_flat_parameter_store():
    nets = _gpu()
    n_flows, nf, G, B = 3, 32, 16, 9
    seed = _seed(G, B)
    ref = _decoder(nets, seed, n_flows, nf, G)
    flat = copy.deepcopy(ref)
    store = flat.flatten_parameters()
    assert flat.flat_store() is store and store.attached()
    g0 = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda()
    from dpf_nets_amd.networks import prior_frozen_engine as PE
    calls = []
    orig = PE._GPriorFrozenFlat.apply
    PE._GPriorFrozenFlat.apply = staticmethod(lambda *a: (calls.append(1), orig(*a))[1])
    try:
        dgs = []
        for dec in (ref, flat):
            g = g0.clone().requires_grad_(True)
            projection_loss(_call(dec, g, "inverse"), seed).backward()
            dgs.append(g.grad)
    finally:
        PE._GPriorFrozenFlat.apply = orig
    assert len(calls) == 1, "the flat node was not taken"
    assert store.grad_written and torch.equal(dgs[0], dgs[1])
    lo, hi = store.flat_g.data_ptr(), store.flat_g.data_ptr() + 4 * store.flat_g.numel()
    for (k, a), (_, b) in zip(ref.named_parameters(), flat.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
        assert lo <= b.grad.data_ptr() < hi and b.grad.untyped_storage().data_ptr() == store.flat_g.untyped_storage().data_ptr(), k
    assert flat.flows[0].nvp1.T_mu_0[0].weight.grad.data_ptr() == store.flat_g.data_ptr()
    # three optimizer steps in eval mode: bit-identical parameters, and the next forward sees them
    for dec in (ref, flat):
        opt = nets.Adam(dec.parameters(), lr=1e-2, weight_decay=1e-6, betas=(0.9, 0.995), amsgrad=True)
        for it in range(3):
            opt.zero_grad()
            g = g0.clone().requires_grad_(True)
            gs, mus, lvs = _call(dec, g, "inverse")
            (gs[0].square().mean() + sum(lvs).mean() + _call(dec, g, "direct")[0][-1].abs().mean()).backward()
            opt.step()
    assert store.attached()
    for (k, a), b in zip(ref.state_dict().items(), flat.state_dict().values()):
        assert torch.equal(a, b), k
    for dec in (ref, flat):
        got = _call(dec, g0, "direct")
        with torch.no_grad():
            tor = dec.forward_torch(g0, "direct")
        for a, b in zip(got, tor):
            assert rel(torch.stack(a), torch.stack(b)) <= TOL


def _randomise_bn(module):
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5)
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.1)


def test_single_modules_and_fallbacks():
    nets = _gpu()
    torch.manual_seed(4)
    G, nf, B = 12, 10, 7
    g0 = torch.randn(B, G, device="cuda")
    cp = nets.RealNVPFlowCouple(nf, G, weight_std=0.1, pattern=1).cuda().eval()
    one = nets.RealNVPFlow(nf, G, weight_std=0.1, warp_inds=list(range(0, G, 2))).cuda().eval()
    for mod, n in ((cp, 2), (one, 1)):
        _randomise_bn(mod)
        mod.eval_autograd = "hip"
        m64 = copy.deepcopy(mod).double()
        r = [torch.randn(n, B, G, device="cuda") for _ in range(3)]
        for mode in ("direct", "inverse"):
            mod.zero_grad(); m64.zero_grad()
            g, g64 = g0.clone().requires_grad_(True), g0.double().requires_grad_(True)
            out, out64 = _call(mod, g, mode), m64.forward_torch(g64, mode)
            if n == 1:
                out, out64 = [[t] for t in out], [[t] for t in out64]
            sum((torch.stack(a) * w).sum() for a, w in zip(out, r)).backward()
            sum((torch.stack(a) * w.double()).sum() for a, w in zip(out64, r)).backward()
            for a, b in zip(out, out64):
                assert rel(torch.stack(a), torch.stack(b)) <= TOL
            assert rel(g.grad, g64.grad) <= TOL
            worst = max(rel(p.grad, q.grad) for p, q in zip(mod.parameters(), m64.parameters()) if float(q.grad.abs().max()) > 0)
            assert worst <= PGRAD, (n, mode, worst)
    # outside the limits: tensor operations, and loud
    odd = nets.RealNVPFlow(nf, G, weight_std=0.1, warp_inds=[0, 3]).cuda().eval()
    odd.eval_autograd = "hip"
    dbl = _decoder(nets, 3, 2, 16, 8).double()
    assert dbl.eval_autograd == "hip"
    for mod, g in ((odd, g0.clone().requires_grad_(True)),
                   (dbl, torch.from_numpy(GO.gprior_inputs(3, 5, 8)).double().cuda().requires_grad_(True))):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = mod(g, mode="direct")
        _warned(caught)
        first = out[0] if mod is odd else out[0][-1]
        assert first.grad_fn is not None and first.dtype == g.dtype
    # no autograd: the fused launch, as the default module
    from dpf_nets_amd.networks.flowlist import FlowList
    hip, tor = _decoder(nets, 3, 2, 16, 8), _decoder(nets, 3, 2, 16, 8, impl="torch")
    g = torch.from_numpy(GO.gprior_inputs(3, 5, 8)).cuda().requires_grad_(True)
    with torch.no_grad():
        a, b = hip(g, mode="inverse"), tor(g, mode="inverse")
    assert all(isinstance(x, FlowList) for x in a) and all(torch.equal(x.stacked, y.stacked) for x, y in zip(a, b))


def _param_blocks(n_flows, nf, G, params_only):
    """[(reference parameter name, offset, numel)] inside the gradient block, the block's floats, and the running-statistics slots."""
    K, out, stat_slots, off = G // 2, [], [], 0
    for prefix, warp, keep in GO.step_plan(n_flows, G):
        for br in ("mu", "logvar"):
            base = "%sT_%s_0.%s_" % (prefix, br, br)
            for name, n in (("mlp0.weight", nf * K), ("mlp0_bn.weight", nf), ("mlp0_bn.bias", nf)):
                out.append((base + name, off, n)); off += n
            if not params_only:
                stat_slots.append((off, 2 * nf)); off += 2 * nf
            for name, n in (("mlp1.weight", K * nf), ("mlp1.bias", K)):
                out.append((base + name, off, n)); off += n
    return out, off, stat_slots


def test_c_abi():
    _gpu()
    from dpf_nets_amd._lib import lib, check, current_stream
    from tests.test_gpu_gprior import _canon, _codes
    L = lib()
    n_flows, nf, G, B = 2, 16, 8, 5
    seed, S = _seed(G, B), 4
    state = GO.make_gprior_state(seed, n_flows, nf, G)
    canon = torch.from_numpy(_canon(state, n_flows, G)).cuda()
    packed = torch.empty(L.dpf_gprior_packed_floats(S, G, nf), dtype=torch.float32, device="cuda")
    check(L.dpf_gprior_pack(S, G, nf, 1e-5, canon.data_ptr(), packed.data_ptr(), current_stream()), "pack")
    g = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda()
    codes = (ctypes.c_int * S)(*_codes(n_flows))
    r = projection_weights(seed, S, B, G, device="cuda")
    assert L.dpf_gprior_frozen_workspace_floats(S, B, G, nf) == S * B * (6 * nf + G)
    ws = torch.empty(L.dpf_gprior_frozen_workspace_floats(S, B, G, nf), dtype=torch.float32, device="cuda")
    # the parameters-only layout and the running statistics as a block of their own
    blocks0, total0, stat_slots = _param_blocks(n_flows, nf, G, False)
    blocks1, total1, _ = _param_blocks(n_flows, nf, G, True)
    assert total0 == canon.numel()
    ponly = torch.cat([canon[o:o + n] for (_, o, n) in blocks0])
    stats = torch.cat([canon[o:o + n] for o, n in stat_slots])
    assert ponly.numel() == total1
    for mi, mode in enumerate(("direct", "inverse")):
        gs, mus, lvs = (torch.empty((S, B, G), device="cuda") for _ in range(3))
        check(L.dpf_gprior_forward(S, B, G, nf, mi, codes, packed.data_ptr(), g.data_ptr(), gs.data_ptr(), mus.data_ptr(),
                                   lvs.data_ptr(), None, None, GO.EPS, current_stream()), "forward")
        ref = oracle64(seed, n_flows, nf, G, B, mode)
        for params_only, block, st, blocks in ((0, canon, None, blocks0), (1, ponly, stats, blocks1)):
            dg = torch.full((B, G), float("nan"), device="cuda")
            dcanon = torch.full_like(block, float("nan"))
            check(L.dpf_gprior_frozen_backward(S, B, G, nf, mi, codes, params_only, block.data_ptr(), st.data_ptr() if st is not None else None,
                                               1e-5, GO.EPS, g.data_ptr(), gs.data_ptr(), mus.data_ptr(), lvs.data_ptr(), r[0].data_ptr(),
                                               r[1].data_ptr(), r[2].data_ptr(), dg.data_ptr(), dcanon.data_ptr(), ws.data_ptr(),
                                               current_stream()), "frozen_backward")
            grads = {k: dcanon[o:o + n] for k, o, n in blocks}
            refs = dict(ref, grads={k: v.reshape(-1) for k, v in ref["grads"].items()})
            _check_vs_oracle((gs, mus, lvs), dg, grads, refs, ("c_abi", mode, params_only))
            if not params_only:
                for o, n in stat_slots:
                    assert bool((dcanon[o:o + n] == 0).all())
        # NULL gradient tables are zeros
        dg0, dc0 = torch.full((B, G), float("nan"), device="cuda"), torch.full_like(canon, float("nan"))
        check(L.dpf_gprior_frozen_backward(S, B, G, nf, mi, codes, 0, canon.data_ptr(), None, 1e-5, GO.EPS, g.data_ptr(), gs.data_ptr(),
                                           mus.data_ptr(), lvs.data_ptr(), None, None, None, dg0.data_ptr(), dc0.data_ptr(), ws.data_ptr(),
                                           current_stream()), "frozen_backward")
        assert bool((dg0 == 0).all()) and bool((dc0 == 0).all())
    # argument errors come back as codes, nothing is launched
    p = ws.data_ptr()

    def bad(S_=S, B_=B, G_=G, mode_=0, codes_=codes, po=0, canon_=p, stats_=p, g_=p, dg_=p, dcanon_=p, ws_=p):
        return L.dpf_gprior_frozen_backward(S_, B_, G_, nf, mode_, codes_, po, canon_, stats_, 1e-5, 1e-6, g_, p, p, p, None, None, None,
                                            dg_, dcanon_, ws_, None)
    assert bad(G_=7) != 0                                              # odd G
    assert bad(codes_=(ctypes.c_int * S)(0, 1, 4, 3)) != 0             # unknown step code
    assert bad(B_=-1) != 0
    assert bad(mode_=2) != 0
    assert bad(dg_=None) != 0 and bad(dcanon_=None) != 0 and bad(ws_=None) != 0 and bad(g_=None) != 0 and bad(canon_=None) != 0
    assert bad(po=1, stats_=None) != 0                                 # the parameters-only layout needs the statistics block
    assert bad(S_=0) != 0
    assert bad(B_=0) == 0 and bad(B_=0, dg_=None, dcanon_=None) == 0
    torch.cuda.synchronize()


def test_vs_reference_golden(golden_dir):
    """The HIP node against what the reference's own GlobalRNVPDecoder gave in eval() mode under autograd (B = 1 included)."""
    nets = _gpu()
    from oracle.gen_golden import _grad_projection
    gold = np.load(os.path.join(golden_dir, "gprior_frozen.npz"))
    meta = json.load(open(os.path.join(golden_dir, "gprior_frozen.json")))
    assert len(meta["cases"]) == 2
    for case, (seed, n_flows, nf, G, B) in meta["cases"].items():
        for mode in ("direct", "inverse"):
            tag = "%s_%s_" % (case, mode)
            dec = _decoder(nets, seed, n_flows, nf, G)
            g = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda().requires_grad_(True)
            lists = _call(dec, g, mode)
            for name, lst in zip(NAMES, lists):
                assert rel(torch.stack(lst), gold[tag + name]) <= TOL, (case, mode, name)
            projection_loss(lists, seed).backward()
            assert rel(g.grad, gold[tag + "dg"]) <= TOL, (case, mode, rel(g.grad, gold[tag + "dg"]))
            for k, v in _grad_projection([(k, p.grad.cpu()) for k, p in dec.named_parameters()], seed).items():
                ref = gold[tag + "gproj_" + k]
                np.testing.assert_allclose(v, ref, rtol=1e-3, atol=1e-4 * max(1.0, float(ref[2])), err_msg=case + mode + k)
