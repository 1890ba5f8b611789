"""The conditions the hostile states and clouds of tests/flow_hostile.py must satisfy before a kernel is judged on them, on every
(state, input, shape, mode) tuple the GPU tests use (test_gpu_flow_hostile.py, test_stack_vs_float64_tensor_ops_hostile of
test_gpu_flow_frozen.py) -- no GPU:

  * the float64 evaluation is finite, its points stay below F16_COORD_MAX (what the pack-time guard assumes of a coordinate), the
    identity layer, the keep channels and the dead unit give exact zeros, the saturated layer saturates on both sides;
  * the pack-time bound of networks/engine.py f16_in_range, restated on CPU tensors, stays below F16_LIMIT (f16x3 stays the served
    precision) with the scaled-up gamma0 within a factor 2 of it, and the restatement is the engine's;
  * the fp32 tensor operations themselves stay within close_but_kinks's cap of float64 at the bars the GPU tests use (outputs:
    REL["f16x3"]; the frozen tuples' grad_p: GRAD_REL["f16x3"]): the inputs are well-posed."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as FO
from tests import flow_hostile as H
from tests.test_gpu_flow import REL
from tests.test_gpu_flow_train import GRAD_REL, close_but_kinks

N_FLOWS = 2
FORWARD = [(B, N, G, mode) for (B, N, G) in [(1, 1, 128), (2, 33, 128), (3, 100, 128), (33, 64, 128), (3, 100, 512)] for mode in ("direct", "inverse")]
FROZEN = [(1, 40, 128, "inverse"), (3, 100, 128, "direct"), (33, 64, 128, "direct"), (3, 100, 512, "direct")]


def _f64(state):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in FO.to_torch(state).items()}


def test_mutator_is_deterministic_and_leaves_its_input_alone():
    base = FO.make_decoder_state(H.SEED, N_FLOWS, 64, 128)
    keep = {k: v.copy() for k, v in base.items()}
    a, b = H.hostile_flow(base, H.SEED), H.hostile_flow(base, H.SEED)
    assert all(np.array_equal(base[k], keep[k]) for k in base)
    assert set(a) == set(base) and all(np.array_equal(a[k], b[k]) and a[k].dtype == base[k].dtype for k in a)
    c = H.hostile_flow(base, H.SEED + 1)
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    one = H.hostile_flow(FO.make_layer_state(3, 64, 128, [0, 2]), 3)                  # a single layer's state
    assert H.guard_bound(one)[0] < H.F16_LIMIT


@pytest.mark.parametrize("G", [128, 512])
@pytest.mark.parametrize("train", [False, True])
def test_state_has_what_it_says(G, train):
    st = H.decoder_state(G, N_FLOWS, train=train)
    for li, pre in enumerate(H.layer_prefixes(st)):
        for br in FO.BRANCHES:
            t0 = "%sT_%s_0.%s_" % (pre, br, br)
            r, _ = H.roles(H.SEED, pre, br)
            g0, b0 = st[t0 + "sd0_bn.weight"], st[t0 + "sd0_bn.bias"]
            assert g0[r["zero"]] == 0.0 and not np.signbit(g0[r["zero"]]) and b0[r["zero"]] == 0.25
            assert 15 <= int((g0 < 0).sum()) <= 23
            for name, beta in (("dead", -0.5), ("const", 0.5)):
                assert not st[t0 + "sd0.weight"][0, r[name]].any() and b0[r[name]] == beta and st[t0 + "sd0_bn.running_mean"][r[name]] == 0.0
            assert not st[t0 + "sd1.weight"][0, r["zero_row1"]].any()
            w2, b2 = st["%sT_%s_1.%s_sd2.weight" % (pre, br, br)], st["%sT_%s_1.%s_sd2.bias" % (pre, br, br)]
            assert (li == H.ID_LAYER) == (not w2.any() and not b2.any())
            if not train:
                rv0, rv1 = st[t0 + "sd0_bn.running_var"], st[t0 + "sd1_bn.running_var"]
                assert rv0.min() < 1e-2 and rv0.max() > 40 and np.abs(st[t0 + "sd0_bn.running_mean"]).max() == 3.0
                assert rv1.min() < 0.011 and rv1.max() > 99
    bound, w1 = H.guard_bound(st)
    assert w1 < 65504.0
    if not train:
        assert 0.5 * H.F16_LIMIT < bound < H.F16_LIMIT, bound              # the scaled-up gamma0 sets it, and f16x3 is still served


def test_guard_restatement_is_the_engines():
    """FlowStack.f16_in_range on the module (CPU tensors) gives the bound of H.guard_bound, and no warning."""
    import warnings
    from dpf_nets_amd import networks as nets
    st = H.decoder_state(128, N_FLOWS)
    dec = nets.LocalCondRNVPDecoder(N_FLOWS, 64, 128)
    dec.load_state_dict(FO.to_torch(st), strict=True)
    stack = dec.eval().stack()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert stack.f16_in_range(torch.device("cpu"))
    bound, w1 = H.guard_bound(st)
    assert stack._f16_bound[0] == pytest.approx(bound, rel=1e-6) and stack._f16_bound[1] == pytest.approx(w1, rel=1e-6)
    # the guard reads |s0|: with EVERY gamma0 negative the engine and the restatement still agree, and the scaled-up one still sets it
    neg = {k: (-np.abs(v) if k.endswith("sd0_bn.weight") else v.copy()) for k, v in st.items()}
    dec = nets.LocalCondRNVPDecoder(N_FLOWS, 64, 128)
    dec.load_state_dict(FO.to_torch(neg), strict=True)
    stack = dec.eval().stack()
    assert stack.f16_in_range(torch.device("cpu"))
    bound, _ = H.guard_bound(neg)
    assert stack._f16_bound[0] == pytest.approx(bound, rel=1e-6) and 0.5 * H.F16_LIMIT < bound < H.F16_LIMIT


def _fp32_and_f64(G, B, N, mode, variant, with_grad):
    state, src, g = H.decoder_case(G, B, N, mode, variant, N_FLOWS)
    out = []
    for st, dt in ((_f64(state), torch.float64), (FO.to_torch(state), torch.float32)):
        p = torch.from_numpy(src).to(dt).requires_grad_(with_grad)
        with torch.set_grad_enabled(with_grad):
            ps, mus, lvs = FO.decoder(st, N_FLOWS, p, torch.from_numpy(g).to(dt), mode)
            if with_grad:                   # the loss of test_gpu_flow_frozen.py
                pm, pl = torch.zeros(B, 3, N, dtype=dt), torch.full((B, 3, N), -3.6, dtype=dt)
                smp = ps + [p] if mode == "inverse" else [p] + ps
                (FO.point_flow_nll(smp, [pm] + mus, [pl] + lvs) + 0.1 * (ps[2] * mus[4]).mean()).backward()
        out.append(([x.detach() for x in ps], [x.detach() for x in mus], [x.detach() for x in lvs], p.grad))
    return state, out[0], out[1]


@pytest.mark.parametrize("variant", H.VARIANTS)
@pytest.mark.parametrize("B,N,G,mode", FORWARD + [c for c in FROZEN if c not in FORWARD])
def test_tuple_is_finite_exact_where_it_must_be_and_well_posed(B, N, G, mode, variant):
    frozen = (B, N, G, mode) in FROZEN
    state, r64, r32 = _fp32_and_f64(G, B, N, mode, variant, frozen)
    ps, mus, lvs, gp = r64
    plan = FO.decoder_layer_plan(N_FLOWS)
    assert all(bool(torch.isfinite(x).all()) for lst in (ps, mus, lvs) for x in lst)
    assert max(float(x.abs().max()) for x in ps) < H.F16_COORD_MAX
    if (B, N, G, mode) in FORWARD:                                         # the cached yardstick of the GPU test is this evaluation
        ref = H.reference64(G, B, N, mode, variant, N_FLOWS)
        assert all(torch.equal(a, b) for x, y in zip(ref, r64[:3]) for a, b in zip(x, y))
    src = torch.from_numpy(H.decoder_case(G, B, N, mode, variant, N_FLOWS)[1]).double()

    def call_input(k):                      # what layer k's call received: the source or the layer executed before it
        first = 0 if mode == "direct" else len(plan) - 1
        return src if k == first else ps[k - 1 if mode == "direct" else k + 1]
    big_live = []                           # largest h0 of the guard-sized unit, in the nets where it is on for part of the points
    for k, (pre, warp) in enumerate(plan):
        keep = [c for c in range(3) if c not in warp]
        assert not mus[k][:, keep].any() and not lvs[k][:, keep].any(), k
        # the dead unit: BN0(W0 x) of its feature is exactly beta0 = -0.5 on every point, relu gives exactly 0
        x = call_input(k)[:, keep, :]
        for br in FO.BRANCHES:
            st = FO.sub_state(_f64(state), pre)
            t0 = "T_%s_0.%s_" % (br, br)
            h = FO.batch_norm(FO.shared_dot(st[t0 + "sd0.weight"], x), st[t0 + "sd0_bn.running_mean"], st[t0 + "sd0_bn.running_var"],
                              st[t0 + "sd0_bn.weight"], st[t0 + "sd0_bn.bias"], False)
            r, _ = H.roles(H.SEED, pre, br)
            on = float((h[:, r["big"]] > 0).double().mean())
            if 0.05 < on < 0.95:
                big_live.append(float(h[:, r["big"]].max()))
            assert bool((h[:, r["dead"]] == -0.5).all()) and bool((h[:, r["const"]] == 0.5).all()) and bool((h[:, r["zero"]] == 0.25).all())
    if B * N >= 40 and not (variant == "same" and B == 1):      # (one cloud of one repeated point: every unit is on or off)
        # the guard-sized gamma0 is no second dead unit: in several nets it switches over the points, and what it passes on is large
        # (|s0| in the hundreds on coordinates of 0.2 .. 4, of 8 .. 20 in the wide cloud: tens, hundreds)
        assert len(big_live) >= 2 and max(big_live) > (100.0 if variant == "wide" else 10.0), big_live
    assert not mus[H.ID_LAYER].any() and not lvs[H.ID_LAYER].any()
    p_in = call_input(H.ID_LAYER)
    s = torch.sqrt(torch.tensor(1e-6, dtype=torch.float32).double() + 1.0)
    assert torch.equal(ps[H.ID_LAYER], s * p_in if mode == "direct" else p_in / s)
    sat = lvs[H.SAT_LAYER][:, plan[H.SAT_LAYER][1]]
    assert float(sat[:, 0].min()) > 0.95 and float(sat[:, 1].max()) < -0.95        # softsign saturated, one side per warped channel
    # ---- well-posed: the fp32 tensor operations against float64 at the bars the GPU tests hold the kernels to
    for name, a64, a32 in zip(("ps", "mus", "lvs"), r64[:3], r32[:3]):
        for k in range(len(plan)):
            if float(a64[k].abs().max()) == 0.0:
                assert float(a32[k].abs().max()) == 0.0
                continue
            close_but_kinks(a32[k], a64[k], REL["f16x3"], (name, k))
    if frozen:
        close_but_kinks(r32[3], gp, GRAD_REL["f16x3"], "grad_p")
