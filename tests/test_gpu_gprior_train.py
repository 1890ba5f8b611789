"""The TRAINING-mode prior flow on HIP (csrc/gprior_train.hip behind prior_flows._GPriorTrain / _GPriorTrainFlat and the C ABI
dpf_gprior_train_forward / _backward) against float64, ELEMENTWISE, at the edges its kernels have:

  a. the module against the pinned oracle under float64 autograd (tests/gprior_train_ref.py, itself pinned by
     tests/test_gprior_train_cpu.py), both modes, at shapes on either side of the GEMM's 32 x 32 tile and its 64-wide k-chunk (the
     batch IS the k extent of the two weight-gradient products), of the column kernels' 32 columns x 8 row groups, with a column
     workgroup that straddles the two nets (nf = 40), K = 1 and odd K;
  b. the same with negative and zero BatchNorm scales and a hidden unit of zero batch variance (`hostile_bn`);
  c. the same where the log(eps + exp(.)) floor and its derivative are active (`floor_active`);
  d. ill-conditioned inputs (B = 2, 3 on K = 1; hidden means far above their spread), held to a multiple of the fp32 tensor-op
     path's own error on the same inputs;
  e. the C ABI on step-code sequences the module never emits (S = 1 of each code, odd S with a repeat) against a plain float64
     step; f. its two block layouts, bit for bit; g. each optional gradient table alone and none; h. NaN-filled buffers with
     sentinels behind every output and the workspace, kept coordinates exactly zero, bit-reproducibility;
  i. the flat parameter store on a hostile state, bit for bit.

Measure: `rel`, max-abs error over the reference's max-abs; no tensor is skipped, and a reference gradient that is identically zero
must be identically zero on the GPU.

Bars.  Ceiling (tests/test_gpu_gprior.py's): outputs and d/dg 1e-4, parameter gradients 1e-3, running statistics 1e-5.  The fp32
tensor-op path (`forward_torch`) measures, against float64 on the inputs of (a), (b), (c) with B >= 7: outputs 7.4e-7, d/dg 7.2e-7,
parameter gradients 1.24e-6, running statistics 1.3e-7.  The kernel sums in another order and its expf is not the host's, so it is
held to 16 x those, rounded: BAR = 2e-5 for outputs, d/dg and parameter gradients, STAT_BAR = 2e-6 -- in (a), (b), (c), (e), (g).
The four cases of R32_CASES are ill-conditioned for ANY fp32 evaluation (fp32 tensor ops: parameter gradients 3.5e-3 at B = 3, 5e-4
at B = 2, 3.5e-4 with offset inputs); there the fp32 tensor-op path's own error r32 is computed on the GPU on the same inputs, per
tensor, and the kernel is held to max(bar, 8 r32) (8: another summation order on a cancelling sum) -- above the ceiling only where
r32 itself is above it.  No other case uses that rule.

MEASURED on an MI355X, worst `rel` of the kernel per class (beside it the fp32 tensor-op path on the same inputs and GPU); every
comparison prints `REL <case> <tensor> <kernel> <r32>`:
                                   outputs            d/dg               parameter gradients   running statistics
  a. seeded, B >= 7                4.0e-7 (6.4e-7)    7.4e-7 (5.1e-7)    8.5e-7 (1.3e-6)       1.2e-7 (1.3e-7)
  b. hostile_bn                    3.7e-7 (6.2e-7)    3.1e-7 (3.8e-7)    6.1e-7 (8.7e-7)       1.2e-7 (1.2e-7)
  c. floor_active                  1.4e-6 (7.2e-7)    1.3e-6 (1.1e-6)    4.1e-6 (7.6e-6)       2.1e-6 (1.7e-6)  <- STAT_EXCEPTION
  d. R32_CASES                     1.3e-5 (1.4e-5)    1.3e-5 (1.3e-5)    2.9e-3 (2.1e-3)       5.4e-6 (6.9e-6)
  e-g. C ABI                       3.0e-7             2.2e-7             6.7e-6                -
  (gradients that cancel to float64 rounding, on their kind's scale: 3.4e-6)
Before this file the factor of the floor was formed as 1 - eps exp(-lv) everywhere; floor_active(2,40,6,9)inverse then measured
2.2e-4 on flows.0.nvp1.T_logvar_0.logvar_mlp0.weight against 7.6e-6 of the fp32 tensor ops (prep_kernel now forms exp(o) / (eps +
exp(o)) from a recomputed o where the floor is active: 4.1e-6).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO
from tests import gprior_train_ref as R
from tests.gprior_train_ref import NAMES, projection_loss, projection_weights, rel

pytestmark = pytest.mark.gpu

CEILING = {"out": 1e-4, "dg": 1e-4, "param": 1e-3, "stat": 1e-5}
BAR = 2e-5                      # outputs, d/dg, parameter gradients: 16 x the fp32 tensor-op path's worst error, rounded
STAT_BAR = 2e-6                 # running statistics: 16 x
BARS = {"out": BAR, "dg": BAR, "param": BAR, "stat": STAT_BAR}
R32_FACTOR = 8
# (n_flows, nf, G, B, g_offset): the ONLY cases held to max(bar, R32_FACTOR * r32)
R32_CASES = ((1, 8, 2, 2, 0.0), (1, 8, 2, 3, 0.0), (2, 40, 6, 9, 50.0), (2, 24, 20, 31, 50.0))
# The ONE place outside R32_CASES where the same rule holds: the running variances of the step that ends the inverse chain of the
# floored case.  exp(-lv / 2) ~ 1e3 on a floored coordinate, and lv ~ -13.8 is stored with 5e-7 of absolute rounding, so ANY fp32
# evaluation hands that step inputs that are 1e-6 off (measured: kernel 1.35e-6, fp32 tensor ops 7.2e-7, both far inside BAR);
# its batch variance is quadratic in them and dwarfs the old running value, so it carries twice that error -- the fp32 tensor ops
# themselves measure 1.6e-6 of STAT_BAR's 2e-6 there, the kernel 2.1e-6.  bn_swish_kernel's two-pass variance has no part in it.
STAT_EXCEPTION = ("floor_active(2,40,6,9)inverse", ("flows.0.nvp1.T_mu_0.mu_mlp0_bn.running_var",
                                                    "flows.0.nvp1.T_logvar_0.logvar_mlp0_bn.running_var"))
MODES = ("direct", "inverse")

SHAPES = [(1, 8, 2, 2), (1, 8, 2, 3), (2, 40, 6, 9), (2, 24, 20, 31), (1, 33, 66, 33), (2, 16, 8, 7), (3, 40, 24, 301),
          (2, 128, 512, 65), (7, 128, 128, 64), (2, 16, 8, 1030)]
HOSTILE_SHAPES = [(2, 40, 6, 9), (2, 24, 20, 31), (3, 40, 24, 301), (7, 128, 128, 64)]
FLOOR_CASES = [(2, 40, 6, 9, "direct"), (2, 24, 20, 31, "direct"), (3, 40, 24, 301, "direct"), (2, 40, 6, 9, "inverse")]
OFFSET_SHAPES = [(2, 40, 6, 9), (2, 24, 20, 31)]
ABI_SHAPES = [(40, 6, 9), (24, 20, 31)]                        # nf, G, B
ABI_CODES = [[0], [1], [2], [3], [3, 0, 2, 1, 1]]
GUARD, SENTINEL = 64, 12345.0
NOISE = 1e-12                   # a float64 gradient below this fraction of its kind's scale is rounding of a sum that cancels


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def _seed(G, B):
    return 700 + G + B


def _bar(cls, r32):
    """The class's bar, or for a case of R32_CASES max(bar, 8 r32) -- above the ceiling only if r32 itself is above it."""
    if r32 is None:
        return BARS[cls]
    bar = max(BARS[cls], R32_FACTOR * r32)
    return bar if r32 > CEILING[cls] else min(bar, CEILING[cls])


def _compare(case, cls, name, got, ref, r32_of=None, use_r32=False, kind_scale=None):
    """One tensor against float64: prints the REL line, then asserts the bar.  r32_of: the fp32 tensor-op path's value, always
    printed when given; it enters the bar only with use_r32 (the cases of R32_CASES).  kind_scale: see _abi_compare."""
    ref = np.asarray(ref, dtype=np.float64)
    got = got.detach().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), (case, name)
    if np.abs(ref).max() == 0:
        print("REL", case, name, "zero", "-")
        assert float(got.abs().max()) == 0.0, (case, name, "the reference is identically zero")
        return 0.0
    if kind_scale is not None and np.abs(ref).max() <= NOISE * kind_scale:
        r = float(got.abs().max()) / kind_scale
        print("REL", case, name, "%.3e" % r, "noise")
        assert r <= BARS[cls], (case, name, r, "the reference is zero but for float64 rounding")
        return r
    r = rel(got, ref)
    r32 = None if r32_of is None else rel(r32_of.detach().reshape(ref.shape), ref)
    print("REL", case, name, "%.3e" % r, "-" if r32 is None else "%.3e" % r32)
    bar = _bar(cls, r32 if use_r32 else None)
    assert r <= bar, (case, name, r, r32, bar)
    assert BARS[cls] <= bar and (bar <= CEILING[cls] or (use_r32 and r32 > CEILING[cls]))
    return r


def _decoder(nets, state, n_flows, nf, G, dev="cuda"):
    dec = nets.GlobalRNVPDecoder(n_flows, nf, G)
    dec.load_state_dict(FO.to_torch(state), strict=True)
    return dec.to(dev).train()


def _step(dec, g, mode, seed, node=None):
    """One training step of the seeded projection loss; `node` names the autograd node that must serve the call."""
    from dpf_nets_amd.networks import prior_flows as PF
    calls = []
    if node is not None:
        orig = getattr(PF, node).apply
        getattr(PF, node).apply = staticmethod(lambda *a: (calls.append(1), orig(*a))[1])
    try:
        lists = dec(g, mode=mode) if node is not None else dec.forward_torch(g, mode)
    finally:
        if node is not None:
            getattr(PF, node).apply = orig
    assert node is None or len(calls) == 1, "the HIP training path (%s) was not taken" % node
    assert all(isinstance(lst, list) and len(lst) == len(lists[0]) for lst in lists)
    projection_loss(lists, seed).backward()
    res = {name: torch.stack(list(lst)).detach() for name, lst in zip(NAMES, lists)}
    res["dg"] = g.grad
    res["grads"] = {k: p.grad for k, p in dec.named_parameters()}
    res["stats"] = {k: v for k, v in dec.state_dict().items() if "running" in k}
    res["tracked"] = [int(v) for k, v in dec.state_dict().items() if "num_batches" in k]
    return res


def _module_case(n_flows, nf, G, B, mode, mutate=None, g_offset=0.0, dev="cuda", node="_GPriorTrain"):
    nets = _gpu() if dev == "cuda" else __import__("dpf_nets_amd.networks", fromlist=["x"])
    use_r32 = (n_flows, nf, G, B, float(g_offset)) in R32_CASES
    assert use_r32 == (B < 7 or g_offset != 0.0), "the r32 rule is for the cases of R32_CASES and no others"
    seed = _seed(G, B)
    case = "%s%s(%d,%d,%d,%d)%s" % (getattr(mutate, "__name__", "seeded"), "+%g" % g_offset if g_offset else "", n_flows, nf, G, B, mode)
    state = R.make_state(seed, n_flows, nf, G, mutate)
    g0 = torch.from_numpy(R.inputs(seed, B, G, g_offset)).to(dev)
    dec = _decoder(nets, state, n_flows, nf, G, dev)
    t32 = _step(copy.deepcopy(dec), g0.clone().requires_grad_(True), mode, seed)              # the fp32 tensor-op path, same inputs
    got = _step(dec, g0.clone().requires_grad_(True), mode, seed, node)
    ref = R.oracle64_train(seed, n_flows, nf, G, B, mode, mutate, g_offset)
    for name in NAMES:
        _compare(case, "out", name, got[name], ref[name], t32[name], use_r32)
    _compare(case, "dg", "dg", got["dg"], ref["dg"], t32["dg"], use_r32)
    assert set(got["grads"]) == set(ref["grads"]) and len(ref["grads"]) == 10 * 2 * n_flows
    for k, v in got["grads"].items():
        assert v is not None, (case, k)
        _compare(case, "param", k, v, ref["grads"][k], t32["grads"][k], use_r32)
    assert set(got["stats"]) == set(ref["stats"]) and len(ref["stats"]) == 4 * 2 * n_flows
    for k, v in got["stats"].items():
        _compare(case, "stat", k, v, ref["stats"][k], t32["stats"][k], use_r32 or (case == STAT_EXCEPTION[0] and k in STAT_EXCEPTION[1]))
    assert got["tracked"] == [1] * (4 * n_flows)
    return dec, got


def test_the_r32_rule_is_capped():
    """At most four cases may be held to a multiple of the fp32 tensor-op path's error, and they are the ill-conditioned ones."""
    assert len(R32_CASES) == 4 and len(set(R32_CASES)) == 4
    assert all(B < 7 or off != 0 for (_, _, _, B, off) in R32_CASES)
    assert _bar("param", None) == BAR and _bar("param", 1e-6) == BAR and _bar("param", 5e-5) == 8 * 5e-5
    assert _bar("param", 5e-4) == 1e-3 and _bar("param", 3.5e-3) == 8 * 3.5e-3 and _bar("stat", 1e-9) == STAT_BAR
    assert all(BARS[c] < CEILING[c] for c in BARS)
    assert len(STAT_EXCEPTION[1]) == 2 and _bar("stat", 1.6e-6) == CEILING["stat"]       # the exception stays under the ceiling


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_flows,nf,G,B", SHAPES)
def test_module_vs_float64(n_flows, nf, G, B, mode):
    _module_case(n_flows, nf, G, B, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_flows,nf,G,B", HOSTILE_SHAPES)
def test_module_vs_float64_hostile_batchnorm(n_flows, nf, G, B, mode):
    _module_case(n_flows, nf, G, B, mode, R.hostile_bn)


@pytest.mark.parametrize("n_flows,nf,G,B,mode", FLOOR_CASES)
def test_module_vs_float64_floor_active(n_flows, nf, G, B, mode):
    """Inverse mode compounds exp(-lv / 2) ~ 1e3 per floored step: only the two-flow shape is looked at there (at three flows
    max|gs| reaches 1e9 and the case says nothing)."""
    _, got = _module_case(n_flows, nf, G, B, mode, R.floor_active)
    assert float(got["lvs"].min()) < -13


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_flows,nf,G,B", OFFSET_SHAPES)
def test_module_vs_float64_offset_inputs(n_flows, nf, G, B, mode):
    """g + 50: every hidden unit's batch mean is far above its spread."""
    _module_case(n_flows, nf, G, B, mode, None, 50.0)


def test_flat_store_bitwise_on_a_hostile_state():
    nets = _gpu()
    n_flows, nf, G, B, mode = 2, 40, 6, 9, "inverse"
    seed = _seed(G, B)
    ref, got = _module_case(n_flows, nf, G, B, mode, R.hostile_bn)
    flat = _decoder(nets, R.make_state(seed, n_flows, nf, G, R.hostile_bn), n_flows, nf, G)
    store = flat.flatten_parameters()
    assert flat.flat_store() is store and store.attached()
    res = _step(flat, torch.from_numpy(R.inputs(seed, B, G)).cuda().requires_grad_(True), mode, seed, "_GPriorTrainFlat")
    assert store.grad_written
    for name in NAMES + ("dg",):
        assert torch.equal(res[name], got[name]), name
    for k in got["grads"]:
        assert torch.equal(res["grads"][k], got["grads"][k]), k
        assert res["grads"][k].untyped_storage().data_ptr() == store.flat_g.untyped_storage().data_ptr(), k
    for k in got["stats"]:
        assert torch.equal(res["stats"][k], got["stats"][k]), k
    assert res["tracked"] == [1] * (4 * n_flows)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def _guarded(n, fill=float("nan")):
    t = torch.full((n + GUARD,), fill, dtype=torch.float32, device="cuda")
    t[n:] = SENTINEL
    return t


def _intact(t, n):
    return t.numel() == n + GUARD and bool((t[n:] == SENTINEL).all())


def _abi(codes, nf, G, B, mode, params_only, block, g, d):
    """dpf_gprior_train_forward then _backward on NaN-filled buffers, each 64 floats longer with a sentinel behind it; d: three
    (S,B,G) tensors or None.  -> the outputs as tensors of their own sizes, after the buffer checks of (h)."""
    from dpf_nets_amd._lib import lib, check, current_stream
    L = lib()
    S, K, mi = len(codes), G // 2, MODES.index(mode)
    cc = (ctypes.c_int * S)(*codes)
    wsn = L.dpf_gprior_train_workspace_floats(B, G, nf)
    assert wsn == B * (6 * nf + 3 * G)
    sizes = dict(gs=S * B * G, mus=S * B * G, lvs=S * B * G, save_h=S * B * 2 * nf, save_stats=S * 4 * nf, dg=B * G, dcanon=block.numel())
    assert block.numel() == S * 2 * (2 * nf * K + (2 if params_only else 4) * nf + K)
    buf = {k: _guarded(n) for k, n in sizes.items()}
    ws = _guarded(wsn)
    check(L.dpf_gprior_train_forward(S, B, G, nf, mi, cc, params_only, block.data_ptr(), g.data_ptr(), buf["gs"].data_ptr(),
                                     buf["mus"].data_ptr(), buf["lvs"].data_ptr(), buf["save_h"].data_ptr(), buf["save_stats"].data_ptr(),
                                     ws.data_ptr(), R.BN_EPS, GO.EPS, current_stream()), "gprior_train_forward")
    assert _intact(ws, wsn)
    ws[:wsn] = float("nan")
    check(L.dpf_gprior_train_backward(S, B, G, nf, mi, cc, params_only, block.data_ptr(), g.data_ptr(), buf["gs"].data_ptr(),
                                      buf["mus"].data_ptr(), buf["lvs"].data_ptr(), buf["save_h"].data_ptr(), buf["save_stats"].data_ptr(),
                                      *[t.data_ptr() if t is not None else None for t in d], buf["dg"].data_ptr(),
                                      buf["dcanon"].data_ptr(), ws.data_ptr(), R.BN_EPS, GO.EPS, current_stream()), "gprior_train_backward")
    torch.cuda.synchronize()
    assert _intact(ws, wsn)
    out = {}
    for k, n in sizes.items():
        assert _intact(buf[k], n), k
        out[k] = buf[k][:n]
        assert bool(torch.isfinite(out[k]).all()), k
    for k in NAMES:
        out[k] = out[k].view(S, B, G)
    for s, c in enumerate(codes):
        keep = R.code_indices(c, G)[1]
        assert bool((out["mus"][s][:, keep] == 0).all()) and bool((out["lvs"][s][:, keep] == 0).all()), s
    return out


def _abi_inputs(codes, nf, G, B, mutate=None):
    S, seed = len(codes), _seed(G, B)
    state = R.make_state(seed, (S + 1) // 2, nf, G, mutate)
    blocks = [R.canon_block(state, S, G, po) for po in (0, 1)]
    return seed, blocks, R.inputs(seed, B, G), [t.numpy() for t in projection_weights(seed, S, B, G)]


def _abi_compare(case, out, ref, S, nf, G, params_only):
    for name in NAMES:
        _compare(case, "out", name, out[name], ref[name])
    _compare(case, "dg", "dg", out["dg"], ref["dg"])
    blocks, total, stat_slots = R.param_blocks(S, nf, G, params_only)
    assert total == out["dcanon"].numel()
    # A loss on one list alone leaves gradients that are zero in exact arithmetic without being identically zero: batch-statistics
    # BatchNorm removes a shift that is constant over the rows, so the bias of a mu net whose step is only ever read through kept
    # coordinates gets a column sum of d_o that cancels.  Float64 leaves ~1e-16 of the terms' scale there, fp32 ~1e-7, and `rel`
    # would divide one rounding error by the other.  Such a tensor -- the reference below NOISE times the largest gradient of
    # the same tensor in any step of the call -- is measured on that scale instead, at the class's bar.
    kind = {}
    for k, o, shape in blocks:
        tail = k.split(".", 3)[3]
        kind[tail] = max(kind.get(tail, 0.0), float(np.abs(ref["dcanon"][o:o + int(np.prod(shape))]).max()))
    for k, o, shape in blocks:
        n = int(np.prod(shape))
        _compare(case, "param", k, out["dcanon"][o:o + n], ref["dcanon"][o:o + n], kind_scale=kind[k.split(".", 3)[3]])
    for o, n in stat_slots:
        assert bool((out["dcanon"][o:o + n] == 0).all()), (case, "running-statistics slot")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("codes", ABI_CODES, ids=lambda c: "".join(map(str, c)))
@pytest.mark.parametrize("nf,G,B", ABI_SHAPES)
def test_c_abi_arbitrary_step_codes(nf, G, B, codes, mode):
    """Sequences the module never emits: a single step of each code, an odd count with a repeated code."""
    _gpu()
    seed, blocks, g, w = _abi_inputs(codes, nf, G, B)
    ref = R.step64(blocks[0], 0, codes, G, nf, g, mode, w)
    out = _abi(codes, nf, G, B, mode, 0, torch.from_numpy(blocks[0]).cuda(), torch.from_numpy(g).cuda(), [torch.from_numpy(x).cuda() for x in w])
    _abi_compare("abi%s(%d,%d,%d)%s" % ("".join(map(str, codes)), nf, G, B, mode), out, ref, len(codes), nf, G, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nf,G,B", ABI_SHAPES)
def test_c_abi_layouts_reproducibility_and_optional_gradients(nf, G, B, mode):
    """(f) params_only = 0 and 1 on the same numbers are bit-equal in every output and every parameter's gradient slice; (h) a
    second call on the same inputs is bit-equal (no atomics); (g) each gradient table alone against float64 on the loss that
    uses only that list, and none at all gives exact zeros."""
    _gpu()
    codes = [3, 0, 2, 1, 1]
    S = len(codes)
    seed, blocks, g, w = _abi_inputs(codes, nf, G, B, R.hostile_bn)
    tg, tw = torch.from_numpy(g).cuda(), [torch.from_numpy(x).cuda() for x in w]
    tb = [torch.from_numpy(b).cuda() for b in blocks]
    full, again, ponly = _abi(codes, nf, G, B, mode, 0, tb[0], tg, tw), _abi(codes, nf, G, B, mode, 0, tb[0], tg, tw), \
        _abi(codes, nf, G, B, mode, 1, tb[1], tg, tw)
    for k in full:
        assert torch.equal(full[k], again[k]), ("second call", k)
        if k != "dcanon":
            assert torch.equal(full[k], ponly[k]), ("layouts", k)
    b0, _, stat_slots = R.param_blocks(S, nf, G, 0)
    b1, total1, none = R.param_blocks(S, nf, G, 1)
    assert not none and total1 == ponly["dcanon"].numel() and len(stat_slots) == 2 * S
    for (k, o0, shape), (k1, o1, _) in zip(b0, b1):
        n = int(np.prod(shape))
        assert k == k1 and torch.equal(full["dcanon"][o0:o0 + n], ponly["dcanon"][o1:o1 + n]), k
    for o, n in stat_slots:
        assert bool((full["dcanon"][o:o + n] == 0).all())
    case = "abi-opt(%d,%d,%d)%s" % (nf, G, B, mode)
    _abi_compare(case + ":all", ponly, R.step64(blocks[1], 1, codes, G, nf, g, mode, w), S, nf, G, 1)
    for i, name in enumerate(NAMES):
        only = [x if j == i else None for j, x in enumerate(w)]
        out = _abi(codes, nf, G, B, mode, 0, tb[0], tg, [x if j == i else None for j, x in enumerate(tw)])
        _abi_compare(case + ":d_" + name, out, R.step64(blocks[0], 0, codes, G, nf, g, mode, only), S, nf, G, 0)
    for po in (0, 1):
        out = _abi(codes, nf, G, B, mode, po, tb[po], tg, [None, None, None])
        assert bool((out["dg"] == 0).all()) and bool((out["dcanon"] == 0).all())
        assert all(torch.equal(out[k], full[k]) for k in NAMES + ("save_h", "save_stats"))
