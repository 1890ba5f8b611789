"""The fused eval stack (csrc/flow.hip, csrc/flow16.hip) on the hostile states and clouds of tests/flow_hostile.py -- negative, zero and
guard-sized BatchNorm scales, running variances far from 1, FiLM factors from 7e-7 to several hundred, dead and constant units, a zero
sd1 row, a saturated softsign and an identity layer -- against FO.decoder in float64, at test_gpu_flow.py's bars, unchanged:
norm-wise REL[prec], elementwise assert_elementwise with ATOL_SCALE[prec].  Forward only: a ReLU that falls the other way leaves every
compared quantity continuous.  tests/test_flow_hostile_cpu.py holds the states' own conditions (finite in float64, inside the f16x3
guard, well-posed for fp32) on every tuple used here.

Every entry meets its bar; none needs test_gpu_flow_frozen.py's OUT_EXCEPTION treatment.  Measured worst error against float64 over all
shapes, modes, clouds and entries: f16x3 1.9e-6 (32-point tiles) and 1.1e-6 (16-point tiles) of REL 4e-6, bf16x6 1.2e-6 of 2e-6, bf16x3
3.0e-5 of 1e-4; the fp32 tensor operations on the CPU, against the same float64, reach 1.2e-6."""
import warnings

import pytest
import torch

from oracle import flow_oracle as FO
from tests import flow_hostile as H
from tests.test_gpu_flow import REL, assert_elementwise, rel, tiling  # noqa: F401  (tiling: fixture)

pytestmark = pytest.mark.gpu

N_FLOWS = 2
SHAPES = [(1, 1, 128), (2, 33, 128), (3, 100, 128), (33, 64, 128), (3, 100, 512)]      # one point, a ragged tile, several tiles, > 32 clouds, G = 512
MODES = ("direct", "inverse")
_DECS = {}


def _decoder(G):
    """The hostile decoder on the GPU, one per G; the packed weights of each precision are made once (FlowStack keeps them)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if G not in _DECS:
        from dpf_nets_amd import networks as nets
        dec = nets.LocalCondRNVPDecoder(N_FLOWS, 64, G)
        dec.load_state_dict(FO.to_torch(H.decoder_state(G, N_FLOWS)), strict=True)
        _DECS[G] = dec.cuda().eval()
    return _DECS[G]


def _forward(dec, prec, src, g, mode):
    """One call at `prec` with warnings as errors; f16x3 must be what was served (a state outside the guard would run at bf16x6)."""
    dec.precision = prec
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            ps, mus, lvs = dec(src, g, mode=mode)
    assert dec.stack().last_precision == prec, (prec, dec.stack().last_precision)
    return ps, mus, lvs


def _check(prec, til, shape, mode, variant, got, ref):
    """Every entry of the three lists and the layer sum against float64; exact zeros where the reference has them by construction."""
    ps, mus, lvs = got
    rps, rmus, rlvs = ref
    plan = FO.decoder_layer_plan(N_FLOWS)
    for k in range(3 * N_FLOWS):
        for name, a, b in (("ps", ps[k], rps[k]), ("mus", mus[k], rmus[k]), ("lvs", lvs[k], rlvs[k])):
            what = (prec, til, shape, mode, variant, name, k)
            r = rel(a, b.numpy())
            print("REL", what, r)
            assert r <= REL[prec], (what, r)
            assert_elementwise(a, b, prec, what)
        keep = [c for c in range(3) if c not in plan[k][1]]
        assert (mus[k][:, keep] == 0).all() and (lvs[k][:, keep] == 0).all(), (k, "keep channels")           # flows.py:96-97
    assert (mus[H.ID_LAYER] == 0).all() and (lvs[H.ID_LAYER] == 0).all(), "identity layer"
    tot = sum(rlvs)
    r = rel(lvs.total(), tot.numpy())
    print("REL", (prec, til, shape, mode, variant, "total"), r)
    assert r <= REL[prec], (prec, til, shape, mode, variant, "total", r)
    assert_elementwise(lvs.total(), tot, prec, (shape, mode, variant, "total"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_N%d_G%d" % s)
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3", "bf16x6"])
def test_hostile_stack_vs_float64(prec, shape, mode, tiling):
    """Per-layer ps, mus, logvars and the layer sum, all three input clouds (as seeded; one cloud a single repeated point; one cloud
    at coordinates of +-8), against float64; then, bit for bit: a second call, and clouds [1:3] alone (a per-point map inside one
    tiling)."""
    if tiling == "tile16" and prec != "f16x3":
        pytest.skip("16-point tiles exist for f16x3 only")
    B, N, G = shape
    dec = _decoder(G)
    for variant in H.VARIANTS:
        _, src, g = H.decoder_case(G, B, N, mode, variant, N_FLOWS)
        tp, tg = torch.from_numpy(src).cuda(), torch.from_numpy(g).cuda()
        got = _forward(dec, prec, tp, tg, mode)
        _check(prec, tiling, shape, mode, variant, got, H.reference64(G, B, N, mode, variant, N_FLOWS))
        first = [x.stacked.clone() for x in got]
        again = _forward(dec, prec, tp, tg, mode)
        assert all(torch.equal(a, b.stacked) for a, b in zip(first, again)), "two calls differ"
        if B >= 3:
            sub = _forward(dec, prec, tp[1:3].contiguous(), tg[1:3].contiguous(), mode)
            assert all(torch.equal(a[:, 1:3], b.stacked) for a, b in zip(first, sub)), "a sub-batch differs"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_N%d_G%d" % s)
def test_hostile_tile16_vs_tile32(shape, mode):
    """The two tilings of the f16x3 kernel add their K slots in a different order: against each other at 2 REL["f16x3"], as
    test_gpu_flow.py holds them."""
    from dpf_nets_amd._lib import lib
    B, N, G = shape
    dec = _decoder(G)
    for variant in H.VARIANTS:
        _, src, g = H.decoder_case(G, B, N, mode, variant, N_FLOWS)
        tp, tg = torch.from_numpy(src).cuda(), torch.from_numpy(g).cuda()
        out = {}
        for t16 in (1, 0):
            old = lib().dpf_flow_set_tile16(t16)
            try:
                before = lib().dpf_flow_tile16_launches()
                out[t16] = [x.stacked.clone() for x in _forward(dec, "f16x3", tp, tg, mode)]
                assert lib().dpf_flow_tile16_launches() == before + t16
            finally:
                lib().dpf_flow_set_tile16(old)
        for name, a, b in zip(("ps", "mus", "lvs"), out[1], out[0]):
            for k in range(3 * N_FLOWS):
                r = rel(a[k], b[k].cpu().numpy())
                assert r <= 2 * REL["f16x3"], (shape, mode, variant, name, k, r)
