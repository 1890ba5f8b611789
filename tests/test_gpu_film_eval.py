"""The eval FiLM conditioner (dpf_flow_film, csrc/flow.hip: film_kernel) through the C ABI, every float of every block against
a float64 NumPy evaluation of the conditioner sub-nets (flows.py:33-45,68-80: Linear(G, 64, no bias) . BatchNorm1d(eval) . Swish
. Linear(64, 64)) plus the fold with BN1 and the output SharedDot that the stack consumes:

    a = eps + exp(cw),  FA = a / sqrt(rv1 + eps_bn),  FC = -a rm1 / sqrt(rv1 + eps_bn) + cb
    block[br] = { D = FC / FA * 2^k,  W2[0] * 2^-k * FA,  W2[1] * 2^-k * FA },  b2[br] = the output SharedDot's bias

(2^k: f16x3's power-of-two scale of the branch's W1, 1 for the bf16 forms).

Cases: L in {1, 14, 63} x B in {1, 4, 8, 9, 32, 64} x G in {128, 512} x {f16x3, bf16x3} x two weight states -- the seeded
synthetic.make_decoder_state one, and the same with negative BatchNorm scales on every third conditioner feature and a dead
(zero-scale) feature in every conditioner BatchNorm.  These cross every sharding of the launch (1, 2 and 4 clouds per
workgroup, one and several workgroups per compute unit); test_film_blocks_other_shardings_and_widths adds ragged groups of two
clouds and the widths that take the kernel's guarded form.

Tolerance.  The figure of merit of a case is  max |got - ref| / max |ref|  over each of the block's three vectors (D, Wa, Wb) of
one branch, all layers and clouds of the case; b2 is a copy and must be equal.  The kernel of commit 922809f (8 clouds per
workgroup, grid (2L, ceil(B/8))) was measured against this very evaluation on these very cases, one MI355X:

    worst figure over the 144 cases of the grid (24 tests): 4.0333e-07   (per test between 3.74e-07 and 4.03e-07)
    worst figure over the further cases (two-cloud ragged groups, G = 48, G = 256): 2.5547e-07

The sharded kernel keeps every output's order of additions (four K-quarters, each one fma chain in ascending k, summed q = 0..3,
in both linears) and the fold's arithmetic, so it is allowed those figures (rounded up in the last printed digit) and no more;
it reaches exactly them, its blocks being byte-equal to that kernel's.

Every float outside the blocks' defined fields -- the tail of each 2 KiB block, and guard regions before the first and after
the last block -- must keep the sentinel it was filled with, ragged B (9) and B = 1 included."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 4.0334e-07          # commit 922809f's kernel on the grid, see the docstring
BOUND_OTHER = 2.5548e-07    # the same on the further cases
F = 64
BN_EPS = float(np.float32(1e-5))
FLOW_EPS = 1e-6
BLOCK = 512                 # floats per (layer, cloud)
GUARD = 1024                # sentinel floats in front of and behind the blocks
SENTINEL = np.uint32(0x7FC0DEAD)
LS, BS = (1, 14, 63), (1, 4, 8, 9, 32, 64)


def _canon(G, hostile):
    """(63, 2, branch floats) canonical fp32 block of a 21-flow decoder (include/dpf_hip.h)."""
    from dpf_nets_amd import synthetic as SY
    from dpf_nets_amd.networks import LocalCondRNVPDecoder
    from dpf_nets_amd.networks.engine import layer_canon_pieces
    dec = LocalCondRNVPDecoder(21, F, G)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in SY.make_decoder_state(17, 21, F, G).items()}, strict=True)
    layers = dec.coupling_layers()
    canon = torch.cat([t.float() for lyr in layers for t in layer_canon_pieces(lyr)]).numpy().copy()
    per_film = 64 * G + 256 + 4096 + 64
    canon = canon.reshape(len(layers), 2, 4740 + 2 * per_film)
    if hostile:
        for sub in range(2):
            gamma = canon[:, :, 4740 + sub * per_film + 64 * G:][:, :, :64]
            gamma[:, :, ::3] *= -1.0
            gamma[:, :, 5 + sub] = 0.0
    return canon


def _meta(L):
    from dpf_nets_amd import synthetic as SY
    rows = []
    for _, warp in SY.decoder_layer_plan(21)[:L]:
        keep = [c for c in (0, 1, 2) if c not in warp]
        rows.append(keep + [-1] * (2 - len(keep)) + list(warp) + [-1] * (2 - len(warp)))
    return rows


def _reference(canon, g, f16):
    """float64: (L, B, 2, 3, 64) block vectors and (L, 2, 2) b2 from the canonical block."""
    L, G = canon.shape[0], g.shape[1]
    per_film = 64 * G + 256 + 4096 + 64
    c = canon.astype(np.float64)
    g = g.astype(np.float64)
    out = np.empty((L, g.shape[0], 2, 3, F))
    b2 = canon[:, :, 4736:4738].copy()
    for l in range(L):
        for br in range(2):
            blk = c[l, br]
            y = []
            for sub in range(2):
                f = blk[4740 + sub * per_film:4740 + (sub + 1) * per_film]
                W0, bn = f[:64 * G].reshape(F, G), f[64 * G:64 * G + 256].reshape(4, F)
                W1, b1 = f[64 * G + 256:64 * G + 256 + 4096].reshape(F, F), f[64 * G + 256 + 4096:]
                u = g @ W0.T
                u = (u - bn[2]) / np.sqrt(bn[3] + BN_EPS) * bn[0] + bn[1]
                h = u / (1.0 + np.exp(-u))
                y.append(h @ W1.T + b1)
            wsc = 1.0
            if f16:
                t = float(np.abs(canon[l, br, 384:4480]).max())
                e = math.frexp(t)[1] - 1
                if t > 0.0 and -100 < e < 100:
                    wsc = 2.0 ** (13 - e)
            s1 = 1.0 / np.sqrt(blk[4544:4608] + BN_EPS)
            t1 = -blk[4480:4544] * s1
            a = float(np.float32(FLOW_EPS)) + np.exp(y[0])
            FA, FC = a * s1, a * t1 + y[1]
            out[l, :, br, 0] = FC / FA * wsc
            out[l, :, br, 1] = blk[4608:4672] / wsc * FA
            out[l, :, br, 2] = blk[4672:4736] / wsc * FA
    return out, b2


def _worst_figure(L, G, precision, hostile, batches):
    from dpf_nets_amd._lib import lib, check, current_stream, PREC
    dev = torch.device("cuda", 0)
    canon = _canon(G, hostile)[:L]
    d_canon = torch.from_numpy(canon.reshape(-1)).to(dev)
    d_meta = torch.tensor(_meta(L), dtype=torch.int32, device=dev)
    packed = torch.empty(lib().dpf_flow_packed_bytes(L, G, PREC[precision]), dtype=torch.uint8, device=dev)
    check(lib().dpf_flow_pack(L, G, PREC[precision], d_canon.data_ptr(), d_meta.data_ptr(), packed.data_ptr(), current_stream()), "flow_pack")
    worst = 0.0
    for B in batches:
        rng = np.random.default_rng(1000 * L + B)
        g = rng.standard_normal((B, G)).astype(np.float32)
        d_g = torch.from_numpy(g).to(dev)
        n = lib().dpf_flow_film_floats(L, B)
        assert n == L * B * BLOCK
        buf = torch.from_numpy(np.full(GUARD + n + GUARD, SENTINEL, dtype=np.uint32).view(np.float32)).to(dev)
        check(lib().dpf_flow_film(L, B, G, PREC[precision], packed.data_ptr(), d_g.data_ptr(), buf.data_ptr() + 4 * GUARD,
                                  FLOW_EPS, current_stream()), "flow_film")
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        bits = raw.view(np.uint32)
        assert (bits[:GUARD] == SENTINEL).all() and (bits[GUARD + n:] == SENTINEL).all(), "wrote outside the blocks (L=%d B=%d)" % (L, B)
        blocks = raw[GUARD:GUARD + n].reshape(L, B, BLOCK)
        assert (blocks[:, :, 388:].view(np.uint32) == SENTINEL).all(), "wrote into a block's undefined tail (L=%d B=%d)" % (L, B)
        ref, b2 = _reference(canon, g, precision == "f16x3")
        got = blocks[:, :, :384].reshape(L, B, 2, 3, F)
        assert np.isfinite(got).all()
        assert np.array_equal(blocks[:, :, 384:388].reshape(L, B, 2, 2), np.broadcast_to(b2[:, None], (L, B, 2, 2)))
        for br in range(2):
            for v in range(3):
                scale = float(np.abs(ref[:, :, br, v]).max())
                if scale == 0.0:                 # a one-channel output SharedDot: the padded second row
                    assert not got[:, :, br, v].any()
                    continue
                worst = max(worst, float(np.abs(got[:, :, br, v] - ref[:, :, br, v]).max()) / scale)
    print("film_eval figure L=%d G=%d %s %s B=%s: %.4e" % (L, G, precision, "hostile" if hostile else "seeded", list(batches), worst))
    return worst


@pytest.mark.parametrize("hostile", [False, True], ids=["seeded", "negative-and-dead-bn"])
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("G", [128, 512])
@pytest.mark.parametrize("L", LS)
def test_film_blocks_against_float64(L, G, precision, hostile):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    worst = _worst_figure(L, G, precision, hostile, BS)
    assert worst <= BOUND, "worst max|got - ref| / max|ref| = %.4e, allowed %.4e" % (worst, BOUND)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("L,G,batches", [(14, 128, (11, 17)), (63, 512, (3,)), (14, 48, (4, 17, 40)), (14, 256, (9, 17, 33))],
                         ids=["two-clouds-ragged", "two-clouds-ragged-512", "G48-guarded", "G256-two-batches"])
def test_film_blocks_other_shardings_and_widths(L, G, batches, precision):
    """Beyond the issue's grid: ragged groups of two clouds per workgroup, and widths that take the guarded form of the kernel
    (G = 48: part of one batch of weights; G = 256: two batches).  Held to the figure that commit 922809f's kernel reaches on them (docstring of the module)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    worst = _worst_figure(L, G, precision, True, batches)
    assert worst <= BOUND_OTHER, "worst max|got - ref| / max|ref| = %.4e, allowed %.4e" % (worst, BOUND_OTHER)
