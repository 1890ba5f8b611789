"""The host glue the three frozen-statistics paths share (networks/layers.py: EvalAutograd, scatter_param_grads) and the slot
tables of the encoder and of the latent prior flow, without a GPU."""
import pytest
import torch
import torch.nn as nn

from dpf_nets_amd.networks.layers import scatter_param_grads


def test_scatter_param_grads(monkeypatch):
    block = torch.arange(100, 160, dtype=torch.float32)                       # distinct values
    slots = [(0, 6), (6, 1), (7, 12), (27, 20), (47, 4)]                       # unequal sizes, a hole of 8 behind the third
    shapes = [(2, 3), (1,), (3, 4), (4, 5), (4,)]
    params = [torch.zeros(s) for s in shapes]
    copies = []
    orig = torch._foreach_copy_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda *a: (copies.append(len(a[0])), orig(*a))[1])
    expect = [block[o:o + n].clone().view(s) for (o, n), s in zip(slots, shapes)]
    needs = (True, False, True, True, False)
    for like in (params, shapes):
        del copies[:]
        out = scatter_param_grads(block, slots, like, needs)
        assert copies == [3]                                                   # one multi-tensor copy
        assert [t is None for t in out] == [not n for n in needs]
        keep = block.clone()
        block.fill_(-1.0)                                                      # a view of the block would follow
        for t, e, s, need in zip(out, expect, shapes, needs):
            if need:
                assert tuple(t.shape) == s and t.dtype == torch.float32 and torch.equal(t, e)
                assert t.untyped_storage().data_ptr() != block.untyped_storage().data_ptr()
        block.copy_(keep)
    del copies[:]
    assert scatter_param_grads(None, slots, shapes, (False,) * 5) == [None] * 5 and copies == []     # the block is not touched:
    assert scatter_param_grads(None, slots, params, (False,) * 5) == [None] * 5 and copies == []     # nothing is allocated
    out = scatter_param_grads(block, slots, params)                            # needs = None: all of them
    assert copies == [5] and all(torch.equal(t, e) for t, e in zip(out, expect))
    views = [block[o:o + n] for o, n in slots]                                 # the list-of-views form of the point flow's nodes
    out = scatter_param_grads(views, None, params, needs)
    assert [t is None for t in out] == [not n for n in needs]
    assert all(torch.equal(t, e) and t.untyped_storage().data_ptr() != block.untyped_storage().data_ptr()
               for t, e, need in zip(out, expect, needs) if need)


def test_encoder_slot_table():
    from dpf_nets_amd.networks import PointNetCloudEncoder
    from dpf_nets_amd.networks.encoder_frozen_engine import frozen_slots, frozen_params
    enc = PointNetCloudEncoder(3, 64, [128, 256, 512])
    slots = frozen_slots(enc)
    assert slots == [(0, 192), (192, 64), (256, 64),
                     (448, 8192), (8640, 128), (8768, 128),
                     (9152, 32768), (41920, 256), (42176, 256),
                     (42944, 131072), (174016, 512), (174528, 512)]
    assert slots[-1][0] + slots[-1][1] + 2 * 512 == 176064                     # E_CANON
    assert [n for _, n in slots] == [t.numel() for t in frozen_params(enc)]
    assert frozen_slots(enc) is slots                                          # once per module


def test_prior_net_walk():
    from dpf_nets_amd.networks.prior_flows import RealNVPFlowCouple, _net_walk
    G, nf = 8, 4
    steps = RealNVPFlowCouple(nf, G).layers()
    nets = [getattr(l, "T_%s_0" % br) for l in steps for br in ("mu", "logvar")]
    want_params = [t for n in nets for t in (n[0].weight, n[1].weight, n[1].bias, n[3].weight, n[3].bias)]
    params, slots, bns, total = _net_walk(steps, True)                         # dpf_gprior_pack's layout: 52 floats a net
    assert slots == [(52 * n + o, k) for n in range(4) for o, k in ((0, 16), (16, 4), (20, 4), (32, 16), (48, 4))]
    assert total == 208 and all(a is b for a, b in zip(params, want_params)) and len(params) == 20
    assert all(a is n[1] for a, n in zip(bns, nets)) and len(bns) == 4
    params, slots, bns, total = _net_walk(steps, False)                        # the parameters-only layout: 44 floats a net
    assert slots == [(44 * n + o, k) for n in range(4) for o, k in ((0, 16), (16, 4), (20, 4), (24, 16), (40, 4))]
    assert total == 176 and all(a is b for a, b in zip(params, want_params)) and len(params) == 20


def test_eval_autograd_on_the_encoder():
    from dpf_nets_amd.networks import PointNetCloudEncoder, GlobalRNVPDecoder
    enc = PointNetCloudEncoder(3, 64, [128, 256, 512])
    assert enc.eval_autograd == "torch"
    enc.eval_autograd = "hip"
    assert enc.eval_autograd == "hip"
    with pytest.raises(ValueError, match=r"eval_autograd must be one of \['torch', 'hip'\], got 'triton'"):
        enc.eval_autograd = "triton"
    assert enc.eval_autograd == "hip" and not any("eval_autograd" in k for k in enc.state_dict())

    class Model(nn.Module):                                                    # as networks/models.py holds its encoder and decoders
        def __init__(self):
            super().__init__()
            self.pc_encoder = PointNetCloudEncoder(3, 64, [128, 256, 512])
            self.g_prior = GlobalRNVPDecoder(1, 4, 8)

    m = Model()
    m.eval_autograd = "hip"                                                    # a plain attribute of a plain module: reaches nobody
    assert m.pc_encoder.eval_autograd == "torch" and m.g_prior.eval_autograd == "torch"
    m.g_prior.eval_autograd = "hip"                                            # a container with the mixin hands it down
    assert all(s.eval_autograd == "hip" for s in m.g_prior.coupling_layers()) and m.pc_encoder.eval_autograd == "torch"
    m.pc_encoder.eval_autograd = "hip"
    assert m.pc_encoder.eval_autograd == "hip"
