"""tests/frozen_composed_ref.py without a GPU: its float64 graph over the forward_torch paths, with the decisions its own, equals plain
float64 autograd of the model's own calls -- encode(), g_prior(g, "inverse"), networks.GaussianFlowNLL, _base(),
pc_decoder.sample_and_decode() and a Chamfer distance written with min() -- in the loss and in every gradient; handing its own
decisions back in changes nothing, the encoder's ReLU decisions included, and a ReLU decision that is no near-tie is counted, not
taken; with g_free the latent is the only input."""
import warnings

import torch

from dpf_nets_amd import networks as nets
from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
from tests import frozen_composed_ref as C

SHAPE = (2, 37, 29, 23)
TOL = 1e-11            # two float64 formulations of one graph: rounding only


def _plain(model, x, noise, target, g_free=None):
    """-> loss, g; the modules' own forward() calls, which on CPU tensors are tensor operations (loud for the flows: ignored here)"""
    B, S = noise.shape[0], noise.shape[2]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", EvalModeAutogradWarning)
        g = model.encode(x)["g_posterior_mus"] if g_free is None else g_free
        gs, mus, lvs = model.g_prior(g, mode="inverse")
        gnll = nets.GaussianFlowNLL()(list(gs) + [g], [model.g0_prior_mus.expand(B, C.G)] + list(mus),
                                      [model.g0_prior_logvars.expand(B, C.G)] + list(lvs))
        mu0, lv0 = model._base(g, B, S)
        pred = model.pc_decoder.sample_and_decode(mu0[0], lv0[0], g, noise=noise)[1][-1].transpose(1, 2)
    d = ((pred[:, :, None, :] - target[:, None, :, :]) ** 2).sum(-1)
    return (d.min(dim=2)[0].mean(1) + d.min(dim=1)[0].mean(1)).sum() + gnll, g


def _close(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert C.rel(a, b) <= TOL, (what, C.rel(a, b))


def test_the_float64_graph_is_plain_autograd_of_the_model():
    x, noise, target = (t.double() for t in C.inputs(C.SEED, SHAPE))
    model = C.build_model(nets, dtype=torch.float64)
    xin = x.clone().requires_grad_(True)               # (a differentiable cloud: the eval-mode encoder has no other CPU path)
    loss, g = _plain(model, xin, noise, target)
    loss.backward()
    plain, plain_dx = C.grads_of(model), xin.grad
    assert sum(v is not None for v in plain.values()) == len(plain) - 2        # encode() leaves the posterior's logvar head unused
    assert plain["g_posterior.logvars.logvar_mlp0.weight"] is None and plain["g0_prior_mus"] is not None
    model.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True)
    own = C.composed_loss(model, xin, noise, target)
    own["loss"].backward()
    assert abs(own["loss"].item() - loss.item()) <= TOL * abs(loss.item())
    _close(own["g"], g, "g")
    _close(xin.grad, plain_dx, "dx")
    first = C.grads_of(model)
    for k in plain:
        _close(first[k], plain[k], k)
    # its own decisions handed back in: the same bits
    model.zero_grad(set_to_none=True)
    again = C.composed_loss(model, x, noise, target, arg=own["arg"], idx1=own["idx1"], idx2=own["idx2"])
    again["loss"].backward()
    assert torch.equal(again["loss"], own["loss"])
    second = C.grads_of(model)
    assert all((first[k] is None and second[k] is None) or torch.equal(first[k], second[k]) for k in first)
    # ... and so with its own ReLU decisions at the argmax points; a decision away from a tie is reported and NOT taken
    relu, h = [], x
    for name, mod in model.pc_encoder.features.named_children():
        if name in C.RELU_SEGMENTS:
            relu.append(torch.gather(h, 2, own["arg"][:, None, :].expand(-1, h.shape[1], -1)).permute(0, 2, 1) > 0)
        h = mod(h)
    relu = torch.cat(relu, dim=2)
    assert tuple(relu.shape) == (SHAPE[0], 512, 448)
    for flip in (False, True):
        model.zero_grad(set_to_none=True)
        if flip:
            relu[1, 7, 300] = ~relu[1, 7, 300]
        third = C.composed_loss(model, x, noise, target, arg=own["arg"], idx1=own["idx1"], idx2=own["idx2"], relu=relu)
        third["loss"].backward()
        assert third["relu_taken"] == 0 and third["relu_far"] == int(flip)
        assert torch.equal(third["loss"], own["loss"])
        grads = C.grads_of(model)
        assert all((first[k] is None and grads[k] is None) or torch.equal(first[k], grads[k]) for k in first)
    # other decisions are taken, not ignored
    moved = C.composed_loss(model, x, noise, target, arg=(own["arg"] + 1) % SHAPE[1], idx1=(own["idx1"] + 1) % SHAPE[3], idx2=own["idx2"])
    assert moved["cd"].sum().item() > own["cd"].sum().item() and not torch.equal(moved["g"], own["g"])


def test_the_latent_as_the_only_input():
    x, noise, target = (t.double() for t in C.inputs(C.SEED, SHAPE))
    model = C.build_model(nets, dtype=torch.float64)
    for p in model.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        g0 = C.composed_loss(model, x, noise, target)["g"]
    ga, gb = g0.clone().requires_grad_(True), g0.clone().requires_grad_(True)
    loss, _ = _plain(model, None, noise, target, g_free=ga)
    loss.backward()
    own = C.composed_loss(model, None, noise, target, g_free=gb)
    own["loss"].backward()
    assert own["pooled"] is None and abs(own["loss"].item() - loss.item()) <= TOL * abs(loss.item())
    _close(gb.grad, ga.grad, "dg")
    assert all(p.grad is None for p in model.parameters())


def test_shapes_and_inputs():
    assert C.CFG["pc_enc_n_features"] == [128, 256, 512] and C.CFG["g_prior_n_flows"] == 2 and C.CFG["p_decoder_n_flows"] == 2
    assert C.SHAPE_BATCHED_FILM[0] > 64 and C.SHAPE_BATCHED_FILM[2] == C.SHAPE_BATCHED_FILM[3] and C.SHAPE_RAGGED[1] > 256
    a, b = C.inputs(C.SEED, C.SHAPE_TINY), C.inputs(C.SEED, C.SHAPE_TINY, batch=1)
    assert [tuple(t.shape) for t in a] == [(1, 3, 33), (1, 3, 40), (1, 31, 3)]
    assert all(not torch.equal(s, t) for s, t in zip(a, b))
