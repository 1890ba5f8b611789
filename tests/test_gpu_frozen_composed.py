"""The frozen-statistics autograd path COMPOSED across the whole autoencoder: Local_Cond_RNVP_MC_Global_RNVP_VAE in eval() with
eval_autograd = "hip" on pc_encoder, g_prior and pc_decoder (default precisions), differentiated through the latent-optimisation /
fine-tuning graph of tests/frozen_composed_ref.py

    g = encode(x).g_posterior_mus;  gnll = GaussianFlowNLL over g_prior(g, "inverse");  pred = pc_decoder.sample_and_decode(.., g, noise)
    loss = chamfer_loss(pred^T, target).sum() + gnll

so that the seams between the four nodes are exercised: one g feeding the prior's node AND the decoder's node, their two dg summed
into the posterior head and the encoder's node; the decoder stack's gradient accumulation (FlatStore.accumulate, the fused FiLM
backward's add-into-flat_g flag); the state the nodes share on the host (the FiLM ticket word, the process-wide ChamferEvaluator
workspace, grad_written, the per-call weight refresh); and run-to-run bit identity of the whole graph.

Reference: the same modules in double() through forward_torch with the discrete decisions of the HIP run -- pooled gathered at the
kernel's own argmax, the Chamfer distances formed at the indices the HIP forward returned, the encoder's ReLUs at a near-tie as the
kernel decided them (below) (tests/test_frozen_composed_cpu.py checks that graph against plain autograd).

Shapes (B, N_in, S, M), each the smallest that reaches its path:
  (3, 300, 200, 257)  two encoder workgroups per cloud with a ragged last tile, a ragged decoded cloud, unequal Chamfer sides;
  (1, 33, 40, 31)     one cloud, less than one tile on every side (B = 1 is legal for every frozen node);
  (65, 33, 64, 64)    past dpf_film_train_max_batch() = 64: the FiLM nets' batched tensor-op branch of _forward_core / _backward_core;
                      S == M, which a swap of Chamfer's two gradients needs to get past autograd's shape check.
A latent size that is no multiple of 4 is left out: the decoder's fused forward, which IS the frozen node's forward, takes G % 16 == 0
only (csrc/flow.hip), and the prior flow an even G.

Bars, every tensor relative to its largest magnitude, each parameter at the bar of its own node's test:
  pc_encoder.*   TOL_GRAD = 5e-4 (tests/encoder_frozen_ref.py);      g, loss, and pred downstream of it: TOL_OUT = 1e-4
  g_prior.*      PGRAD = 1e-3, g0_prior_* and d/dg TOL = 1e-4 (tests/test_gpu_gprior_frozen.py)
  pc_decoder.*   GRAD = 2e-4 with bias_floor; pred from a given latent OUT = 4e-6 (tests/test_gpu_flow_frozen.py)
  g_posterior.*  GRAD + TOL_OUT = 3e-4: d W = dg^T pooled, the decoder's dg at its bar times the encoder's pooled at its bar
  d loss / d g as the only leaf: GRAD (the looser of the two nodes whose dg it sums)
every one in the form test_gpu_flow_frozen._compare uses, max(node bar, R32_FACTOR["f16x3"] = 5 x the error of the fp32 tensor-op
path of the same model against float64 on the same inputs and decisions); both errors are printed.

Measured worst errors against float64 over the three shapes and the two-batch run, HIP path (fp32 tensor-op yardstick in brackets):
loss 5.6e-8 (5.6e-8), g 1.7e-6 (6.8e-7), pred 2.6e-7 (2.6e-7); with the latent as the leaf pred 2.6e-7 (2.5e-7), dg 2.4e-7 (2.5e-7);
parameter gradients: pc_decoder 9.3e-6 at (1, 33, 40, 31), g_prior 2.7e-6, g0_prior_mus 1.4e-6, g0_prior_logvars 2.7e-7,
g_posterior 1.1e-6, pc_encoder 3.2e-6 at (1, 33, 40, 31) (the yardstick is at 1e-7-class everywhere, so no
bar is ever raised above its node's).

The encoder's ReLUs are a third discrete decision.  At (65, 33, 64, 64) unit 190 of sd1 at point 12 of cloud 10 has a float64
pre-activation of 4.5e-7 of its layer's largest magnitude, below the bf16x3 forward's 1e-5-class error, and the kernel puts it on
the other side of zero; that point is the argmax of 11 features, and with float64's own decision sd1.weight is at 5.23e-4 and
sd1_bn.bias at 5.33e-4 of float64 (TOL_GRAD = 5e-4), the whole error in row 190.  The backward recomputes every ReLU of the argmax
points with the forward's own arithmetic and leaves the activations in its workspace (csrc/encoder_frozen.hip), so _kernel_relu reads
the kernel's decisions there and the reference takes them over -- ONLY where its own pre-activation is within TIE_TOL = TOL_OUT = 1e-4
of zero relative to its layer (tests/encoder_frozen_ref.near_zero_points' rule); any other disagreement fails the test (relu_far == 0
is asserted on the float64 graph).  Measured: 11 decisions taken at (65, 33, 64, 64), none at the other shapes, no disagreement away
from a tie anywhere; the encoder's gradients of that case are then within 2.1e-6.
"""
import warnings

import pytest
import torch

from tests import encoder_frozen_ref as ER
from tests import frozen_composed_ref as C
from tests.test_gpu_flow_frozen import OUT, GRAD
from tests.test_gpu_flow_train import R32_FACTOR, bias_floor
from tests.test_gpu_gprior_frozen import TOL as PRIOR_TOL, PGRAD as PRIOR_PGRAD

pytestmark = pytest.mark.gpu

FACTOR = R32_FACTOR["f16x3"]
HEAD = GRAD + ER.TOL_OUT
FLAT = [False, True]
ACC_SHAPE = C.SHAPE_RAGGED


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def _param_bar(name):
    for prefix, bar in (("pc_encoder.", ER.TOL_GRAD), ("g_prior.", PRIOR_PGRAD), ("pc_decoder.", GRAD), ("g0_prior_", PRIOR_TOL),
                        ("g_posterior.", HEAD)):
        if name.startswith(prefix):
            return bar
    raise KeyError(name)


def _model(nets, flat, frozen=False):
    """-> the seeded model on the GPU with the three HIP nodes asked for, [decoder store, prior store] or None"""
    model = C.build_model(nets, device="cuda")
    for m in (model.pc_encoder, model.g_prior, model.pc_decoder):
        m.eval_autograd = "hip"
    stores = model.flatten_parameters() if flat else None
    if frozen:
        for p in model.parameters():
            p.requires_grad_(False)
    return model, stores


def _nodes(root):
    """{class name: node} of the autograd graph under `root`"""
    seen, todo, names = set(), [root], {}
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.setdefault(type(fn).__name__, fn)
        todo += [f for f, _ in fn.next_functions]
    return names


def _kernel_relu(pool):
    """(B,512,448) bool: the hidden units of layers 0-2 that are live at every argmax point, as dpf_encoder_frozen_backward recomputes
    them from what the node saved (the first block of its workspace: a0 | a1 | a2 per virtual point, csrc/encoder_frozen.hip)"""
    from dpf_nets_amd._lib import lib, check, current_stream
    x, canon, packed, pooled, arg = pool.saved_tensors
    B, _, N = x.shape
    L_ = lib()
    ws = torch.zeros(L_.dpf_encoder_frozen_workspace_bytes(B), dtype=torch.uint8, device=x.device)
    dcanon, ones = torch.empty_like(canon), torch.ones_like(pooled)
    check(L_.dpf_encoder_frozen_backward(B, N, pool.prec, canon.data_ptr(), packed.data_ptr(), x.data_ptr(), pooled.data_ptr(), arg.data_ptr(),
                                         ones.data_ptr(), dcanon.data_ptr(), None, ws.data_ptr(), current_stream()), "encoder_frozen_backward")
    torch.cuda.synchronize()
    return ws[:B * 512 * 448 * 4].view(torch.float32).view(B, 512, 448) > 0


def _forward(nets, model, x, noise, target, g_free=None, flat_nodes=False):
    """The composed forward on the HIP nodes, and proof that it was them: an EvalModeAutogradWarning is an error, the decoder served
    f16x3, pooled's grad_fn is the encoder's frozen node, and the prior's, the decoder's and Chamfer's nodes are in the graph.
    -> dict: loss, g, pred, and the decisions a reference takes over: arg, relu (_kernel_relu), idx1, idx2"""
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    from dpf_nets_amd.networks.utils import chamfer_loss
    model.pc_decoder.stack().last_precision = None
    with warnings.catch_warnings():
        warnings.simplefilter("error", EvalModeAutogradWarning)
        g = model.encode(x)["g_posterior_mus"] if g_free is None else g_free
        B, S = g.shape[0], noise.shape[2]
        gs, mus, lvs = model.g_prior(g, mode="inverse")
        gnll = nets.GaussianFlowNLL()(gs + [g], [model.g0_prior_mus.expand(B, C.G)] + mus, [model.g0_prior_logvars.expand(B, C.G)] + lvs)
        mu0, lv0 = model._base(g, B, S)
        ps = model.pc_decoder.sample_and_decode(mu0[0], lv0[0], g, noise=noise)[1]
        pred = ps[-1].transpose(1, 2).contiguous()
        cd = chamfer_loss(pred, target)
    loss = cd.sum() + gnll
    assert model.pc_decoder.stack().last_precision == "f16x3"
    nodes = _nodes(loss.grad_fn)
    suffix = "FlatBackward" if flat_nodes else "Backward"
    assert "_FlowStackFrozen" + suffix in nodes and "_GPriorFrozen" + suffix in nodes and "ChamferLossFunctionBackward" in nodes, sorted(nodes)
    arg = relu = None
    if g_free is None:
        pool = [f for f, _ in g.grad_fn.next_functions if type(f).__name__ == "_FrozenPoolBackward"]
        assert len(pool) == 1, [type(f).__name__ for f, _ in g.grad_fn.next_functions]       # the posterior head's input IS the node's output
        arg = pool[0].saved_tensors[4].clone()
        assert arg.dtype == torch.int32 and tuple(arg.shape) == (B, 512)
        relu = _kernel_relu(pool[0])
    else:
        assert "_FrozenPoolBackward" not in nodes
    return dict(loss=loss, g=g, pred=pred, arg=arg, relu=relu, idx1=cd.grad_fn.idx1, idx2=cd.grad_fn.idx2, nodes=sorted(nodes))


def _data(shape, batch=0):
    return tuple(t.cuda() for t in C.inputs(C.SEED, shape, batch))


_HIP = {}


def _latent(nets, shape, batch=0):
    return _hip(nets, shape, False, batch=batch)["g"]


def _hip(nets, shape, flat, frozen=False, batch=0, fresh=False):
    """One forward + backward of the HIP graph on a model of its own; computed once per case and shared unless `fresh`.
    frozen: every parameter frozen, the leaf is the latent of the unfrozen run as a free tensor."""
    key = (shape, flat, frozen, batch)
    if not fresh and key in _HIP:
        return _HIP[key]
    model, stores = _model(nets, flat, frozen)
    g_free = _latent(nets, shape, batch).clone().requires_grad_(True) if frozen else None
    f = _forward(nets, model, *_data(shape, batch), g_free=g_free, flat_nodes=flat and not frozen)
    f["loss"].backward()
    res = dict(loss=f["loss"].detach(), g=f["g"].detach(), pred=f["pred"].detach(), arg=f["arg"], relu=f["relu"], idx1=f["idx1"], idx2=f["idx2"],
               nodes=f["nodes"], grads=C.grads_of(model), dg=g_free.grad if frozen else None,
               flat_g=[s.flat_g.clone() for s in stores] if flat else None, written=[s.grad_written for s in stores] if flat else None)
    if not fresh:
        _HIP[key] = res
    return res


_REF = {}


def _reference(nets, dtype, shape, frozen, batches, decisions):
    """forward_torch of the same model in `dtype` on the same inputs with the HIP run's decisions, the losses of `batches` summed,
    one backward.  Computed once per case and shared: every HIP run of a case takes the same decisions (asserted by the callers)."""
    key = (dtype, shape, frozen, batches)
    if key not in _REF:
        model = C.build_model(nets, dtype=dtype, device="cuda")
        if frozen:
            for p in model.parameters():
                p.requires_grad_(False)
        loss, outs, leaves = 0.0, [], []
        for batch, d in zip(batches, decisions):
            g_free = _latent(nets, shape, batch).to(dtype).clone().requires_grad_(True) if frozen else None
            out = C.composed_loss(model, *_data(shape, batch), arg=d["arg"], idx1=d["idx1"], idx2=d["idx2"], g_free=g_free, relu=d["relu"])
            print("RELU %s %s batch %d: %d near-tie decisions taken from the kernel, %d disagreements elsewhere"
                  % (shape, dtype, batch, out["relu_taken"], out["relu_far"]))
            if dtype == torch.float64:
                assert out["relu_far"] == 0, out["relu_far"]     # away from a tie the kernel's ReLUs are float64's
            loss = loss + out["loss"]
            outs.append(out)
            leaves.append(g_free)
        loss.backward()
        _REF[key] = dict(loss=loss.detach(), g=outs[0]["g"].detach(), pred=outs[0]["pred"].detach(), grads=C.grads_of(model),
                         dg=leaves[0].grad if frozen else None, decisions=decisions)
    ref = _REF[key]
    for d, e in zip(decisions, ref["decisions"]):
        assert all((d[k] is None and e[k] is None) or torch.equal(d[k], e[k]) for k in ("arg", "relu", "idx1", "idx2")), "the decisions moved"
    return ref


def _check_tensor(failures, what, name, got, r64, r32, node_bar, floor=0.0):
    e, e32 = C.rel(got, r64, floor), C.rel(r32, r64, floor)
    bar = max(node_bar, FACTOR * e32)
    print("REL %s %-70s hip %.2e fp32 %.2e bar %.2e" % (what, name, e, e32, bar))
    if not e <= bar:
        failures.append((name, e, e32, bar))
    return e


def _check_grads(what, got, r64, r32):
    """Every parameter gradient at max(its node's bar, FACTOR x the fp32 tensor-op path's error); -> the worst error per family"""
    failures, worst = [], {}
    assert set(got) == set(r64["grads"])
    for k, ref in r64["grads"].items():
        if ref is None:
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k
            continue
        assert got[k] is not None and bool(torch.isfinite(got[k]).all()), k
        if float(ref.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, k
            continue
        floor = bias_floor(r64["grads"], k) if k.startswith("pc_decoder.") else 0.0
        e = _check_tensor(failures, what, k, got[k], ref, r32["grads"][k], _param_bar(k), floor)
        fam = k.split(".")[0]
        worst[fam] = max(worst.get(fam, 0.0), e)
    print("WORST", what, " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert not failures, failures
    return worst


@pytest.mark.parametrize("flat", FLAT)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_values_and_every_gradient_vs_float64(shape, flat):
    """1, every parameter a leaf (encoder, posterior head, prior flow, decoder, g0_prior_*), per tensor and over the two flat stores."""
    nets = _gpu()
    h = _hip(nets, shape, flat)
    dec = [dict(arg=h["arg"], relu=h["relu"], idx1=h["idx1"], idx2=h["idx2"])]
    r64, r32 = (_reference(nets, dt, shape, False, (0,), dec) for dt in (torch.float64, torch.float32))
    what = "%s %s" % (shape, "flat" if flat else "per-tensor")
    failures = []
    _check_tensor(failures, what, "loss", h["loss"], r64["loss"], r32["loss"], ER.TOL_OUT)
    _check_tensor(failures, what, "g", h["g"], r64["g"], r32["g"], ER.TOL_OUT)
    _check_tensor(failures, what, "pred", h["pred"], r64["pred"], r32["pred"], ER.TOL_OUT)
    assert not failures, failures
    _check_grads(what, h["grads"], r64, r32)
    if flat:
        assert all(h["written"]) and all(float(fg.abs().max()) > 0 for fg in h["flat_g"])
        per = _hip(nets, shape, False)
        assert torch.equal(h["loss"], per["loss"])
        for k, v in per["grads"].items():
            assert (v is None and h["grads"][k] is None) or torch.equal(v, h["grads"][k]), k


@pytest.mark.parametrize("flat", FLAT)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_latent_as_the_only_leaf_vs_float64(shape, flat):
    """1, second configuration: every parameter frozen, the posterior mean of the first configuration a free tensor.  No encoder
    in front: pred at the decoder's own OUT, d loss / d g at GRAD."""
    nets = _gpu()
    h = _hip(nets, shape, flat, frozen=True)
    dec = [dict(arg=None, relu=None, idx1=h["idx1"], idx2=h["idx2"])]
    r64, r32 = (_reference(nets, dt, shape, True, (0,), dec) for dt in (torch.float64, torch.float32))
    what = "%s %s frozen" % (shape, "flat" if flat else "per-tensor")
    failures = []
    _check_tensor(failures, what, "loss", h["loss"], r64["loss"], r32["loss"], OUT)
    _check_tensor(failures, what, "pred", h["pred"], r64["pred"], r32["pred"], OUT)
    _check_tensor(failures, what, "dg", h["dg"], r64["dg"], r32["dg"], GRAD)
    assert not failures, failures
    assert torch.equal(h["dg"], _hip(nets, shape, False, frozen=True)["dg"])


def _store_views_attached(stores):
    return all(s.attached() and s.grads_attached(full=True) for s in stores)


@pytest.mark.parametrize("flat", FLAT)
def test_second_backward_doubles_every_gradient(flat):
    """2: backward(retain_graph=True) twice without clearing gives exactly twice the single-backward gradient, bit for bit (x + x
    is exact), in every parameter and every block of both flat stores; the single backward has the bits of a run of its own."""
    nets = _gpu()
    model, stores = _model(nets, flat)
    f = _forward(nets, model, *_data(ACC_SHAPE), flat_nodes=flat)
    f["loss"].backward(retain_graph=True)
    first = C.grads_of(model)
    first_flat = [s.flat_g.clone() for s in stores] if flat else []
    f["loss"].backward()
    single = _hip(nets, ACC_SHAPE, flat)
    for k, p in model.named_parameters():
        if first[k] is None:
            assert p.grad is None and single["grads"][k] is None, k
            continue
        assert torch.equal(first[k], single["grads"][k]), k
        assert float(first[k].abs().max()) > 0 and torch.equal(p.grad, 2 * first[k]), k
    for s, one in zip(stores or [], first_flat):
        assert s.grad_written and torch.equal(s.flat_g, 2 * one)


@pytest.mark.parametrize("flat", FLAT)
def test_two_batches_one_backward(flat):
    """2: two forward calls of one model on two different batches, the losses summed, one backward.  Every gradient against float64
    of the two-batch loss at the bars of test 1, and against the sum of the two single-batch HIP runs BIT FOR BIT: every addend is
    formed before it is added -- AccumulateGrad and FlatStore.accumulate / PriorFlatStore.accumulate add finished tensors, and the
    fused FiLM backward (csrc/film_train.hip: put, tile_store) finishes an entry's sum over the clouds in registers / LDS before the
    one read-add-write into flat_g.  No block has partial sums added straight into the buffer, so none is held to the float64 bar only."""
    nets = _gpu()
    model, stores = _model(nets, flat)
    fa = _forward(nets, model, *_data(ACC_SHAPE, 0), flat_nodes=flat)
    fb = _forward(nets, model, *_data(ACC_SHAPE, 1), flat_nodes=flat)
    assert not torch.equal(fa["g"], fb["g"])
    (fa["loss"] + fb["loss"]).backward()
    got = C.grads_of(model)
    a, b = _hip(nets, ACC_SHAPE, flat, batch=0), _hip(nets, ACC_SHAPE, flat, batch=1)
    assert torch.equal(fa["loss"].detach(), a["loss"]) and torch.equal(fb["loss"].detach(), b["loss"])
    for k, v in got.items():
        if v is None:
            assert a["grads"][k] is None and b["grads"][k] is None, k
            continue
        assert torch.equal(v, a["grads"][k] + b["grads"][k]), (k, C.rel(v, a["grads"][k] + b["grads"][k]))
    for i, s in enumerate(stores or []):
        assert s.grad_written and torch.equal(s.flat_g, a["flat_g"][i] + b["flat_g"][i])
    dec = [dict(arg=f["arg"], relu=f["relu"], idx1=f["idx1"], idx2=f["idx2"]) for f in (fa, fb)]
    r64, r32 = (_reference(nets, dt, ACC_SHAPE, False, (0, 1), dec) for dt in (torch.float64, torch.float32))
    _check_grads("two batches %s" % ("flat" if flat else "per-tensor"), got, r64, r32)


@pytest.mark.parametrize("flat", FLAT)
def test_backward_after_zero_grad_repeats_the_bits(flat):
    """2: after networks.Adam.zero_grad() (the flat path for the two stores: one fill, the views stay) a new forward + backward gives
    the first one's bits"""
    nets = _gpu()
    model, stores = _model(nets, flat)
    opt = nets.Adam(model.parameters(), lr=1e-3)
    _forward(nets, model, *_data(ACC_SHAPE), flat_nodes=flat)["loss"].backward()
    first = C.grads_of(model)
    opt.zero_grad()
    if flat:
        assert _store_views_attached(stores) and not any(s.grad_written for s in stores)
        assert all(float(s.flat_g.abs().max()) == 0.0 for s in stores)
    in_store = set(id(p) for s in stores or [] for p in s.params)
    assert all(p.grad is None for p in model.parameters() if id(p) not in in_store)
    _forward(nets, model, *_data(ACC_SHAPE), flat_nodes=flat)["loss"].backward()
    for k, v in C.grads_of(model).items():
        assert (v is None and first[k] is None) or torch.equal(v, first[k]), k
    single = _hip(nets, ACC_SHAPE, flat)
    assert all(first[k] is None or torch.equal(first[k], single["grads"][k]) for k in first)
    if flat:
        assert all(s.grad_written for s in stores) and _store_views_attached(stores)


def _pattern(n, device):
    return ((torch.arange(n, device=device) % 7).to(torch.float32) - 3.0) * 0.125


@pytest.mark.parametrize("flat", FLAT)
def test_a_gradient_already_there_is_added_to(flat):
    """2: a non-zero gradient before the backward -- flat_g of both stores, .grad of every other parameter -- is preserved and added
    to, bit for bit: nothing overwrites"""
    nets = _gpu()
    model, stores = _model(nets, flat)
    in_store = set(id(p) for s in stores or [] for p in s.params)
    for s in stores or []:
        s.flat_g.copy_(_pattern(s.flat_g.numel(), "cuda"))
    before = {}
    for k, p in model.named_parameters():
        if id(p) not in in_store:
            p.grad = _pattern(p.numel(), "cuda").view(p.shape).clone()
        before[k] = p.grad.clone()
    _forward(nets, model, *_data(ACC_SHAPE), flat_nodes=flat)["loss"].backward()
    single = _hip(nets, ACC_SHAPE, flat)
    for k, p in model.named_parameters():
        want = before[k] if single["grads"][k] is None else before[k] + single["grads"][k]
        assert torch.equal(p.grad, want), k
    for i, s in enumerate(stores or []):
        assert s.grad_written and torch.equal(s.flat_g, _pattern(s.flat_g.numel(), "cuda") + single["flat_g"][i])


@pytest.mark.parametrize("flat", FLAT)
def test_frozen_parameters_form_no_gradient(flat):
    """2: every parameter frozen, g the only leaf: no parameter gradient is formed, flat_g of both stores is untouched and grad_written
    stays false, every BatchNorm buffer and num_batches_tracked is unchanged"""
    nets = _gpu()
    model, stores = _model(nets, flat, frozen=True)
    for s in stores or []:
        s.flat_g.copy_(_pattern(s.flat_g.numel(), "cuda"))
        assert not s.grad_written
    buffers = {k: v.clone() for k, v in model.named_buffers()}
    assert sum("num_batches_tracked" in k for k in buffers) > 50
    in_store = set(id(p) for s in stores or [] for p in s.params)
    g = _latent(nets, ACC_SHAPE).clone().requires_grad_(True)
    f = _forward(nets, model, *_data(ACC_SHAPE), g_free=g)
    f["loss"].backward()
    assert g.grad is not None and torch.equal(g.grad, _hip(nets, ACC_SHAPE, False, frozen=True)["dg"])
    assert all(p.grad is None for p in model.parameters() if id(p) not in in_store)
    for s in stores or []:
        assert not s.grad_written and torch.equal(s.flat_g, _pattern(s.flat_g.numel(), "cuda"))
    after = dict(model.named_buffers())
    assert set(after) == set(buffers) and all(torch.equal(after[k], buffers[k]) for k in buffers)


def _same_bits(a, b):
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["g"], b["g"]) and torch.equal(a["pred"], b["pred"])
    for k, v in a["grads"].items():
        assert (v is None and b["grads"][k] is None) or torch.equal(v, b["grads"][k]), k
    for x, y in zip(a["flat_g"] or [], b["flat_g"] or []):
        assert torch.equal(x, y)


@pytest.mark.parametrize("flat", FLAT)
def test_two_fresh_models_give_identical_bits(flat):
    """3: two fresh models from the same state: the same loss bits and the same bits in every gradient"""
    nets = _gpu()
    _same_bits(_hip(nets, ACC_SHAPE, flat, fresh=True), _hip(nets, ACC_SHAPE, flat, fresh=True))


def test_identical_bits_beside_a_busy_stream():
    """3: the same with the Chamfer search of other clouds running on a second stream meanwhile (as
    test_gpu_chamfer_grad_det.test_repeatable_beside_a_busy_stream)"""
    nets = _gpu()
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    other = torch.randn(8, 2048, 3, device="cuda"), torch.randn(8, 2048, 3, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    runs = []
    for r in range(3):
        with torch.cuda.stream(side):
            for _ in range(4):
                BK.NNDistance(*other)
        runs.append(_hip(nets, ACC_SHAPE, True, fresh=True))
    torch.cuda.synchronize()
    for r in runs[1:]:
        _same_bits(runs[0], r)


def test_five_adam_steps_on_the_latent_repeat_bit_for_bit():
    """3: five steps of networks.Adam on g alone, parameters frozen, run twice from the same start: the five losses and the final g
    are bit-identical between the two runs (they are compared with each other only)"""
    nets = _gpu()
    start = _latent(nets, ACC_SHAPE)
    data = _data(ACC_SHAPE)

    def run():
        model, _ = _model(nets, False, frozen=True)
        g = start.clone().requires_grad_(True)
        opt = nets.Adam([g], lr=1e-2)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            f = _forward(nets, model, *data, g_free=g)
            f["loss"].backward()
            opt.step()
            losses.append(f["loss"].detach().clone())
        return torch.stack(losses), g.detach().clone()
    (la, ga), (lb, gb) = run(), run()
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert not torch.equal(ga, start) and len(set(la.tolist())) == 5


@pytest.mark.parametrize("shape", C.SHAPES)
def test_no_silent_fallback(shape):
    """4: every composed forward of this file goes through _forward, which turns an EvalModeAutogradWarning into an error and asserts
    the decoder's f16x3, the encoder's node under pooled and the other three nodes in the graph.  Here: that holds at every shape,
    and a sub-module quietly on tensor ops (or on the detached fused launch) makes _forward FAIL."""
    nets = _gpu()
    from dpf_nets_amd.networks.flows import EvalModeAutogradWarning
    for flat in FLAT:
        names = _hip(nets, shape, flat)["nodes"]
        suffix = "FlatBackward" if flat else "Backward"
        assert {"_FrozenPoolBackward", "_GPriorFrozen" + suffix, "_FlowStackFrozen" + suffix, "ChamferLossFunctionBackward"} <= set(names)
    data = _data(shape)
    for name, error in (("pc_decoder", EvalModeAutogradWarning), ("g_prior", EvalModeAutogradWarning), ("pc_encoder", AssertionError)):
        model, _ = _model(nets, False)
        getattr(model, name).eval_autograd = "torch"
        with pytest.raises(error):
            _forward(nets, model, *data)
