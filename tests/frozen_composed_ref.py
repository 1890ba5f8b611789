"""Shared by tests/test_gpu_frozen_composed.py and tests/test_frozen_composed_cpu.py: the latent-optimisation / fine-tuning graph of
the whole autoencoder in eval() mode

    g    = g_posterior(max over the points of pc_encoder(x)).mus
    gnll = GaussianFlowNLL over g_prior(g, "inverse") and g0_prior_mus / g0_prior_logvars     (losses.py:18-26, as models.py:136-140 lists them)
    pred = the last cloud of pc_decoder(noise * exp(0.5 logvar0) + mu0, g, "direct"),  (mu0, logvar0) = model._base(g)
    loss = sum over the clouds of [mean_i min_j |pred_i - target_j|^2 + mean_j min_i |pred_i - target_j|^2] + gnll

restated over the modules' `forward_torch` paths in whatever dtype the model has (float64: the reference; float32: the yardstick the
bars' max(node bar, factor x its error) form needs), with the two DISCRETE decisions handed in: the encoder's argmax (pooled is
gathered at `arg`, as tests/encoder_frozen_ref.autograd_reference does) and Chamfer's nearest neighbours (the distances are formed at
`idx1`, `idx2`).  None stands for the graph's own decision: the first point attaining the maximum, the first minimum.
A third decision can be handed in, `relu`: which of the 448 hidden units of the encoder's first three layers are live at every argmax
point, as the kernel's backward recomputed them.  It is TAKEN only at a near-tie -- a pre-activation of this graph within TIE_TOL of
zero relative to its layer's largest magnitude, tests/encoder_frozen_ref.near_zero_points' rule -- where the ReLU becomes the linear
map z * [live]; any other disagreement is counted in `relu_far` (a wrong decision of the kernel, for the caller to assert on).

The model is the smallest the kernels serve: the encoder's only architecture 3 -> 64 -> [128, 256, 512], G = 128, a prior flow of
2 couples (4 steps, 32 features), a point decoder of 2 triples (6 coupling layers, 64 features), the 'fixed' base distribution and a
posterior head without hidden layers (oracle/model_oracle.CONFIG at G = 128, whose seeded state is make_model_state's)."""
import math

import numpy as np
import torch

from oracle import detrng
from oracle import flow_oracle as FO
from oracle import model_oracle as MO

TIE_TOL = 1e-4             # tests/encoder_frozen_ref.TOL_OUT: the error the encoder's forward is allowed is what makes a sign undecidable
RELU_SEGMENTS = {"init_sd_relu": (0, 64), "sd0_relu": (64, 192), "sd1_relu": (192, 448)}      # a0 | a1 | a2 of a virtual point
G = 128
CFG = dict(MO.CONFIG, g_latent_space_size=G)
SEED = 11
# (B, N_in, S, M): clouds, points the encoder reads, points the decoder samples, points of the target
SHAPE_RAGGED = (3, 300, 200, 257)      # two encoder workgroups per cloud (256 points each), ragged tiles on every side, S != M
SHAPE_TINY = (1, 33, 40, 31)           # one cloud, less than one tile everywhere
SHAPE_BATCHED_FILM = (65, 33, 64, 64)  # past dpf_film_train_max_batch() = 64: the FiLM nets' batched tensor-op branch; S == M
SHAPES = (SHAPE_RAGGED, SHAPE_TINY, SHAPE_BATCHED_FILM)


_STATES = {}


def build_model(nets, seed=SEED, dtype=torch.float32, device="cpu"):
    """The seeded model in eval() mode (every BatchNorm with non-trivial running statistics); the state is drawn once per seed."""
    if seed not in _STATES:
        _STATES[seed] = FO.to_torch(MO.make_model_state(seed, CFG))
    model = nets.Local_Cond_RNVP_MC_Global_RNVP_VAE(**CFG)
    model.load_state_dict(_STATES[seed], strict=True)
    return model.to(device=device, dtype=dtype).eval()


def inputs(seed, shape, batch=0):
    """x (B,3,N_in), noise (B,3,S), target (B,M,3): float32 tensors; `batch` picks another draw of the three."""
    B, N, S, M = shape
    tag = "composed%d:" % batch
    x = detrng.normal_f32(detrng.key(seed, tag + "x"), (B, 3, N), 0.0, 0.25)
    noise = detrng.normal_f32(detrng.key(seed, tag + "noise"), (B, 3, S), 0.0, 1.0)
    target = detrng.normal_f32(detrng.key(seed, tag + "target"), (B, M, 3), 0.0, 0.25)
    return torch.from_numpy(x), torch.from_numpy(noise), torch.from_numpy(target)


def gaussian_flow_nll(samples, mus, logvars):
    """losses.py:18-26 with a plain sum over the list"""
    s0, m0, lv0 = samples[0], mus[0], logvars[0]
    return 0.5 * (torch.sum(sum(logvars) + (s0 - m0) ** 2 / torch.exp(lv0)) / s0.shape[0] + math.log(2.0 * math.pi) * s0.shape[1])


def chamfer_at(pred, target, idx1=None, idx2=None):
    """(B,) cd[b] = mean_i |pred_i - target_idx1[i]|^2 + mean_j |target_j - pred_idx2[j]|^2; None: the first minimum of this graph's
    own squared distances.  -> cd, idx1 (B,S), idx2 (B,M)"""
    if idx1 is None or idx2 is None:
        with torch.no_grad():
            d = ((pred[:, :, None, :] - target[:, None, :, :]) ** 2).sum(-1)                     # (B,S,M)
            idx1 = d.argmin(dim=2) if idx1 is None else idx1
            idx2 = d.argmin(dim=1) if idx2 is None else idx2
    idx1, idx2 = idx1.to(torch.int64), idx2.to(torch.int64)
    near1 = torch.gather(target, 1, idx1[:, :, None].expand(-1, -1, 3))
    near2 = torch.gather(pred, 1, idx2[:, :, None].expand(-1, -1, 3))
    d1 = ((pred - near1) ** 2).sum(-1)
    d2 = ((target - near2) ** 2).sum(-1)
    return d1.mean(1) + d2.mean(1), idx1, idx2


def encoder_features(enc, x, arg, relu):
    """forward_torch of the encoder with the ReLU decisions `relu` (B,512,448) of the argmax points taken at near-ties.
    -> features (B,512,N), decisions taken, disagreements away from a tie (or between two features sharing a point)"""
    B = x.shape[0]
    rows = torch.arange(B, device=x.device)[:, None].expand(B, arg.shape[1])
    taken = far = 0
    for name, mod in enc.features.named_children():
        if name not in RELU_SEGMENTS:
            x = mod(x)
            continue
        lo, hi = RELU_SEGMENTS[name]
        with torch.no_grad():
            z = x.detach()
            at = z.permute(0, 2, 1)[rows, arg]                                                  # (B,512,C): the virtual points' pre-activations
            hip = relu[:, :, lo:hi].to(z.device)
            tie = at.abs() <= TIE_TOL * z.abs().max()
            differ = hip != (at > 0)
            use = torch.where(tie, hip, at > 0)
            mask = z > 0
            mask.permute(0, 2, 1)[rows, arg] = use
            far += int((differ & ~tie).sum()) + int((mask.permute(0, 2, 1)[rows, arg] != use).sum())
            taken += int((differ & tie).sum())
        x = x * mask.to(x.dtype)
    return x, taken, far


def composed_loss(model, x, noise, target, arg=None, idx1=None, idx2=None, g_free=None, relu=None):
    """The graph above over forward_torch, in the model's dtype and on its device.  g_free (B,G): the latent itself is the input
    (latent optimisation: the encoder and the posterior head are not run).  -> dict: loss, cd, gnll, g, pooled, pred (B,S,3), arg, idx1, idx2, relu_taken, relu_far"""
    p0 = next(model.parameters())
    dt, dev = p0.dtype, p0.device
    noise, target = noise.to(device=dev, dtype=dt), target.to(device=dev, dtype=dt)
    pooled, taken, far = None, 0, 0
    if g_free is None:
        if relu is None:
            feat = model.pc_encoder.forward_torch(x.to(device=dev, dtype=dt))                     # (B,512,N)
        else:
            feat, taken, far = encoder_features(model.pc_encoder, x.to(device=dev, dtype=dt), arg.to(device=dev, dtype=torch.int64), relu)
        if arg is None:
            with torch.no_grad():
                arg = (feat == feat.max(dim=2, keepdim=True)[0]).to(torch.int64).argmax(dim=2)   # the first point attaining the maximum
        arg = arg.to(device=dev, dtype=torch.int64)
        pooled = torch.gather(feat, 2, arg[:, :, None])[..., 0]
        g = model.g_posterior(pooled)[0]
    else:
        g = g_free
    B = g.shape[0]
    gs, mus, lvs = model.g_prior.forward_torch(g, "inverse")
    gnll = gaussian_flow_nll(list(gs) + [g], [model.g0_prior_mus.expand(B, G)] + list(mus), [model.g0_prior_logvars.expand(B, G)] + list(lvs))
    mu0, lv0 = model._base(g, B, noise.shape[2])
    z = noise * torch.exp(0.5 * lv0[0]) + mu0[0]
    pred = model.pc_decoder.forward_torch(z, g, "direct")[0][-1].transpose(1, 2)
    cd, idx1, idx2 = chamfer_at(pred, target, None if idx1 is None else idx1.to(dev), None if idx2 is None else idx2.to(dev))
    return dict(loss=cd.sum() + gnll, cd=cd, gnll=gnll, g=g, pooled=pooled, pred=pred, arg=arg, idx1=idx1, idx2=idx2,
                relu_taken=taken, relu_far=far)


def grads_of(model):
    """{name: gradient clone or None} of every parameter"""
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def rel(got, ref, floor=0.0):
    """The per-node tests' measure: the largest error over the reference's largest magnitude (or `floor`, if that is larger)."""
    got, ref = got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (max(float(np.abs(ref).max()), floor) + 1e-30))
