"""float64 restatement of the TRAINING-mode PointNet encoder + max over the points + backward, with the tie rule of
csrc/encoder_train.hip written down (not collected; tests/test_encoder_train_ref_cpu.py checks it, tests/test_gpu_encoder_train_edges.py
uses it).  Per layer l = 0..3, over all n = B N points:

    y_l = W_l a_{l-1}      mean_l, var_l (biased) over the points      xhat_l = (y_l - mean_l) rstd_l,  rstd_l = 1 / sqrt(var_l + 1e-5)
    z_l = gamma_l xhat_l + beta_l      a_l = relu(z_l)

    arg[b, f]  = the lowest point index attaining max_p y_3[b, f, p] when gamma_3[f] rstd_3[f] >= 0, min_p y_3 otherwise
    pooled     = relu(z_3 at arg)                     (max pooling with the subgradient at ties fixed: a gather, never torch.max)

    dz_3 = g [pooled > 0] at arg, zero elsewhere      dbeta_l = sum dz_l      dgamma_l = sum dz_l xhat_l
    dy_l = gamma_l rstd_l (dz_l - dbeta_l / n - xhat_l dgamma_l / n)      dW_l = dy_l^T a_{l-1}      dz_{l-1} = [z_{l-1} > 0] dy_l W_l

    running_mean <- (1 - m) running_mean + m mean_l      running_var <- (1 - m) running_var + m var_l n / (n - 1)   (torch.nn.BatchNorm1d)

Two points of a cloud with identical coordinates have identical y_3 (every point goes through the same arithmetic); "the lowest
index attaining the extreme" is then the lowest index among the winner's copies.  The restatement takes the copies from the
coordinates, so that it does not depend on whether a float64 GEMM gives two equal rows the same last bit.

SEEDS: every GPU case's seed is picked on this float64 restatement alone (seed_is_clean): a ReLU whose pre-activation lies within
the forward error of zero takes the other subgradient, and a runner-up within the forward error of the winner takes the sparse
gradient to another point; neither is an error of the kernel, so the cases keep DELTA clear of both."""
import numpy as np
import torch

from oracle import detrng
from oracle import encoder_oracle as EO
from tests.encoder_frozen_ref import LAYERS, EPS, edge_state, param_names

TOL_OUT, TOL_GRAD, TOL_STAT = 1e-4, 5e-4, 2e-5      # the bars of tests/test_gpu_encoder_train.py
DELTA = 1e-6                                         # >= 10 x the forward error of bf16x6 (4-9e-8)
STATES = ("plain", "signs", "all_down", "dead_mid")
SHAPES = ((2, 5), (3, 33), (5, 700))
SHIFT = 8.0
RULES = ("contract", "max_y3", "last")               # the kernel's pooling rule, and two deliberately wrong ones


# ---- states and inputs -----------------------------------------------------------------------------------------------
def make_state(name, seed):
    """plain: the seeded state.  signs: in every layer gamma < 0 on 1::5, gamma = 0 on 3::16; last-layer beta = -50 on 2::9.
    all_down: every last-layer gamma negated (every (cloud, feature) pools through the tile minima).  dead_mid: in each of
    layers 0-2 beta = -50 on 2::11 (dead at every point) and then gamma = 0, beta = +0.7 on 5::13 (a constant positive activation;
    an index in both, 57 the first, is of the second kind)."""
    if name == "signs":
        return edge_state(seed)
    st = {k: np.array(v, copy=True) for k, v in EO.make_encoder_state(seed).items()}
    if name == "all_down":
        st["features.sd2_bn.weight"] *= -1.0
    elif name == "dead_mid":
        for layer in LAYERS[:3]:
            g, b = st["features.%s_bn.weight" % layer], st["features.%s_bn.bias" % layer]
            b[2::11] = -50.0
            g[5::13] = 0.0
            b[5::13] = 0.7
    elif name != "plain":
        raise ValueError(name)
    return st


def with_duplicates(x):
    """point 0 of every cloud copied onto point N-1 and, for N > 40, point 3 onto point 35 (a tie across a 32-point tile boundary)"""
    x = x.clone()
    N = x.shape[2]
    x[:, :, N - 1] = x[:, :, 0]
    if N > 40:
        x[:, :, 35] = x[:, :, 3]
    return x


def case_clouds(seed, B, N, kind):
    """the float32 clouds a case feeds, one per training call.  kind: plain | dup | shift (+8 on every axis) | pair (two calls)"""
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N))
    if kind == "plain":
        return [x]
    if kind == "dup":
        return [with_duplicates(x)]
    if kind == "shift":
        return [x + SHIFT]
    if kind == "pair":
        return [x, torch.from_numpy(EO.encoder_inputs(seed + 1000, B, N))]
    raise ValueError(kind)


def case_inputs(B, N, state, kind="plain"):
    """-> seed, numpy state, [clouds (B,3,N) float32], g (B,512) float32"""
    key = (B, N, state, kind)
    seed = SEEDS[key] if key in SEEDS else LEAST_UNCLEAN[key][0]
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512)))
    return seed, make_state(state, seed), case_clouds(seed, B, N, kind), g


def _t(st, key):
    return torch.from_numpy(np.asarray(st[key])).to(torch.float64)


# ---- the restatement --------------------------------------------------------------------------------------------------
def _copies(x):
    """first[b, p] / last[b, p]: the lowest / highest point index of cloud b with the coordinates of point p"""
    B, _, N = x.shape
    same = (x[:, :, :, None] == x[:, :, None, :]).all(1)                   # (B,N,N)
    idx = torch.arange(N)
    first = torch.where(same, idx[None, None, :], torch.full((), N)).min(2)[0]
    last = torch.where(same, idx[None, None, :], torch.full((), -1)).max(2)[0]
    return same, first, last


def forward(st, x, rule="contract"):
    """st: numpy state; x (B,3,N).  -> dict: per layer y, mean, var, rstd, xhat, z (over the B N points, cloud-major), a (inputs
    of the layers), arg, pooled, key (what arg maximises: y3 or -y3 per feature, (B,N,512))"""
    x = x.to(torch.float64)
    B, _, N = x.shape
    W = [_t(st, "features.%s.weight" % n)[0] for n in LAYERS]
    gam = [_t(st, "features.%s_bn.weight" % n) for n in LAYERS]
    bet = [_t(st, "features.%s_bn.bias" % n) for n in LAYERS]
    out = {k: [] for k in ("y", "mean", "var", "rstd", "xhat", "z")}
    a = [x.permute(0, 2, 1).reshape(B * N, 3)]
    for l in range(4):
        y = a[-1] @ W[l].t()
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        rstd = 1.0 / torch.sqrt(var + EPS)
        xhat = (y - mean) * rstd
        z = xhat * gam[l] + bet[l]
        for k, v in zip(("y", "mean", "var", "rstd", "xhat", "z"), (y, mean, var, rstd, xhat, z)):
            out[k].append(v)
        a.append(torch.relu(z))
    y3 = out["y"][3].reshape(B, N, 512)
    up = (gam[3] * out["rstd"][3] >= 0) if rule != "max_y3" else torch.ones(512, dtype=torch.bool)
    key = torch.where(up, y3, -y3)
    _, first, last = _copies(x)
    winner = key.argmax(1)                                                 # (B,512): any of the winner's copies
    arg = torch.gather(last if rule == "last" else first, 1, winner)
    z3 = out["z"][3].reshape(B, N, 512)
    pooled = torch.relu(torch.gather(z3, 1, arg[:, None, :])[:, 0])
    out.update(a=a[:4], arg=arg, pooled=pooled, key=key, W=W, gam=gam, B=B, N=N)
    return out


def backward(fw, g):
    """fw: forward(); g (B,512) -> dx (B,3,N), {state key: gradient}"""
    B, N = fw["B"], fw["N"]
    n = float(B * N)
    gz = torch.where(fw["pooled"] > 0, g.to(torch.float64), torch.zeros((), dtype=torch.float64))
    dz = torch.zeros(B, N, 512, dtype=torch.float64)
    dz.scatter_(1, fw["arg"][:, None, :], gz[:, None, :])
    dz = dz.reshape(B * N, 512)
    grads = {}
    for l in (3, 2, 1, 0):
        name = LAYERS[l]
        xhat = fw["xhat"][l]
        dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
        dy = fw["gam"][l] * fw["rstd"][l] * (dz - dbeta / n - xhat * (dgamma / n))
        grads["features.%s_bn.bias" % name] = dbeta
        grads["features.%s_bn.weight" % name] = dgamma
        grads["features.%s.weight" % name] = (dy.t() @ fw["a"][l])[None]
        da = dy @ fw["W"][l]
        if l > 0:
            dz = torch.where(fw["z"][l - 1] > 0, da, torch.zeros((), dtype=torch.float64))
    return da.reshape(B, N, 3).permute(0, 2, 1).contiguous(), grads


def running_stats(st, fws, momentum, unbiased=True, once=False):
    """the eight running statistics after one training call per entry of fws (forward() results), starting from st.
    unbiased=False and once=True (only the last call's update is applied) are the deliberately wrong variants."""
    out = {}
    for l, name in enumerate(LAYERS):
        rm, rv = _t(st, "features.%s_bn.running_mean" % name), _t(st, "features.%s_bn.running_var" % name)
        for fw in (fws[-1:] if once else fws):
            n = float(fw["B"] * fw["N"])
            var = fw["var"][l] * (n / (n - 1.0)) if unbiased else fw["var"][l]
            rm = (1.0 - momentum) * rm + momentum * fw["mean"][l]
            rv = (1.0 - momentum) * rv + momentum * var
        out["features.%s_bn.running_mean" % name] = rm
        out["features.%s_bn.running_var" % name] = rv
    return out


def restate(st, xs, g, momentum=0.1, rule="contract", unbiased=True, once=False):
    """One training call per cloud of xs.  -> dict: pooled, arg, dx, grads of the LAST call; stats after all of them; fw (last call)"""
    fws = [forward(st, x, rule) for x in xs]
    dx, grads = backward(fws[-1], g)
    return {"pooled": fws[-1]["pooled"], "arg": fws[-1]["arg"], "dx": dx, "grads": grads,
            "stats": running_stats(st, fws, momentum, unbiased, once), "fw": fws[-1]}


def structural_zeros(st, fw):
    """Where the gradients are zero by structure, with the margin of seed_is_clean so that the kernel's ReLUs decide alike:
    -> dead_pooled (512,) bool: pooled[:, f] = 0 in every cloud; dead[l] (C_l,) bool, l = 0..2: feature dead at every point;
    zero_gamma[l] (C_l,) bool, l = 0..3: gamma_l = 0 (dy_l = 0, so row f of dW_l is zero)"""
    dead = [(fw["z"][l] < -DELTA * fw["z"][l].abs().max()).all(0) for l in range(3)]
    return (fw["pooled"] == 0).all(0), dead, [fw["gam"][l] == 0 for l in range(4)]


# ---- condition on the seeds ---------------------------------------------------------------------------------------------
def seed_is_clean(st, x, delta=DELTA):
    """On the float64 restatement alone: (ReLU margin) no pre-activation of layers 0-2 at an argmax point, and no z3 at arg, lies
    within delta x (that layer's largest |z|) of zero; (argmax gap) for every feature with gamma3 != 0 the winner leads the best
    runner-up of OTHER coordinates by more than delta x max |y3|.  -> (clean, number of near-zero pre-activations, number of
    narrow gaps)"""
    fw = forward(st, x)
    B, N = fw["B"], fw["N"]
    pts = torch.zeros(B, N, dtype=torch.bool)
    pts.scatter_(1, fw["arg"], torch.ones(B, 512, dtype=torch.bool))
    pts = pts.reshape(-1)
    near = 0
    for l in range(3):
        z = fw["z"][l]
        near += int((z[pts].abs() <= delta * z.abs().max()).sum())
    z3 = fw["z"][3].reshape(B, N, 512)
    near += int((torch.gather(z3, 1, fw["arg"][:, None, :]).abs() <= delta * z3.abs().max()).sum())
    same, _, _ = _copies(x.to(torch.float64))
    key = fw["key"]
    win = torch.gather(key, 1, fw["arg"][:, None, :])                        # (B,1,512)
    other = ~torch.gather(same, 1, fw["arg"][:, :, None].expand(B, 512, N)).permute(0, 2, 1)      # (B,N,512): not a copy of the winner
    runner = torch.where(other, key, torch.full((), -float("inf"), dtype=torch.float64)).max(1)[0]
    live = fw["gam"][3] != 0
    narrow = int(((win[:, 0] - runner <= delta * fw["y"][3].abs().max()) & live).sum())
    return near == 0 and narrow == 0, near, narrow


def case_is_clean(B, N, state, kind, seed):
    st = make_state(state, seed)
    return all(seed_is_clean(st, x)[0] for x in case_clouds(seed, B, N, kind))


def ties_are_sharp(B, N, state, seed):
    """a dup case can tell "the last winning point" from the first: the two restatements' dx differ by more than 100 x TOL_GRAD"""
    st, (x,) = make_state(state, seed), case_clouds(seed, B, N, "dup")
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512)))
    return rel(backward(forward(st, x, "last"), g)[0], backward(forward(st, x), g)[0]) > 100.0 * TOL_GRAD


def scan(B, N, state, kind, seeds=range(1, 201)):
    """the first clean seed of 1..200 -- for a dup case the first clean one whose ties are sharp (how SEEDS was filled; CPU only)"""
    for seed in seeds:
        if case_is_clean(B, N, state, kind, seed) and (kind != "dup" or ties_are_sharp(B, N, state, seed)):
            return seed
    return None


# ---- the GPU cases: (B, N, state, kind) -> the first seed of 1..200 that seed_is_clean accepts (scan) -------------------------
SEEDS = {
    (2, 5, "plain", "plain"): 1, (3, 33, "plain", "plain"): 2, (5, 700, "plain", "plain"): 12,
    (2, 5, "signs", "plain"): 1, (3, 33, "signs", "plain"): 1, (5, 700, "signs", "plain"): 7,
    (2, 5, "all_down", "plain"): 1, (3, 33, "all_down", "plain"): 2, (5, 700, "all_down", "plain"): 14,
    (2, 5, "dead_mid", "plain"): 1, (3, 33, "dead_mid", "plain"): 2,
    (3, 33, "plain", "dup"): 1, (5, 700, "plain", "dup"): 1, (3, 33, "signs", "dup"): 1, (5, 700, "signs", "dup"): 11,
    (3, 33, "plain", "pair"): 2, (1, 2, "plain", "plain"): 1,
    (3, 33, "plain", "shift"): 2, (5, 700, "plain", "shift"): 12,
}
# dead_mid at (5,700) has NO clean seed in 1..200: beta = -50 makes its layers' largest |z| ten times the seeded state's, so DELTA x
# max |z| is 5e-5 where the other states have 5e-6, and a seed has 15 near-zero pre-activations at the median (a longer scan cannot
# pick around that).  The case is kept, at the seed of 1..200 with the fewest violations, recorded here as (seed, near-zero
# pre-activations, narrow gaps); tests/test_encoder_train_ref_cpu.py holds the record to seed_is_clean's own count.
LEAST_UNCLEAN = {(5, 700, "dead_mid", "plain"): (103, 5, 1)}


# ---- helpers shared by the CPU and GPU tests --------------------------------------------------------------------------------
def load_module(enc, st, dtype=torch.float64):
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    return enc.to(dtype).train()


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))
