"""Shared by tests/test_gpu_gprior_train.py and tests/test_gprior_train_cpu.py: the float64 references of the TRAINING-mode prior
flow (csrc/gprior_train.hip behind networks/prior_flows.py) --

  * `oracle64_train`: the pinned oracle (oracle/gprior_oracle.py, training=True) on the CPU under float64 autograd with the state's
    float tensors as leaves, and the BatchNorm running statistics after one step;
  * `step64`: a plain float64 restatement of one C-ABI call for an explicit list of step codes on a canonical block in either
    layout of include/dpf_hip.h (ordinary torch autograd, nothing of the kernel's host side);
  * the state mutators `hostile_bn` and `floor_active`, applied to the state dict before the GPU module and the oracle see it.

The seeded loss, the names and the error measure are tests/gprior_frozen_ref.py's."""
import numpy as np
import torch

from oracle import detrng
from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO
from tests.gprior_frozen_ref import NAMES, projection_loss, projection_weights, rel  # noqa: F401  (re-exported)

BN_EPS = 1e-5
NET_PIECES = ("mlp0.weight", "mlp0_bn.weight", "mlp0_bn.bias", "mlp0_bn.running_mean", "mlp0_bn.running_var", "mlp1.weight", "mlp1.bias")


# ---- state mutators ------------------------------------------------------------------------------------------------------------
def hostile_bn(state, seed):
    """Negative and zero BatchNorm scales and a dead hidden unit, in every net: the sign of round(0.4 nf) seeded entries of every
    mlp0_bn.weight is flipped (never entry 0), entry 0 is set to exactly 0, and the last row of every mlp0.weight is zeroed -- that
    hidden unit is exactly 0 on every row: batch variance 0, rstd = 1 / sqrt(bn_eps)."""
    for k in sorted(state):
        if k.endswith("mlp0_bn.weight"):
            w = state[k]
            nf = w.shape[0]
            order = np.argsort(detrng.uniform(detrng.key(seed, "hostile:" + k), nf - 1), kind="stable") + 1
            w[order[:max(1, int(round(0.4 * nf)))]] *= np.float32(-1.0)
            w[0] = 0.0
        elif k.endswith("mlp0.weight"):
            state[k][-1, :] = 0.0
    return state


def floor_active(state, seed):
    """Every second entry of logvar_mlp1.bias at -14, every fourth at -20: exp(o) falls to and below eps = 1e-6, so the
    log(eps + exp(.)) floor and its derivative exp(o) / (eps + exp(o)) are active (logvars from about -13.8 up to 1)."""
    for k in sorted(state):
        if k.endswith("logvar_mlp1.bias"):
            state[k][::2] = -14.0
            state[k][::4] = -20.0
    return state


def make_state(seed, n_flows, nf, G, mutate=None):
    """The seeded state (numpy, reference names) after `mutate(state, seed)`: what the GPU module loads and the oracle reads."""
    state = {k: np.array(v, copy=True) for k, v in GO.make_gprior_state(seed, n_flows, nf, G).items()}
    if mutate is not None:
        state = mutate(state, seed)
    return state


def inputs(seed, B, G, g_offset=0.0):
    """The seeded (B,G) codes plus a constant, rounded to fp32 once: the GPU and the oracle start from the same numbers."""
    return (GO.gprior_inputs(seed, B, G) + np.float32(g_offset)).astype(np.float32)


# ---- the oracle under float64 autograd -----------------------------------------------------------------------------------------
_CACHE = {}


def oracle64_train(seed, n_flows, nf, G, B, mode, mutate=None, g_offset=0.0):
    """-> dict: gs, mus, lvs (S,B,G), dg (B,G), grads {reference parameter name: gradient} and stats {running-statistics name: value
    after one step at momentum 0.1 with the unbiased variance}, all float64 numpy.  Computed once per case and shared; callers must
    not write into it."""
    key = (seed, n_flows, nf, G, B, mode, getattr(mutate, "__name__", None), float(g_offset))
    if key not in _CACHE:
        st = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in FO.to_torch(make_state(seed, n_flows, nf, G, mutate)).items()}
        params = {k: v.requires_grad_(True) for k, v in st.items()
                  if v.dtype == torch.float64 and "running" not in k and not k.endswith("eps")}
        g = torch.from_numpy(inputs(seed, B, G, g_offset)).double().requires_grad_(True)
        stats = {}
        lists = GO.global_rnvp_decoder(st, n_flows, g, mode, training=True, stats_out=stats)
        projection_loss(lists, seed).backward()
        res = {name: torch.stack(lst).detach().numpy() for name, lst in zip(NAMES, lists)}
        res["dg"] = g.grad.numpy()
        res["grads"] = {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in params.items()}
        res["stats"] = {k: v.detach().numpy() for k, v in stats.items()}
        _CACHE[key] = res
    return _CACHE[key]


# ---- canonical blocks ----------------------------------------------------------------------------------------------------------
def module_codes(n_flows):
    """The step codes GlobalRNVPDecoder emits: couples of pattern i % 2, nvp1 then nvp2."""
    return [2 * (i % 2) + k for i in range(n_flows) for k in range(2)]


def param_blocks(S, nf, G, params_only):
    """[(reference parameter name, offset, shape)] of the first S steps inside a block of the given layout, the block's floats, and
    the running-statistics slots [(offset, floats)] (none in the parameters-only layout)."""
    K, out, stat_slots, off = G // 2, [], [], 0
    for prefix, warp, keep in GO.step_plan((S + 1) // 2, G)[:S]:
        for br in ("mu", "logvar"):
            base = "%sT_%s_0.%s_" % (prefix, br, br)
            for name, shape in (("mlp0.weight", (nf, K)), ("mlp0_bn.weight", (nf,)), ("mlp0_bn.bias", (nf,))):
                out.append((base + name, off, shape)); off += int(np.prod(shape))
            if not params_only:
                stat_slots.append((off, 2 * nf)); off += 2 * nf
            for name, shape in (("mlp1.weight", (K, nf)), ("mlp1.bias", (K,))):
                out.append((base + name, off, shape)); off += int(np.prod(shape))
    return out, off, stat_slots


def canon_block(state, S, G, params_only):
    """The first S steps of a reference-named state as one fp32 block in either layout of include/dpf_hip.h."""
    pieces = []
    for prefix, warp, keep in GO.step_plan((S + 1) // 2, G)[:S]:
        for br in ("mu", "logvar"):
            base = "%sT_%s_0.%s_" % (prefix, br, br)
            pieces += [state[base + k].ravel() for k in NET_PIECES if not (params_only and "running" in k)]
    return np.concatenate(pieces).astype(np.float32)


# ---- one C-ABI call in float64 -------------------------------------------------------------------------------------------------
def code_indices(code, G):
    """(warped, kept) coordinates of a step code: 0 even, 1 odd, 2 first half, 3 second half are the WARPED ones."""
    K = G // 2
    warp = list((range(0, G, 2), range(1, G, 2), range(0, K), range(K, G))[code])
    return warp, [i for i in range(G) if i not in set(warp)]


def step64(block, params_only, codes, G, nf, g, mode, weights, eps=GO.EPS, bn_eps=BN_EPS):
    """dpf_gprior_train_forward + _backward restated: `block` (fp32 numpy, either layout) holds len(codes) steps, g (B,G) fp32
    numpy, `weights` three (S,B,G) arrays or None per list (the NULL gradient tables) defining the loss sum(list * weight).
    -> dict: gs, mus, lvs (S,B,G), dg (B,G), dcanon (the block's layout, zeros where nothing flows), stats (S,2,2nf) = batch mean |
    biased variance (mu net, then logvar net); float64 numpy."""
    S, K, B = len(codes), G // 2, g.shape[0]
    eps = float(np.float32(eps))                                  # the C ABI takes a float, and the oracle reads the fp32 buffer
    leaf = torch.from_numpy(np.asarray(block, dtype=np.float64)).requires_grad_(True)
    gin = torch.from_numpy(np.asarray(g, dtype=np.float64)).requires_grad_(True)
    nbn = 2 if params_only else 4
    cn = 2 * nf * K + nbn * nf + K
    assert leaf.numel() == S * 2 * cn, (leaf.numel(), S, cn)
    gs, mus, lvs, stats = [None] * S, [None] * S, [None] * S, [None] * S
    cur = gin
    for s in (range(S) if mode == "direct" else range(S - 1, -1, -1)):
        warp, keep = code_indices(codes[s], G)
        x, o, st = cur[:, keep], [], []
        for net in range(2):
            p = leaf[(2 * s + net) * cn:(2 * s + net + 1) * cn]
            w0, gam, bet = p[:nf * K].view(nf, K), p[nf * K:nf * K + nf], p[nf * K + nf:nf * K + 2 * nf]
            q = p[nf * K + nbn * nf:]
            w1, b1 = q[:K * nf].view(K, nf), q[K * nf:]
            h = x @ w0.t()
            mean = h.mean(0)
            var = ((h - mean) ** 2).mean(0)
            y = (h - mean) / torch.sqrt(var + bn_eps) * gam + bet
            o.append((y * torch.sigmoid(y)) @ w1.t() + b1)
            st += [mean.detach(), var.detach()]
        mu, lv = torch.zeros_like(cur), torch.zeros_like(cur)
        mu[:, warp] = o[0]
        lv[:, warp] = torch.log(eps + torch.exp(o[1]))
        cur = torch.exp(0.5 * lv) * cur + mu if mode == "direct" else torch.exp(-0.5 * lv) * (cur - mu)
        gs[s], mus[s], lvs[s] = cur, mu, lv
        stats[s] = torch.stack([torch.cat([st[0], st[2]]), torch.cat([st[1], st[3]])])
    res = {name: torch.stack(lst) for name, lst in zip(NAMES, (gs, mus, lvs))}
    loss = None
    for name, w in zip(NAMES, weights):
        if w is not None:
            term = (res[name] * torch.from_numpy(np.asarray(w, dtype=np.float64))).sum()
            loss = term if loss is None else loss + term
    if loss is not None:
        loss.backward()
    res = {k: v.detach().numpy() for k, v in res.items()}
    res["dg"] = gin.grad.numpy() if gin.grad is not None else np.zeros((B, G))
    res["dcanon"] = leaf.grad.numpy() if leaf.grad is not None else np.zeros(leaf.numel())
    res["stats"] = torch.stack(stats).numpy()
    return res
