"""Shared by tests/test_gpu_gprior_frozen.py and tests/test_gprior_frozen_cpu.py: the float64 reference of the eval-mode prior
flow under autograd -- the pinned oracle (oracle/gprior_oracle.py, training=False) on the CPU with the state's float tensors as
leaves -- and the seeded loss of tests/test_gpu_gprior.py::test_training_mode_vs_reference_golden."""
import numpy as np
import torch

from oracle import detrng
from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO

NAMES = ("gs", "mus", "lvs")


def projection_weights(seed, S, B, G, device="cpu", dtype=torch.float32):
    return [torch.from_numpy(detrng.normal_f32(detrng.key(seed, "gprior_r_" + name), (S, B, G))).to(device=device, dtype=dtype)
            for name in NAMES]


def projection_loss(lists, seed):
    """Each of the three stacked lists times its seeded normal tensor, summed."""
    loss = 0.0
    for lst, r in zip(lists, projection_weights(seed, len(lists[0]), *lists[0][0].shape, device=lists[0][0].device,
                                                dtype=lists[0][0].dtype)):
        loss = loss + (torch.stack(list(lst)) * r).sum()
    return loss


_CACHE = {}


def oracle64(seed, n_flows, nf, G, B, mode, mutate=None):
    """-> dict: gs, mus, lvs (S,B,G), dg (B,G) and grads {reference parameter name: gradient}, all float64 numpy.  Computed once
    per case and shared; callers must not write into it.  mutate(state, seed) (tests/gprior_train_ref.py) is applied to a copy of
    the seeded state first."""
    key = (seed, n_flows, nf, G, B, mode) + (() if mutate is None else (mutate.__name__,))
    if key not in _CACHE:
        state = GO.make_gprior_state(seed, n_flows, nf, G)
        if mutate is not None:
            state = mutate({k: np.array(v, copy=True) for k, v in state.items()}, seed)
        st = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in FO.to_torch(state).items()}
        params = {k: v.requires_grad_(True) for k, v in st.items()
                  if v.dtype == torch.float64 and "running" not in k and not k.endswith("eps")}
        g = torch.from_numpy(GO.gprior_inputs(seed, B, G)).double().requires_grad_(True)
        lists = GO.global_rnvp_decoder(st, n_flows, g, mode, training=False)
        projection_loss(lists, seed).backward()
        res = {name: torch.stack(lst).detach().numpy() for name, lst in zip(NAMES, lists)}
        res["dg"] = g.grad.numpy()
        res["grads"] = {k: v.grad.numpy() for k, v in params.items()}
        _CACHE[key] = res
    return _CACHE[key]


def rel(got, ref):
    """tests/test_gpu_gprior.py's measure: max-abs error over the reference's max-abs."""
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))
