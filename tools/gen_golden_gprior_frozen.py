"""Generate tests/golden/gprior_frozen.npz + .json: the reference's own GlobalRNVPDecoder (lib/networks/decoders.py:7-38) in
eval() mode UNDER AUTOGRAD on the CPU -- the three DIRECT-order lists, d/dg and a projection of every parameter gradient for
the seeded loss of tests/test_gpu_gprior.py::test_training_mode_vs_reference_golden (each stacked list times a seeded normal
tensor, summed).  Pins oracle/gprior_oracle.py for eval-mode gradients (tests/test_gprior_frozen_cpu.py) and the HIP path
itself (tests/test_gpu_gprior_frozen.py).

    python -m tools.gen_golden_gprior_frozen          (DPF_REFERENCE = the reference checkout; CPU only)

The reference is imported at generation time through oracle.gen_golden's helpers; nothing of it is stored but what it computed."""
import json
import os

import numpy as np
import torch

from oracle import detrng
from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO
from oracle import gen_golden as GG

CASES = {"a": (7, 2, 16, 8, 5), "b": (8, 1, 8, 2, 1)}             # seed, n_flows, n_features, G, B


def main():
    torch.set_num_threads(4)
    decoders = GG._import_reference()[1]
    out = {}
    for case, (seed, n_flows, nf, G, B) in CASES.items():
        st = GO.make_gprior_state(seed, n_flows, nf, G)
        g = torch.from_numpy(GO.gprior_inputs(seed, B, G))
        for mode in ("direct", "inverse"):
            dec = decoders.GlobalRNVPDecoder(n_flows, nf, G)
            dec.load_state_dict(FO.to_torch(st), strict=True)
            dec.eval()
            gin = g.clone().requires_grad_(True)
            lists = dec(gin, mode=mode)
            tag = "%s_%s_" % (case, mode)
            loss = 0.0
            for name, lst in zip(("gs", "mus", "lvs"), lists):
                out[tag + name] = torch.stack(lst).detach().numpy()
                r = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "gprior_r_" + name), (len(lst), B, G)))
                loss = loss + (torch.stack(lst) * r).sum()
            loss.backward()
            out[tag + "dg"] = gin.grad.numpy()
            for k, v in GG._grad_projection([(k, p.grad) for k, p in dec.named_parameters()], seed).items():
                out[tag + "gproj_" + k] = v
    np.savez_compressed(os.path.join(GG.OUT, "gprior_frozen.npz"), **out)
    with open(os.path.join(GG.OUT, "gprior_frozen.json"), "w") as f:
        json.dump({"cases": {k: list(v) for k, v in CASES.items()}}, f, indent=1)
    for name in ("gprior_frozen.npz", "gprior_frozen.json"):
        print(name, os.path.getsize(os.path.join(GG.OUT, name)))


if __name__ == "__main__":
    main()
