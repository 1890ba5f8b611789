"""Generate tests/golden/encoder_frozen.npz + .json: the reference's own PointNetCloudEncoder (lib/networks/encoders.py:9-28) in
eval() mode UNDER AUTOGRAD on the CPU, followed by the models' max over the points (models.py:106,124) -- pooled, d/dx and a
projection of the twelve parameter gradients for the seeded loss of oracle.gen_golden.gen_encoder (pooled times a seeded normal
tensor, summed).  Case "a" is the seeded state, case "b" the state of tests/encoder_frozen_ref.edge_state (negative and zero
BatchNorm scales in every layer, dead features).  Pins tests/encoder_frozen_ref.py for eval-mode gradients
(tests/test_encoder_frozen_cpu.py) and the HIP path itself (tests/test_gpu_encoder_frozen.py).

    python -m tools.gen_golden_encoder_frozen          (DPF_REFERENCE = the reference checkout; CPU only)

The reference is imported at generation time through oracle.gen_golden's helpers; nothing of it is stored but what it computed."""
import json
import os

import numpy as np
import torch

from oracle import detrng
from oracle import encoder_oracle as EO
from oracle import flow_oracle as FO
from oracle import gen_golden as GG
from tests.encoder_frozen_ref import edge_state

# seed, B, N, edge state.  Shapes and seeds are picked on the float64 restatement alone (a search over 700 seeds per shape): the
# live features' two largest values, their pooled values and the argmax points' 448 pre-activations stay 1.2e-5 (a) / 2.8e-5 (b)
# clear of a tie / of zero, relative to the tensor's largest magnitude -- some ten times the error of the bf16x3 forward -- so
# every precision of the HIP path routes the gradients as the reference's fp32 module does.  (Wider clearance does not exist at
# these sizes: ~250 live features and ~1000 pre-activations per cloud leave 3e-5 at best for one cloud of two points, 5e-6 for
# two clouds of five.)  Many features share each point, which is what the dx grouping needs.
CASES = {"a": (532, 1, 3, 0), "b": (245, 1, 2, 1)}


def main():
    torch.set_num_threads(4)
    GG._import_reference()
    from lib.networks import encoders
    out = {}
    for case, (seed, B, N, edge) in CASES.items():
        st = edge_state(seed) if edge else EO.make_encoder_state(seed)
        enc = encoders.PointNetCloudEncoder(3, 64, [128, 256, 512])
        enc.load_state_dict(FO.to_torch(st), strict=True)
        enc.eval()
        xin = torch.from_numpy(EO.encoder_inputs(seed, B, N)).requires_grad_(True)
        pooled = torch.max(enc(xin), dim=2)[0]
        r = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), tuple(pooled.shape)))
        (pooled * r).sum().backward()
        out[case + "_pooled"] = pooled.detach().numpy()
        out[case + "_dx"] = xin.grad.numpy()
        for k, v in GG._grad_projection([(k, p.grad) for k, p in enc.named_parameters()], seed).items():
            out[case + "_gproj_" + k] = v
    np.savez_compressed(os.path.join(GG.OUT, "encoder_frozen.npz"), **out)
    with open(os.path.join(GG.OUT, "encoder_frozen.json"), "w") as f:
        json.dump({"cases": {k: list(v) for k, v in CASES.items()}}, f, indent=1)
    for name in ("encoder_frozen.npz", "encoder_frozen.json"):
        print(name, os.path.getsize(os.path.join(GG.OUT, name)))


if __name__ == "__main__":
    main()
