"""Time one forward + backward of the eval-mode prior flow under autograd: g_prior(g, mode='inverse') at the reference's
config (n_flows 7, n_features 128, G 128) with the loss of tests/test_gpu_gprior_frozen.py::test_partial_use_and_accumulation.

    python -m tools.gprior_frozen_time --impl hip            # eval_autograd = "hip": csrc/gprior_frozen.hip
    python -m tools.gprior_frozen_time --impl torch          # the tensor-op path (what every such call took before)

HIP events around `--reps` warmed-up repetitions per batch size; one JSON line per (batch size, what requires grad):
  latent    g requires grad, the parameters are frozen (latent optimisation: log p(g) as a prior term)
  finetune  g and every parameter require grad (the packed weights are refreshed on every call)
Needs a GPU; there is no CPU fallback.  For a launch count run it with small --reps under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import warnings

import torch

from oracle import flow_oracle as FO
from oracle import gprior_oracle as GO


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=("hip", "torch"), required=True)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", default="1,32,64")
    ap.add_argument("--n-flows", type=int, default=7)
    ap.add_argument("--what", default="latent,finetune")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gprior_frozen_time: needs a GPU")
    from dpf_nets_amd import networks as nets
    nf, G, seed = 128, 128, 21
    warnings.simplefilter("ignore")
    for what in a.what.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            dec = nets.GlobalRNVPDecoder(a.n_flows, nf, G)
            dec.load_state_dict(FO.to_torch(GO.make_gprior_state(seed, a.n_flows, nf, G)), strict=True)
            dec = dec.cuda().eval()
            dec.eval_autograd = a.impl
            dec.requires_grad_(what == "finetune")
            g = torch.from_numpy(GO.gprior_inputs(seed, B, G)).cuda().requires_grad_(True)

            def step():
                g.grad = None
                dec.zero_grad(set_to_none=True)
                gs, mus, lvs = dec(g, mode="inverse")
                (gs[0].square().mean() + sum(lvs).mean() + 1e-3 * (0.5 * mus[1]).sum()).backward()

            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                step()
            t1.record()
            torch.cuda.synchronize()
            print(json.dumps({"impl": a.impl, "what": what, "n_flows": a.n_flows, "B": B, "reps": a.reps,
                              "ms_per_forward_backward": round(t0.elapsed_time(t1) / max(a.reps, 1), 4),
                              "dg_abs_sum": float(g.grad.abs().sum())}), flush=True)


if __name__ == "__main__":
    main()
