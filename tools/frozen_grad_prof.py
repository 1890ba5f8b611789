"""Forward + backward time of the 63-layer point decoder under autograd, three paths from one run:
  (a) eval(), eval_autograd = "torch": tensor operations (the baseline)
  (b) eval(), eval_autograd = "hip":   the frozen-statistics HIP node (csrc/flow_frozen.hip)
  (c) train():                         the training-mode HIP step at the same shape
p, g and every parameter require grad; (b) is also timed with the parameters frozen.  HIP events on the launch stream, warm-up, median of --runs (>= 20).

    python tools/frozen_grad_prof.py [--clouds 32 8] [--points 2048] [--runs 20] > profiles/frozen_grad_prof.json
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpf_nets_amd import networks as nets          # noqa: E402


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[32, 8])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=20)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    torch.manual_seed(0)
    dec = nets.LocalCondRNVPDecoder(21, 64, 128, weight_std=0.01).cuda()
    out = {"device": torch.cuda.get_device_name(0), "n_flows": 21, "G": 128, "N": args.points, "runs": args.runs, "shapes": []}
    for B in args.clouds:
        p = (torch.randn(B, 3, args.points, device="cuda") * 0.3).requires_grad_(True)
        g = torch.randn(B, 128, device="cuda").requires_grad_(True)

        def step():
            ps, mus, lvs = dec(p, g, mode="inverse")
            (ps[0].square().mean() + sum(lvs).mean()).backward()
            dec.zero_grad(set_to_none=True)
            p.grad = g.grad = None

        row = {"B": B}
        dec.eval()
        dec.eval_autograd = "torch"
        row["a_eval_torch_ms"] = timed(step, 2, args.torch_runs)
        dec.eval_autograd = "hip"
        row["b_eval_hip_ms"] = timed(step, args.warmup, args.runs)
        dec.train()
        row["c_train_hip_ms"] = timed(step, args.warmup, args.runs)
        # (b) again with the parameters frozen (latent / input optimisation): no per-call repack and range verdict, no gather
        # and scatter of 2016 parameter gradients on the host -- what is left is the kernels and the node
        dec.eval()
        for q in dec.parameters():
            q.requires_grad_(False)
        row["b_eval_hip_inputs_only_ms"] = timed(step, args.warmup, args.runs)
        for q in dec.parameters():
            q.requires_grad_(True)
        out["shapes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
