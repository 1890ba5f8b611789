"""Time one forward + backward of  torch.max(enc(x), 2)[0]  through the eval-mode PointNet encoder at N = 2048 (B = 8 and 32):

    python -m tools.encoder_frozen_time

  torch_x     eval(), eval_autograd = "torch", x requires grad: the tensor-op path (what every such call took before)
  hip_x       eval_autograd = "hip", x requires grad, the parameters are frozen (optimising a cloud through a frozen model)
  hip_all     eval_autograd = "hip", x and the twelve parameters require grad (the packed weights are refreshed on every call)
  train_hip   train() mode on csrc/encoder_train.hip, x and the parameters, for scale

HIP events on the launch stream around `--reps` warmed-up repetitions, and the host clock around the same repetitions and a
final synchronize (the two agree whichever side is the bottleneck; a difference would show time outside the stream); one JSON
line per (what, B).  The loss is the seeded one of the tests
(pooled times a fixed normal tensor, summed).  Needs a GPU; there is no CPU fallback.  For per-kernel times run it with small
--reps under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import time
import warnings

import torch

from oracle import detrng
from oracle import encoder_oracle as EO
from oracle import flow_oracle as FO

WHAT = {"torch_x": ("torch", False, True, False), "hip_x": ("hip", False, True, False), "hip_all": ("hip", False, True, True),
        "train_hip": ("torch", True, True, True)}             # eval_autograd, train(), x grad, parameter grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--what", default=",".join(WHAT))
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_frozen_time: needs a GPU")
    from dpf_nets_amd import networks as nets
    warnings.simplefilter("ignore")
    seed = 21
    for what in a.what.split(","):
        mode, train, x_grad, p_grad = WHAT[what]
        for B in (int(b) for b in a.batches.split(",")):
            enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512])
            enc.load_state_dict(FO.to_torch(EO.make_encoder_state(seed)), strict=True)
            enc = enc.cuda().train(train)
            enc.precision, enc.eval_autograd = a.precision, mode
            enc.requires_grad_(p_grad)
            x = torch.from_numpy(EO.encoder_inputs(seed, B, a.points)).cuda().requires_grad_(x_grad)
            r = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512))).cuda()

            def step():
                x.grad = None
                enc.zero_grad(set_to_none=True)
                (torch.max(enc(x), dim=2)[0] * r).sum().backward()

            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            t0.record()
            for _ in range(a.reps):
                step()
            t1.record()
            torch.cuda.synchronize()
            h1 = time.perf_counter()
            print(json.dumps({"what": what, "B": B, "N": a.points, "precision": a.precision, "reps": a.reps,
                              "ms_events": round(t0.elapsed_time(t1) / max(a.reps, 1), 4),
                              "ms_host": round((h1 - h0) * 1e3 / max(a.reps, 1), 4),
                              "dx_abs_sum": float(x.grad.abs().sum())}), flush=True)


if __name__ == "__main__":
    main()
