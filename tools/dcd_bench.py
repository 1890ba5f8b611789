"""Timings of the density-aware Chamfer distance (csrc/dcd.hip) on the device -> profiles/dcd_forms.txt.  Not part of bench.py.

    python tools/dcd_bench.py [--out profiles/dcd_forms.txt] [--reps 15]

Every step is a child process of its own under its own time limit (a step that exceeds it is reported and the rest is skipped):
    launch       the dpf_dcd call alone on a stored nn_distance result, form 1 (counts in LDS, one launch) and form 2 (counts in the
                 workspace, four launches), the two alternating
    forward      metrics.density_aware_chamfer (NNDistance + dpf_dcd + reading the statuses) beside NNDistance alone
    loop         what the launch replaces: the per-cloud bincount / gather / exp / mean loop on tensor ops, on the same stored result
at 32 x 2048 x 2048 and 50 x 2500 x 2500 (the evaluation shapes); `launch` also at 1 x 32768 x 32768, the cap of form 1.
A sample is CALLS back-to-back calls between two stream synchronisations, divided by CALLS; the figure is the median of --reps samples
after 3 warm-up samples, with the lowest and highest sample as its spread."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((32, 2048, 2048), (50, 2500, 2500))
CAP_SHAPE = (1, 32768, 32768)
CALLS = 20
LIMITS = {"launch": 240, "forward": 240, "loop": 300}


def clouds(B, n, m, seed=0):
    """a Gaussian target and a prediction with half its points collapsed onto 8 spots of it: counts from 1 to n / 16"""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    y = (0.3 * rng.standard_normal((B, m, 3))).astype(np.float32)
    x = (0.3 * rng.standard_normal((B, n, 3))).astype(np.float32)
    x[:, n // 2:] = y[:, rng.integers(0, 8, size=n - n // 2)]
    dev = torch.device("cuda", 0)
    return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def samples_us(fns, reps, calls=CALLS):
    """{name: (median, lowest, highest)} in microseconds per call; the functions alternate sample by sample"""
    import torch
    times = {k: [] for k in fns}
    for r in range(reps + 3):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            if r >= 3:
                times[k].append((time.perf_counter() - t0) * 1e6 / calls)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return "%9.1f us (%.1f .. %.1f)" % t


def bincount_loop(d1, i1, d2, i2, alpha=1000.0):
    """calc_dcd as its users write it today: a Python loop over the batch, a bincount and a gather per cloud and side"""
    import torch
    out = []
    for b in range(d1.shape[0]):
        halves = []
        for d, i, t in ((d1[b], i1[b].long(), d2.shape[1]), (d2[b], i2[b].long(), d1.shape[1])):
            count = torch.bincount(i, minlength=t).gather(0, i).double()
            w = (d.numel() / t) / (count + 1e-6)
            halves.append((1 - torch.exp(-alpha * d.double()) * w).mean())
        out.append((halves[0] + halves[1]) / 2)
    return torch.stack(out).float()


def step(name, reps):
    import torch
    from dpf_nets_amd.metrics import density_aware_chamfer, density_aware_chamfer_raw
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    for B, n, m in SHAPES + ((CAP_SHAPE,) if name == "launch" else ()):
        x, y = clouds(B, n, m)
        d1, i1, d2, i2 = BK.NNDistance(x, y)
        shape = "%d x %d x %d" % (B, n, m)
        if name == "launch":
            t = samples_us({f: (lambda f=f: density_aware_chamfer_raw(d1, i1, d2, i2, form=f)) for f in (1, 2)}, reps)
            print("launch       %-18s form 1 %s   form 2 %s   (with the call's eight torch.empty)" % (shape, fmt(t[1]), fmt(t[2])))
        elif name == "forward":
            with torch.no_grad():
                t = samples_us({"dcd": lambda: density_aware_chamfer(x, y), "nn": lambda: BK.NNDistance(x, y)}, reps)
            print("forward      %-18s density_aware_chamfer %s   NNDistance alone %s" % (shape, fmt(t["dcd"]), fmt(t["nn"])))
        elif name == "loop":
            want = density_aware_chamfer(x, y)
            got = bincount_loop(d1, i1, d2, i2)
            assert torch.allclose(got, want, rtol=1e-6, atol=1e-7), float((got - want).abs().max())
            t = samples_us({"loop": lambda: bincount_loop(d1, i1, d2, i2)}, max(3, reps // 3), calls=2)
            print("loop         %-18s per-cloud bincount loop on tensor ops %s" % (shape, fmt(t["loop"])))
        else:
            raise SystemExit("unknown step " + name)
    print("device: " + torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcd_forms.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    lines = ["density-aware Chamfer distance (csrc/dcd.hip): tools/dcd_bench.py, medians of %d samples of %d calls (lowest .. highest sample)"
             % (args.reps, CALLS)]
    for name in ("launch", "forward", "loop"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            lines.append("%s: exceeded its limit of %d s; the remaining steps were not run" % (name, LIMITS[name]))
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append("%s: exit status %d; the remaining steps were not run\n%s" % (name, r.returncode, r.stderr[-2000:]))
            break
    text = "\n".join(dict.fromkeys(lines)) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if "not run" not in text else 1


if __name__ == "__main__":
    sys.exit(main())
