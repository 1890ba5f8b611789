"""Timing of dpf_point_mesh_distance (csrc/point_mesh.hip) beside a chunked tensor-op brute force on the same device, and the
sweep behind the form boundary of dispatch::pm_form.  Not part of bench.py.

    python tools/point_mesh_bench.py [--out FILE]            B = 50 clouds of N = 2500 points against soups of 1 000 / 20 000 / 100 000 faces
    python tools/point_mesh_bench.py --sweep [--out FILE]    form 1 against form 2 over workgroup counts around the boundary

Events on the launch stream, warm-up first, the median of the timed repeats.  The baseline is the float32 tensor formulation a
user would write (three clamped segments and the plane per face, minimum over faces), chunked over points so that a chunk's
(points x faces) temporaries stay near 64 MB each; it is timed on --base-slots clouds and scaled to B, which is stated in the
output.  fp32 VALU fraction: the kernel's VALU instructions per (point, face) pair (counted in the assembly listing's inner
loop, --valu-per-pair) x pairs / time, against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_cases as MC                                                                     # noqa: E402
from dpf_nets_amd import datasets, metrics                                                  # noqa: E402

LANE_RATE = 256 * 4 * 16 * 2.4e9          # fp32 VALU lane-instructions per second at the nominal clock


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def brute_force(points, tri, chunk_elems=1 << 24):
    """points (N, 3), tri (F, 3, 3) float32 on the device -> (N,) squared distances, by tensor ops"""
    F = tri.shape[0]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n = torch.cross(b - a, c - a, dim=-1)
    nn = (n * n).sum(-1, keepdim=True).clamp_min(1e-30)
    step = max(1, chunk_elems // F)
    out = []
    for i in range(0, points.shape[0], step):
        p = points[i:i + step, None]
        best = None
        for s, e in ((a, b), (b, c), (c, a)):
            d = e - s
            t = (((p - s) * d).sum(-1, keepdim=True) / (d * d).sum(-1, keepdim=True).clamp_min(1e-30)).clamp(0, 1)
            dist = ((p - (s + t * d)) ** 2).sum(-1)
            best = dist if best is None else torch.minimum(best, dist)
        q = p - ((p - a) * n).sum(-1, keepdim=True) / nn * n
        inside = torch.ones_like(best, dtype=torch.bool)
        for s, e in ((a, b), (b, c), (c, a)):
            inside &= (torch.cross((e - s).expand_as(q), q - s, dim=-1) * n).sum(-1) >= 0
        plane = ((p - q) ** 2).sum(-1)
        best = torch.where(inside, torch.minimum(best, plane), best)
        out.append(best.min(1)[0])
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--base-slots", type=int, default=2)
    ap.add_argument("--valu-per-pair", type=float, default=0.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = (1000, 20000, 100000)
    meshes = [MC.soup(F, 400 + i) for i, F in enumerate(sizes)]
    store = datasets.MeshStore(*MC.pack(meshes), device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    if args.sweep:
        say("# form 1 (whole) against form 2 (split) -- ms, median of %d after %d warm-ups; wgs = B * ceil(N / 256)" % (args.repeats, args.warmup))
        say("# %6s %6s %8s %6s %10s %10s %10s" % ("B", "N", "F", "wgs", "form1", "form2", "form0"))
        for m, F in ((1, 20000), (2, 100000)):
            for B, N in ((1, 256), (1, 2048), (4, 2048), (8, 2500), (16, 2500), (25, 2500), (32, 2500), (50, 2500), (64, 2500), (100, 2500),
                         (200, 2500)):
                pts = torch.randn((B, N, 3), device=dev, generator=gen) * 0.4
                t = [timed(lambda f=f: metrics.point_mesh_distance(pts, store, [m] * B, form=f), args.warmup, args.repeats) for f in (1, 2, 0)]
                say("  %6d %6d %8d %6d %10.4f %10.4f %10.4f" % (B, N, F, B * ((N + 255) // 256), t[0], t[1], t[2]))
    else:
        B, N = 50, 2500
        say("# B = %d clouds of N = %d points; HIP: dpf_point_mesh_distance (form 0), median of %d after %d warm-ups" % (B, N, args.repeats, args.warmup))
        say("# baseline: chunked float32 tensor ops on %d clouds, scaled by %g" % (args.base_slots, B / args.base_slots))
        say("# %8s %12s %14s %8s %14s %10s" % ("F", "HIP ms", "baseline ms", "ratio", "Gpairs/s", "VALU frac"))
        for m, F in enumerate(sizes):
            pts = torch.randn((B, N, 3), device=dev, generator=gen) * 0.4
            hip = timed(lambda: metrics.point_mesh_distance(pts, store, [m] * B), args.warmup, args.repeats)
            tri = torch.from_numpy(meshes[m][0][meshes[m][1].astype(np.int64)]).to(dev)
            base = timed(lambda: [brute_force(pts[b], tri) for b in range(args.base_slots)], 1, 2) * B / args.base_slots
            d, _ = metrics.point_mesh_distance(pts, store, [m] * B)
            ref = brute_force(pts[0], tri)
            err = float((d[0] - ref).abs().max())
            pairs = B * N * F
            frac = args.valu_per_pair * pairs / (hip * 1e-3) / LANE_RATE if args.valu_per_pair else float("nan")
            say("  %8d %12.4f %14.2f %8.1f %14.2f %10.3f   (max |HIP - baseline| on cloud 0: %.2g)"
                % (F, hip, base, base / hip, pairs / (hip * 1e-3) / 1e9, frac, err))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
