"""Timing of dpf_mesh_point_distance (csrc/mesh_point.hip) in both kernel forms, beside a chunked tensor-op brute force of the same
column minimum and beside dpf_point_mesh_distance -- the sibling direction, which evaluates the same number of pairs -- on the
same inputs.  Not part of bench.py.

    python tools/mesh_point_bench.py [--out FILE]      B = 50 clouds of N = 2500 points against a soup of 20 000 faces, then a
                                                       few shapes around the form boundary of dispatch::mp_form

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  The baseline is
the float32 tensor formulation a user would write (three clamped segments and the plane per pair, minimum over the points),
chunked over points so that a chunk's (points x faces) temporaries stay near 64 MB each; it is timed on --base-slots clouds and
scaled to B, which is stated in the output."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mesh_cases as MC                                                                     # noqa: E402
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd import datasets, metrics                                                  # noqa: E402


def brute_force_cols(points, tri, chunk_elems=1 << 24):
    """points (N, 3), tri (F, 3, 3) float32 on the device -> (F,) squared distances to the nearest point, by tensor ops"""
    F = tri.shape[0]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n = torch.cross(b - a, c - a, dim=-1)
    nn = (n * n).sum(-1, keepdim=True).clamp_min(1e-30)
    step = max(1, chunk_elems // F)
    out = None
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
        best = torch.where(inside, torch.minimum(best, plane), best).min(0)[0]
        out = best if out is None else torch.minimum(out, best)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--base-slots", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sizes = (2500, 20000)
    meshes = [MC.soup(F, 400 + i) for i, F in enumerate(sizes)]
    store = datasets.MeshStore(*MC.pack(meshes), device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    B, N, m, F = 50, 2500, 1, 20000
    pts = torch.randn((B, N, 3), device=dev, generator=gen) * 0.4
    say("# B = %d clouds of N = %d points against F = %d faces: %.3g pairs; ms, median of %d after %d warm-ups" % (B, N, F, B * N * F, args.repeats, args.warmup))
    t = {f: timed(lambda f=f: metrics.mesh_point_distance(pts, store, [m] * B, form=f), args.warmup, args.repeats) for f in (1, 2, 0)}
    full = timed(lambda: metrics.mesh_point_distance(pts, store, [m] * B, return_closest=True, return_area=True), args.warmup, args.repeats)
    sib = timed(lambda: metrics.point_mesh_distance(pts, store, [m] * B), args.warmup, args.repeats)
    tri = torch.from_numpy(meshes[m][0][meshes[m][1].astype(np.int64)]).to(dev)
    base = timed(lambda: [brute_force_cols(pts[b], tri) for b in range(args.base_slots)], 1, 2) * B / args.base_slots
    d, _ = metrics.mesh_point_distance(pts, store, [m] * B)
    err = float((d[0] - brute_force_cols(pts[0], tri)).abs().max())
    req = pts.clone().requires_grad_(True)
    dist, _ = metrics.mesh_point_distance(req, store, [m] * B)
    g = torch.ones_like(dist)
    bwd = timed(lambda: torch.autograd.grad(dist, req, g, retain_graph=True), args.warmup, args.repeats)
    say("  mesh_point_distance  form 1 (whole) %10.4f   form 2 (split) %10.4f   form 0 %10.4f   form 0 with closest and area %10.4f" % (t[1], t[2], t[0], full))
    say("  point_mesh_distance  form 0         %10.4f   (the sibling direction, the same pairs: mesh_point / point_mesh = %.2f)" % (sib, t[0] / sib))
    say("  tensor-op brute force of the column minimum %10.2f   (%d clouds, scaled by %g; %.1f x the kernel; max |HIP - baseline| on cloud 0: %.2g)"
        % (base, args.base_slots, B / args.base_slots, base / t[0], err))
    say("  backward (one gather launch)        %10.4f" % bwd)
    say("  %.2f Gpairs/s (form 0)" % (B * N * F / (t[0] * 1e-3) / 1e9))
    say("# around the form boundary -- wgs = B * ceil(F / 256), point tiles = ceil(N / 256)")
    say("# %6s %6s %8s %6s %6s %10s %10s %10s" % ("B", "N", "F", "wgs", "tiles", "form1", "form2", "form0"))
    for mi, Fm in enumerate(sizes):
        for Bs, Ns in ((1, 2500), (4, 2500), (16, 2500), (50, 2500), (4, 20000)):
            p = torch.randn((Bs, Ns, 3), device=dev, generator=gen) * 0.4
            r = [timed(lambda f=f: metrics.mesh_point_distance(p, store, [mi] * Bs, form=f), args.warmup, args.repeats) for f in (1, 2, 0)]
            say("  %6d %6d %8d %6d %6d %10.4f %10.4f %10.4f" % (Bs, Ns, Fm, Bs * ((Fm + 255) // 256), (Ns + 255) // 256, r[0], r[1], r[2]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
