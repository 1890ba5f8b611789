"""Times the deterministic Chamfer backward (dpf_nndistancegrad_det, dpf_chamfer_cd_backward) against two yardsticks it does not
touch: (a) dpf_nndistancegrad, the atomic backward, and (b) dpf_nndistance_cd, the forward search of the same shape.

    python tools/chamfer_grad_time.py [--out profiles/chamfer_grad_time.txt] [--calls 20] [--rounds 7]

Shapes: bench.py's cfg2 and cfg5 (read from its CONFIGS, the file is not edited), a rank-sized batch (4 clouds of cfg2's points)
and a collapsed target cloud at cfg5's size (every query in one list).  Method: every variant's `--calls` calls are captured into
one graph, so the kernels run back to back whatever the host's launch rate; a replay is timed with HIP events on the launch stream;
the variants alternate within a round and the per-call median over the rounds is reported (min beside it).  Needs the GPU: there
is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from dpf_nets_amd._lib import lib, check, current_stream  # noqa: E402
from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK  # noqa: E402


def shapes():
    c2, c5 = bench.CONFIGS["cfg2"], bench.CONFIGS["cfg5"]
    return [("cfg2", c2["clouds"], c2["points"], False), ("rank-sized", 4, c2["points"], False),
            ("cfg5", c5["clouds"], c5["points"], False), ("cfg5 collapsed", c5["clouds"], c5["points"], True)]


def variants(b, n, collapsed):
    L = lib()
    x1, x2 = torch.randn(b, n, 3, device="cuda"), torch.randn(b, n, 3, device="cuda")
    if collapsed:
        x2 = x2[:, :1].expand(b, n, 3).contiguous()
    d1, i1, d2, i2 = BK.NNDistance(x1, x2)
    gd1, gd2, gcd = torch.randn(b, n, device="cuda"), torch.randn(b, n, device="cuda"), torch.randn(b, device="cuda")
    g1, g2 = torch.empty(b, n, 3, device="cuda"), torch.empty(b, n, 3, device="cuda")
    cd = torch.empty(b, device="cuda")
    cdws = BK.CDWorkspace(b, n, n, x1.device)
    nbytes = L.dpf_nndistancegrad_det_workspace_bytes(b, n, n)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    keep = (x1, x2, d1, i1, d2, i2, gd1, gd2, gcd, g1, g2, cd, cdws, ws)
    P = lambda t: t.data_ptr()  # noqa: E731

    def forward():
        check(L.dpf_nndistance_cd(b, n, P(x1), n, P(x2), P(d1), P(i1), P(d2), P(i2), P(cd), P(cdws.buf), cdws.nbytes, 1, current_stream()), "cd")

    def atomic():
        check(L.dpf_nndistancegrad(b, n, P(x1), n, P(x2), P(gd1), P(i1), P(gd2), P(i2), P(g1), P(g2), current_stream()), "grad")

    def row(o1, o2, r1=gd1, r2=gd2):
        check(L.dpf_nndistancegrad_det(b, n, P(x1), n, P(x2), P(r1), P(i1), P(r2), P(i2), P(g1) if o1 else None, P(g2) if o2 else None,
                                       P(ws), nbytes, current_stream()), "det")

    def per_cloud(o1, o2):
        check(L.dpf_chamfer_cd_backward(b, n, P(x1), n, P(x2), P(i1), P(i2), P(gcd), P(g1) if o1 else None, P(g2) if o2 else None,
                                        P(ws), nbytes, current_stream()), "cd_backward")

    def rows_then_row():                        # what autograd does behind nn_distance + mean(1) + mean(1): expand / div / contiguous, both gradients
        r1 = (gcd[:, None].expand(b, n) / n).contiguous()
        r2 = (gcd[:, None].expand(b, n) / n).contiguous()
        row(True, True, r1, r2)

    return keep, [("forward search + CD (dpf_nndistance_cd)", forward), ("atomic backward (dpf_nndistancegrad)", atomic),
                  ("deterministic, rows, both outputs", lambda: row(True, True)), ("deterministic, rows, grad_xyz1 only", lambda: row(True, False)),
                  ("deterministic, per cloud, both outputs", lambda: per_cloud(True, True)),
                  ("deterministic, per cloud, grad_xyz1 only", lambda: per_cloud(True, False)),
                  ("expand / div / contiguous + deterministic rows, both", rows_then_row)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_grad_time: needs the GPU")
    lines = ["deterministic Chamfer backward, us per call (median / min of %d graph replays of %d back-to-back calls; %s)"
             % (args.rounds, args.calls, torch.cuda.get_device_name(0))]
    for name, b, n, collapsed in shapes():
        keep, vs = variants(b, n, collapsed)
        graphs = []
        for _, fn in vs:
            fn(); fn()                                     # warm-up outside the capture (code objects, LDS limits)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.calls):
                    fn()
            g.replay()
            graphs.append(g)
        torch.cuda.synchronize()
        times = [[] for _ in vs]
        for _ in range(args.rounds):
            for k, g in enumerate(graphs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); g.replay(); e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        lines.append("%s: B = %d, n = m = %d%s" % (name, b, n, ", target cloud collapsed to one point" if collapsed else ""))
        for (label, _), t in zip(vs, times):
            lines.append("    %-56s %9.2f / %9.2f" % (label, statistics.median(t), min(t)))
        del graphs, keep
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
