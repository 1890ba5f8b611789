"""bench.py's timed loop with several steps in flight (--streams S): every stream replays its own captured graph with its own
buffers, so steps that overlap on the chip must still produce exactly what a step produces alone."""
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steps_in_flight_produce_the_single_step_results():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, ROOT)
    import bench
    args = types.SimpleNamespace(batch=6, points=700, layers=6, latent=128, precision="f16x3", lists=False)
    dev = torch.device("cuda", 0)
    dec, state, n_flows, z, g, tgt, tgt_pm = bench.build_workload(args, dev, args.batch)
    step = bench.make_step(dec, z, g, tgt_pm, args.layers)
    ref = [t.clone() for t in step()]
    torch.cuda.synchronize()
    S = 3
    streams = [torch.cuda.Stream() for _ in range(S)]
    graphs, outs = [], []
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            step()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            outs.append(step())
        graphs.append(gr)
    for o in outs:                                   # poison the graphs' output buffers, then replay round-robin
        for t in o:
            t.zero_()
    for i in range(11):
        with torch.cuda.stream(streams[i % S]):
            graphs[i % S].replay()
    torch.cuda.synchronize()
    assert len({o[0].data_ptr() for o in outs}) == S                 # each stream has its own buffers
    for o in outs:
        for got, want in zip(o, ref):
            assert torch.equal(got, want)
    # the in-flight kernel timing helper runs and reports the three kernels
    kt = bench.kernel_timings_in_flight(dec, z, g, tgt_pm, args.layers, args.precision, 2, steps=12, warm=4)
    assert set(kt) == {"film_kernel", "flow_kernel", "nn_kernel"} and all(v > 0 for v in kt.values())


def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline alone; --dump-outputs writes what the timed
    path returned in its last step (13 steps: the last one is a one-step graph behind a 10-step graph), which must be what
    the same step computes in a fresh process."""
    import json
    import subprocess
    import numpy as np
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    sys.path.insert(0, ROOT)
    import bench
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "13", "--warmup", "2", "--settle", "0",
                        "--batch", "4", "--points", "512", "--layers", "6", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 13 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert not {"roofline", "cpu_baseline", "parity", "pipelined", "extra"} & set(line)
    args = types.SimpleNamespace(batch=4, points=512, layers=6, latent=128, precision="f16x3", lists=False)
    dev = torch.device("cuda", 0)
    dec, state, n_flows, z, g, tgt, tgt_pm = bench.build_workload(args, dev, args.batch)
    ref = bench.make_step(dec, z, g, tgt_pm, args.layers)()
    torch.cuda.synchronize()
    names = ("points", "sum_logvar", "dist1", "idx1", "dist2", "idx2", "chamfer_per_cloud")
    for name, want in zip(names, ref):
        got = np.load(out_dir / (name + ".npy"))
        want = want.cpu().numpy()
        assert got.dtype == (np.float32 if want.dtype == np.float32 else np.float64), name
        assert got.shape == want.shape and np.array_equal(got, want.astype(got.dtype)), name
