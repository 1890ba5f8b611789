"""Phase account of the Chamfer filter kernel nnm_kernel<16> at the headline shape (B = 32, n = m = 2048, the CD entry point).

Needs a -DDPF_PROFILE build of csrc/chamfer_mfma.hip (`make -C dpf_nets_amd/csrc prof` -> libdpf_hip_prof.so and the kept
chamfer_mfma_prof.s).  Prints, per phase, the shader cycles (s_memtime ticks) between the stamps of the 16 waves of
eight workgroups, and the instructions that stand between the same stamps in the assembly, by class.  The assembly count is
STATIC and in layout order: a loop body counts once (the evaluation rounds and the work-list loops run more than once), cold
blocks the compiler moved behind the kernel's end are listed under the stamp they follow.
    python tools/nnm_phase_prof.py [--lib PATH] [--asm PATH] [--asm-only]
    python tools/nnm_phase_prof.py --blocks dpf_nets_amd/csrc/chamfer_mfma.s      (the shipped kernel's hot blocks, by class)"""
import argparse
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# stamp k of a wave -> stamp k + 1, except where slots hold counters: 11 = evaluation rounds of the pass, 12 = the rounds the
# per-chunk evaluation (before r10) had made of the same masks, 13 = work items of the pass
PHASES = [(0, 1, "entry -> mu, query R2 known"), (1, 2, "fragment build (pass 0)"), (2, 3, "R2 reduce, barrier, tau"),
          (3, 4, "chunk 0: sweep"), (4, 5, "chunk 0: minimum, threshold, mask"), (5, 6, "chunk 1: sweep"),
          (6, 7, "chunk 1: minimum, final threshold, mask"), (7, 8, "pass: prune, scan, work list"), (8, 9, "pass: evaluation rounds"),
          (9, 10, "pass: owners merge"), (10, 14, "half merge, stores"), (14, 15, "sum, barrier, ticket, CD finish")]
STAMPS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 15]


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def asm_account(path, kernel="nnm_kernelILi16E"):
    """instructions of the kernel's body, split at its s_memtime stamps (layout order)"""
    body, inside = [], False
    for line in open(path):
        if not inside:
            inside = kernel in line and line.rstrip().split(":")[0].endswith("E") and line.startswith("_Z")
            continue
        if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
            break
        m = re.match(r"\t([a-z_0-9]+)", line)
        if m:
            body.append(m.group(1))
    segs = [{}]
    for op in body:
        if op == "s_memtime":
            segs.append({})
            continue
        c = classify(op)
        segs[-1][c] = segs[-1].get(c, 0) + 1
    return segs, body


def meta(path, kernel="nnm_kernelILi16E"):
    """register and scratch figures of the kernel from the amdhsa.kernels list of the listing's metadata"""
    text = open(path).read()
    text = text[text.find("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - ", text)[1:]:                      # one list entry per kernel
        m = re.search(r"\.name:\s+(\S+)", entry)
        if m and kernel in m.group(1):
            for key in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size"):
                out[key] = int(re.search(re.escape(key) + r":\s+(\d+)", entry).group(1))
    return out


def print_asm(path):
    segs, body = asm_account(path)
    tot = {}
    for op in body:
        tot[classify(op)] = tot.get(classify(op), 0) + 1
    print("assembly %s: nnm_kernel<16> %s" % (os.path.basename(path), meta(path)))
    print("  whole kernel, static: " + "  ".join("%s %d" % kv for kv in sorted(tot.items())))
    if len(segs) > 1:
        print("  between the stamps, layout order (segment k = after the k-th s_memtime of the listing; the stamps' own stores count)")
        for k, sg in enumerate(segs):
            print("   seg %2d: %-5d %s" % (k, sum(sg.values()), "  ".join("%s %d" % kv for kv in sorted(sg.items()))))


def block_account(path, kernel="nnm_kernelILi16E"):
    """instructions per basic block (label to label) of the kernel, by class; waits and s_nop apart from SALU"""
    blocks, cur, inside = [], None, False
    for line in open(path):
        if not inside:
            if line.startswith("_Z") and kernel in line.split(":")[0]:
                inside, cur = True, ["entry", {}, []]
                blocks.append(cur)
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"(\.LBB\d+_\d+):", line)
        if m:
            cur = [m.group(1), {}, []]
            blocks.append(cur)
            continue
        m = re.match(r"\t([a-z_0-9]+)", line)
        if m:
            op = m.group(1)
            c = "wait" if op in ("s_waitcnt", "s_nop") else classify(op)
            cur[1][c] = cur[1].get(c, 0) + 1
            cur[2].append(op)
    return blocks


CLASSES = ("VALU", "MFMA", "LDS", "SALU", "VMEM", "wait")


def print_blocks(path, rounds):
    """The three blocks a wave spends its issues in at the headline shape, found by what they hold -- the full-chunk sweep (32
    MFMAs and the fewest SALU: immediate offsets), the chunk's minimum + mask (the add-with-carry chain; before r10 the block also
    held the chunk's scan, which now stands once per pass behind the loop), a work-list evaluation round (ds_read_b128 of points +
    the owners' queries by ds_bpermute) -- and their sum per wave and pass: 2 chunks x (sweep + mask) + `rounds` x round.
    Prologue, build, prune + scan, list loops and epilogue are not in the sum."""
    bl = block_account(path)
    sweep = min((b for b in bl if b[1].get("MFMA", 0) == 32), key=lambda b: b[1].get("SALU", 0))
    mask = max(bl, key=lambda b: sum(1 for op in b[2] if op.startswith("v_addc_co")))
    rnd = max((b for b in bl if "ds_bpermute_b32" in b[2] and b[1].get("MFMA", 0) == 0),
              key=lambda b: sum(1 for op in b[2] if op == "ds_read_b128"))
    print("hot blocks of %s (unstamped listing), issues per execution: %s" % (os.path.basename(path), meta(path)))
    print("  %-28s %6s  %s" % ("block", "all", "  ".join("%5s" % c for c in CLASSES)))
    tot = dict.fromkeys(CLASSES, 0.0)
    for name, b, k in (("full-chunk sweep (32 tiles)", sweep, 2), ("minimum + mask", mask, 2), ("evaluation round (64 items)", rnd, rounds)):
        print("  %-28s %6d  %s   x %g   [%s]" % (name, sum(b[1].values()), "  ".join("%5d" % b[1].get(c, 0) for c in CLASSES), k, b[0]))
        for c in CLASSES:
            tot[c] += k * b[1].get(c, 0)
    print("  %-28s %6.0f  %s" % ("per wave and pass, these", sum(tot.values()), "  ".join("%5.0f" % tot[c] for c in CLASSES)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "dpf_nets_amd", "libdpf_hip_prof.so"))
    ap.add_argument("--asm", default=os.path.join(ROOT, "dpf_nets_amd", "csrc", "chamfer_mfma_prof.s"))
    ap.add_argument("--asm-only", action="store_true")
    ap.add_argument("--blocks", metavar="LISTING", help="hot-block issue counts of an UNSTAMPED chamfer_mfma.s, then exit")
    ap.add_argument("--rounds", type=float, default=1.2, help="evaluation rounds per wave and pass (measured at the headline shape: the account's last lines; 2.2 before r10)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    a = ap.parse_args()
    if a.blocks:
        print_blocks(a.blocks, a.rounds)
        return
    if os.path.exists(a.asm):
        print_asm(a.asm)
    if a.asm_only:
        return
    import numpy as np
    import torch
    from dpf_nets_amd import _lib
    _lib.lib_path = lambda: a.lib
    from oracle.gen_golden import chamfer_inputs
    h = _lib.lib()
    h.dpf_debug_set_nnm_prof.argtypes = [ctypes.c_void_p]
    B, n = a.batch, a.points
    x, y = chamfer_inputs(7, B, n, n)
    dev = torch.device("cuda", 0)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    d1 = torch.empty(B, n, device=dev); d2 = torch.empty(B, n, device=dev)
    i1 = torch.empty(B, n, dtype=torch.int32, device=dev); i2 = torch.empty(B, n, dtype=torch.int32, device=dev)
    cd = torch.empty(B, device=dev)
    ws = torch.zeros(h.dpf_nndistance_cd_workspace_bytes(B, n, n) // 4 + 4, dtype=torch.int32, device=dev)
    prof = torch.zeros((8, 16, 16), dtype=torch.int64, device=dev)

    def call():
        rc = h.dpf_nndistance_cd(B, n, x.data_ptr(), n, y.data_ptr(), d1.data_ptr(), i1.data_ptr(), d2.data_ptr(), i2.data_ptr(),
                                 cd.data_ptr(), ws.data_ptr(), ws.numel() * 4, 1, None)
        assert rc == 0, rc
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        prof.zero_()
        h.dpf_debug_set_nnm_prof(prof.data_ptr())
        call()
        torch.cuda.synchronize()
        h.dpf_debug_set_nnm_prof(None)
        runs.append(prof.cpu().numpy().astype(np.int64).reshape(-1, 16))
    t = np.stack(runs)                                   # (runs, 128 waves, 16 slots)
    assert (t[:, :, STAMPS] > 0).all(), "a stamp is missing: is this the headline shape (two chunks, one pass, a list within its capacity)?"
    print("library %s: B = %d, n = m = %d; shader cycles (s_memtime) per phase over %d runs x %d waves" % (os.path.basename(a.lib), B, n, t.shape[0], t.shape[1]))
    print("  %-38s %8s %8s %8s %8s" % ("phase", "median", "p10", "p90", "max"))
    for k0, k1, name in PHASES:
        v = (t[:, :, k1] - t[:, :, k0]).ravel()
        print("  %-38s %8.0f %8.0f %8.0f %8.0f" % (name, np.median(v), np.percentile(v, 10), np.percentile(v, 90), v.max()))
    tot = (t[:, :, 15] - t[:, :, 0]).ravel()
    print("  %-38s %8.0f %8.0f %8.0f %8.0f" % ("entry -> end, per wave", np.median(tot), np.percentile(tot, 10), np.percentile(tot, 90), tot.max()))
    wg = t.reshape(t.shape[0], 8, 16, 16)
    span = (wg[:, :, :, 15].max(axis=2) - wg[:, :, :, 0].min(axis=2)).ravel()
    print("  %-38s %8.0f %8.0f %8.0f %8.0f" % ("first entry -> last end, per workgroup", np.median(span), np.percentile(span, 10), np.percentile(span, 90), span.max()))
    tail = (wg[:, :, 0, 15] - wg[:, :, :, 14].max(axis=2)).ravel()
    print("  %-38s %8.0f %8.0f %8.0f %8.0f" % ("last wave's stores -> wave 0's end", np.median(tail), np.percentile(tail, 10), np.percentile(tail, 90), tail.max()))
    print("  per wave and pass (mean, min .. max): evaluation rounds %.2f (%d .. %d); evaluated per chunk the same masks gave %.2f (%d .. %d); "
          "work items %.1f (%d .. %d)" % (t[:, :, 11].mean(), t[:, :, 11].min(), t[:, :, 11].max(), t[:, :, 12].mean(), t[:, :, 12].min(),
                                          t[:, :, 12].max(), t[:, :, 13].mean(), t[:, :, 13].min(), t[:, :, 13].max()))


if __name__ == "__main__":
    main()
