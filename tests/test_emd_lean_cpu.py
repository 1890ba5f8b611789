"""The approx-EMD entries that never store the matching (dpf_approxmatch_costonly_ws, dpf_matchcostgrad_recompute_ws), checked
without a GPU: declared, bound, exported, and -- on the ISA the cross-compiler emits with the Makefile's flags -- the matrix-core
gradient kernel holds MFMAs, no scratch access and no packed fp32, and the whole listing passes the emd.o rule's gate."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpf_nets_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = {"dpf_approxmatch_costonly_ws": 10, "dpf_matchcostgrad_recompute_workspace_bytes": 3, "dpf_matchcostgrad_recompute_ws": 12}


def _declaration(header, name):
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    assert m, name + " is not declared in include/dpf_hip.h"
    return [a for a in m.group(1).split(",") if a.strip()]


def test_new_entries_are_declared_in_the_header():
    header = open(os.path.join(ROOT, "include", "dpf_hip.h")).read()
    for name, arity in NEW.items():
        assert len(_declaration(header, name)) == arity, name


def test_new_entries_are_in_the_ctypes_table_with_matching_arity():
    from dpf_nets_amd import _lib
    header = open(os.path.join(ROOT, "include", "dpf_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(_declaration(header, name)), name
    import ctypes
    assert _lib.SIGNATURES["dpf_matchcostgrad_recompute_workspace_bytes"][0] is ctypes.c_size_t


def test_new_entries_are_exported_by_the_library():
    from dpf_nets_amd import _lib
    if not _lib.have_lib() or not shutil.which("nm"):
        pytest.skip("libdpf_hip.so is not built (or no nm)")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name


def _makefile_emd_rule():
    """(FLAGS, the listing's compile line, the gate's line) of emd.o as make would run them (a dry run: every variable expanded)"""
    if not shutil.which("make"):
        pytest.skip("no make")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*)$", mk, flags=re.M).group(1)
    rule = subprocess.run(["make", "-n", "-B", "-C", CSRC, "emd.o"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    compile_s = next(ln for ln in rule if " -S " in ln)
    gate = next(ln for ln in rule if "mfma_overlap_check.py" in ln)
    return flags, compile_s.strip(), gate.strip()


@pytest.fixture(scope="module")
def emd_listing(tmp_path_factory):
    """emd.hip's device assembly, compiled by the emd.o rule's own command line"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    flags, compile_s, _gate = _makefile_emd_rule()
    out = tmp_path_factory.mktemp("isa") / "emd.s"
    cmd = compile_s.replace("$(HIPCC)", HIPCC).replace("$(FLAGS)", flags).replace("$(ARCH)", "gfx950").replace("$(INC)", "-I../../include")
    cmd = cmd.split()
    assert cmd[-2:] == ["-o", "emd.s"], cmd
    cmd[-1] = str(out)
    r = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out), r.stderr


def _kernels(isa):
    parts = re.split(r"^(_Z[A-Za-z0-9_]+):[^\n]*$", isa, flags=re.M)
    return {parts[i]: re.split(r"^\.Lfunc_end\d+:", parts[i + 1], flags=re.M)[0] for i in range(1, len(parts) - 1, 2)}


def test_gradient_kernels_are_in_the_listing(emd_listing):
    path, remarks = emd_listing
    ks = _kernels(open(path).read())
    mfma = [b for n, b in ks.items() if "emd_mfma_grad_kernel" in n]
    valu = [b for n, b in ks.items() if "emd_materialize2_grad_kernel" in n]
    sums = [n for n in ks if "emd_grad2_recompute_sum_kernel" in n]
    assert len(mfma) == 1 and len(valu) == 1 and len(sums) == 2, sorted(ks)
    body = mfma[0]
    assert len(re.findall(r"\bv_mfma_f32_32x32x16_f16\b", body)) >= 4
    assert "scratch_" not in body
    assert not re.search(r"\bv_pk_\w+_f32\b", body)
    assert "scratch_" not in valu[0]
    assert "atomic" not in body and "atomic" not in valu[0]             # fixed-order partial sums, no float atomics
    for fn in ("emd_mfma_grad_kernel", "emd_materialize2_grad_kernel"):   # reported, not asserted
        block = [ln for ln in remarks.splitlines() if "remark:" in ln]
        at = next((i for i, ln in enumerate(block) if "Function Name" in ln and fn in ln), None)
        if at is not None:
            print("\n".join(ln.split("remark: ")[1] for ln in block[at:at + 10]))


def test_listing_passes_the_emd_rule_gate(emd_listing):
    path, _ = emd_listing
    _flags, _compile, gate = _makefile_emd_rule()
    argv = gate.split()
    assert argv[0] == "python3" and argv[1].endswith("mfma_overlap_check.py") and argv[-1] == "emd.s", argv
    assert "--no-scratch" in argv and "--no-packed-f32" in argv and "--require-register-c" in argv
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mfma_overlap_check.py")] + argv[2:-1] + [path],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
