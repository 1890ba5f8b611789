"""csrc/dispatch.h decides which kernel form serves a call: pure functions of (shape, switches), checked here without a GPU.

A tiny program with its own main() is compiled with the host compiler alone (dispatch.h includes no HIP header) and prints the
form chosen for every query below.  The expectations are written out by hand from the conditions of the launch code the header
replaced, each pair of cases at and one past a threshold.  The approx-EMD slice counts (test_emd_slices) were recorded from
that earlier code's picker functions, copied verbatim into a scratch program and run at the shapes the suite uses.

Flow: the pair / single layers-per-buffer choice is reachable only with DPF_FLOW_SKEW=0 at a two-part precision; bf16x6
(three parts) takes neither the skewed nor the pair form, whatever DPF_FLOW_LPB says.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

PROBE = r"""
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "dispatch.h"
using namespace dispatch;
static bool assign(Switches &sw, const std::string &tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    const std::string k = tok.substr(0, eq);
    const int v = atoi(tok.c_str() + eq + 1);
    struct { const char *name; int Switches::*field; } fields[] = {
        {"flow_tile16", &Switches::flow_tile16}, {"flow16_cw", &Switches::flow16_cw}, {"flow16_split", &Switches::flow16_split},
        {"flow_waves", &Switches::flow_waves}, {"flow_lpb", &Switches::flow_lpb}, {"flow_skew", &Switches::flow_skew},
        {"nn_small", &Switches::nn_small}, {"nn_ksw", &Switches::nn_ksw}, {"nn_ks", &Switches::nn_ks}, {"nnm_qw", &Switches::nnm_qw},
        {"emd_matrix_env", &Switches::emd_matrix_env}, {"emd_matrix_set", &Switches::emd_matrix_set},
        {"train_split", &Switches::train_split}, {"train_roles", &Switches::train_roles},
        {"train_fuse_colsum", &Switches::train_fuse_colsum}};
    for (auto &f : fields) if (k == f.name) { sw.*(f.field) = v; return true; }
    return false;
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        in >> kind;
        long a[6] = {0, 0, 0, 0, 0, 0};
        int na = 0;
        Switches sw;                                      // every switch "not set"
        while (in >> tok) {
            if (assign(sw, tok)) continue;
            if (tok.find('=') != std::string::npos || na == 6) { printf("bad token %s\n", tok.c_str()); return 2; }
            a[na++] = atol(tok.c_str());
        }
        if (kind == "flow") {                             // L B N precision has_xs packed16_ok
            const FlowForm f = flow_form((int)a[0], (int)a[1], (int)a[2], (int)a[3], a[4] != 0, a[5] != 0, sw);
            if (f.kernel == FlowKernel::Tile32) printf("tile32 fw=%d lpb=%d xs_rows=%d\n", f.fw, f.lpb, f.xs_rows);
            else printf("%s cw=%d\n", f.kernel == FlowKernel::Tile16Split ? "tile16split" : "tile16", f.cw);
        } else if (kind == "small") {
            printf("%d\n", nn_small_serves((int)a[0], (int)a[1], (int)a[2], sw) ? 1 : 0);
        } else if (kind == "nn") {
            const NNForm f = nn_form((int)a[0], (int)a[1], (int)a[2], sw);
            printf("%s %d\n", f.kernel == NNKernel::Staged ? "staged" : f.kernel == NNKernel::Sliced ? "sliced" : "scan", f.width);
        } else if (kind == "pays") {
            printf("%d\n", nnm_pays((int)a[0], (int)a[1], (int)a[2], sw) ? 1 : 0);
        } else if (kind == "qw") {                        // b n m force16
            printf("%d\n", nnm_qw((int)a[0], (int)a[1], (int)a[2], a[3] != 0, sw));
        } else if (kind == "pqw") {
            printf("%d\n", pairwise_qw((int)a[0]));
        } else if (kind == "emd") {                       // deferred
            printf("%d\n", emd_matrix_family(a[0] != 0, sw) ? 1 : 0);
        } else if (kind == "pick") {
            const int b = (int)a[0], n = (int)a[1], m = (int)a[2];
            printf("match=%d mfma=%d slices=%d grad=%d\n", pick_match_slices(b, n, m), pick_mfma_slices(b, n, m), pick_slices(b, n, m),
                   pick_grad_slices(b, n, m));
        } else if (kind == "gradform") {                  // b n m has_workspace
            const GradForm g = grad_form((int)a[0], (int)a[1], (int)a[2], a[3] != 0);
            printf("%s\n", g == GradForm::TwoPass ? "twopass" : g == GradForm::Fused2 ? "fused2" : "fused1");
        } else if (kind == "train") {                     // ns nblk n_cu
            const TrainForm f = train_form((int)a[0], (int)a[1], (int)a[2], sw);
            printf("h1=%d s1=%d s2=%d roles=%d fuse=%d\n", f.split_h1, f.split1, f.split2, f.roles, f.fuse_colsum);
        } else if (kind == "env") {                       // the process's environment, then the setters
            const Switches e = snapshot();
            printf("%d %d %d %d %d %d | %d %d %d %d | %d %d | %d %d %d ; ", e.flow_tile16, e.flow16_cw, e.flow16_split, e.flow_waves,
                   e.flow_lpb, e.flow_skew, e.nn_small, e.nn_ksw, e.nn_ks, e.nnm_qw, e.emd_matrix_env, e.emd_matrix_set, e.train_split,
                   e.train_roles, e.train_fuse_colsum);
            const int old = set_mode(settable().flow_tile16, 7), now = set_mode(settable().flow_tile16, -5);
            const int m0 = settable().emd_matrix.exchange(0), m1 = snapshot().emd_matrix_set;
            printf("set %d %d %d | %d %d\n", old, now, snapshot().flow_tile16, m0, m1);
        } else {
            printf("bad kind %s\n", kind.c_str());
            return 2;
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    d = tmp_path_factory.mktemp("dispatch")
    (d / "probe.cpp").write_text(PROBE)
    exe = d / "probe"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", str(ROOT / "include"), "-I", str(ROOT / "dpf_nets_amd" / "csrc"),
                    str(d / "probe.cpp"), "-o", str(exe)], check=True)

    def ask(cases, env=None):
        """cases: {query: expected answer}; one run of the program answers them all"""
        clean = {k: v for k, v in os.environ.items() if not k.startswith("DPF_")}
        out = subprocess.run([str(exe)], input="\n".join(cases) + "\n", env={**clean, **(env or {})}, text=True,
                             capture_output=True, check=True).stdout.splitlines()
        assert len(out) == len(cases), out
        got = dict(zip(cases, out))
        wrong = {q: (got[q], want) for q, want in cases.items() if got[q] != want}
        assert not wrong, f"(got, expected) per query: {wrong}"

    return ask


F16X3, BF16, BF16X3, BF16X6 = 4, 1, 2, 3


def flow(B, N, *sw, L=2, prec=F16X3, xs=0, p16=1):
    return " ".join(["flow", str(L), str(B), str(N), str(prec), str(xs), str(p16), *sw])


def test_flow_kernel_thresholds(probe):
    probe({
        # B ceil(N / 16) <= 1024 tiles: the 16-point kernel; B ceil(N / 64) >= 160 there: 4 compute waves
        flow(1, 16384): "tile16 cw=4",
        flow(2, 8192): "tile16 cw=4",
        flow(1, 16385): "tile32 fw=4 lpb=1 xs_rows=129",          # 1025 tiles; 65 workgroups of 256 points < 224
        # <= 512 tiles: a tile's two branches on two waves
        flow(1, 8192): "tile16split cw=4",
        flow(1, 8193): "tile16 cw=2",                             # 513 tiles; 129 < 160
        flow(1, 9000): "tile16 cw=2",                             # 141 < 160
        flow(1, 10240): "tile16 cw=4",                            # 160
        # who never gets the 16-point kernel
        flow(1, 1024, prec=BF16): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, prec=BF16X3): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, prec=BF16X6): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, xs=1): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, L=129): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, p16=0): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024, "flow_tile16=0"): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(1, 1024): "tile16split cw=4",
        # mode 1: whenever the precision allows
        flow(1, 16385, "flow_tile16=1"): "tile16 cw=4",
        flow(1, 16385, "flow_tile16=1", prec=BF16X3): "tile32 fw=4 lpb=1 xs_rows=129",
        flow(1, 16385, "flow_tile16=1", xs=1): "tile32 fw=4 lpb=1 xs_rows=129",
        # the forced forms of the 16-point kernel
        flow(1, 16384, "flow16_cw=2"): "tile16 cw=2",
        flow(1, 9000, "flow16_cw=4"): "tile16 cw=4",
        flow(1, 16384, "flow16_split=1"): "tile16split cw=4",
        flow(1, 8192, "flow16_split=0"): "tile16 cw=2",           # 128 < 160
    })


def test_flow_workgroup_waves_and_layers_per_buffer(probe):
    off = "flow_tile16=0"
    probe({
        # B ceil(N / 256) < 224: 4-wave workgroups; 8 waves take the skewed form at the one- and two-part precisions
        flow(223, 256): "tile32 fw=4 lpb=1 xs_rows=2",
        flow(224, 256): "tile32 fw=8 lpb=0 xs_rows=1",
        flow(224, 256, prec=BF16): "tile32 fw=8 lpb=0 xs_rows=1",
        flow(224, 256, prec=BF16X3): "tile32 fw=8 lpb=0 xs_rows=1",
        # small clouds
        flow(1, 65, off): "tile32 fw=4 lpb=1 xs_rows=1",
        flow(1, 64, off): "tile32 fw=2 lpb=1 xs_rows=1",
        flow(1, 33, off): "tile32 fw=2 lpb=1 xs_rows=1",
        flow(1, 32, off): "tile32 fw=1 lpb=1 xs_rows=1",
        flow(300, 64, off): "tile32 fw=2 lpb=1 xs_rows=1",
        # three parts: neither skewed nor paired, whatever the switches say
        flow(224, 256, prec=BF16X6): "tile32 fw=8 lpb=1 xs_rows=1",
        flow(224, 256, "flow_lpb=2", prec=BF16X6): "tile32 fw=8 lpb=1 xs_rows=1",
        flow(257, 256, "flow_skew=0", prec=BF16X6): "tile32 fw=8 lpb=1 xs_rows=1",
        # without the skewed form: two layers per buffer up to 256 workgroups, and as DPF_FLOW_LPB forces
        flow(224, 256, "flow_skew=0", prec=BF16X3): "tile32 fw=8 lpb=2 xs_rows=1",
        flow(256, 256, "flow_skew=0"): "tile32 fw=8 lpb=2 xs_rows=1",
        flow(257, 256, "flow_skew=0"): "tile32 fw=8 lpb=1 xs_rows=1",
        flow(257, 256, "flow_skew=0", "flow_lpb=2"): "tile32 fw=8 lpb=2 xs_rows=1",
        flow(224, 256, "flow_skew=0", "flow_lpb=1"): "tile32 fw=8 lpb=1 xs_rows=1",
        flow(224, 256, "flow_skew=0", L=1): "tile32 fw=8 lpb=1 xs_rows=1",
        flow(224, 256, "flow_skew=0", "flow_lpb=2", L=1): "tile32 fw=8 lpb=1 xs_rows=1",
        # xs_rows = ceil(N / (32 fw)), from the waves actually launched
        flow(300, 1000, prec=BF16X3, xs=1): "tile32 fw=8 lpb=0 xs_rows=4",
        flow(300, 1000, "flow_waves=4", prec=BF16X3, xs=1): "tile32 fw=4 lpb=1 xs_rows=8",
        flow(300, 1000, "flow_waves=3", prec=BF16X3, xs=1): "tile32 fw=2 lpb=1 xs_rows=16",
        flow(300, 1000, "flow_waves=1", prec=BF16X3, xs=1): "tile32 fw=1 lpb=1 xs_rows=32",
        flow(1, 40, "flow_waves=16", prec=BF16X3, xs=1): "tile32 fw=8 lpb=0 xs_rows=1",
    })


def test_chamfer_staged_scan_serves(probe):
    probe({
        # min cloud >= 1024, max cloud <= 8192, ceil(nmax / 64) b 2 <= 256 workgroups
        "small 4 2048 2048": "1",
        "small 5 2048 2048": "0",
        "small 4 1023 2048": "0",
        "small 4 1024 2048": "1",
        "small 1 8192 8192": "1",
        "small 1 8193 8193": "0",
        "small 4 2048 2048 nn_small=0": "0",
        "small 5 2048 2048 nn_small=1": "1",
        "small 1 100 100 nn_small=1": "1",
        "small 1 8193 8193 nn_small=1": "0",
        "small 65536 100 100 nn_small=1": "0",
    })


def test_chamfer_scan_forms(probe):
    probe({
        # the staged scan: 4 waves when 4 per workgroup are >= 2048, else 8
        "nn 4 2048 2048": "staged 8",
        "nn 7 2048 2048 nn_small=1": "staged 8",                  # 448 workgroups
        "nn 8 2048 2048 nn_small=1": "staged 4",                  # 512
        "nn 4 2048 2048 nn_ksw=4": "staged 4",
        "nn 4 2048 2048 nn_ksw=16": "staged 16",
        "nn 4 2048 2048 nn_ksw=5": "staged 16",
        # DPF_NN_KS keeps the staged scan out
        "nn 4 2048 2048 nn_ks=8": "sliced 8",
        "nn 4 2048 2048 nn_ks=16": "sliced 16",
        "nn 4 2048 2048 nn_ks=4": "scan 4",
        # waves1 = b (ceil(n / 128) + ceil(m / 128)) < 512 with min cloud >= 1024: 8 slices
        "nn 5 2048 2048": "sliced 8",
        "nn 15 2048 2048": "sliced 8",                            # 480
        "nn 16 2048 2048": "scan 4",                              # 512
        "nn 4 1023 2048": "scan 4",
        "nn 31 2048 2048": "scan 4",                              # 992
        "nn 32 2048 2048": "scan 2",                              # 1024
        "nn 63 2048 2048": "scan 2",                              # 2016
        "nn 64 2048 2048": "scan 1",                              # 2048
        "nn 1 63 63": "scan 1",
        "nn 1 63 64": "scan 4",
        "nn 4 2048 2048 nn_small=0": "sliced 8",
    })


def test_chamfer_matrix_core_filter(probe):
    probe({
        # fewer than 64 eight-wave workgroups: no, however many pairs
        "pays 1 7936 8192": "0",                                  # 31 + 32
        "pays 1 8192 8192": "1",                                  # 64; 1.3e8 pairs
        # >= 1e8 pairs: yes, also beyond one pass
        "pays 6 4070 2048": "1",                                  # 100 024 320
        "pays 6 4069 2048": "0",                                  # 99 999 744
        # the 3e7 band: one pass (<= 2048 points) and not where the staged scan serves
        "pays 8 2048 2048": "1",
        "pays 8 2049 2048": "0",
        "pays 4 2500 2500": "0",
        "pays 4 2048 2048": "0",
        "pays 4 2048 2048 nn_small=0": "1",
        "pays 5 2048 2048 nn_small=1": "0",
        "pays 4 2048 1800 nn_small=0": "0",                       # 2.95e7
        "pays 0 2048 2048": "0",
        # its workgroup: 16 waves at >= 128 workgroups of 16, then 8 at >= 128 of 8, else 4
        "qw 16 2048 2048 0": "16",
        "qw 15 2048 2048 0": "8",
        "qw 8 2048 2048 0": "8",
        "qw 7 2048 2048 0": "4",
        "qw 7 2048 2048 1": "16",
        "qw 16 2048 2048 0 nnm_qw=4": "4",
        "qw 7 2048 2048 0 nnm_qw=8": "8",
        "qw 7 2048 2048 0 nnm_qw=16": "16",
        "qw 16 2048 2048 0 nnm_qw=5": "16",
        "pqw 256": "8",
        "pqw 257": "16",
    })


def test_emd_family(probe):
    probe({
        "emd 1": "1",
        "emd 1 emd_matrix_set=0": "0",
        "emd 1 emd_matrix_env=0": "0",
        "emd 1 emd_matrix_set=0 emd_matrix_env=0": "0",
        "emd 0": "0",
    })


def test_emd_slices(probe):
    probe({
        "pick 32 2048 2048": "match=8 mfma=8 slices=2 grad=4",
        "pick 16 8192 8192": "match=4 mfma=4 slices=1 grad=2",
        "pick 2 8192 8192": "match=16 mfma=8 slices=8 grad=8",
        "pick 64 2048 2048": "match=4 mfma=4 slices=1 grad=2",
        "pick 1 33 700": "match=8 mfma=4 slices=8 grad=8",
        "gradform 32 2048 2048 1": "twopass",
        "gradform 16 8192 8192 1": "fused2",
        "gradform 2 8192 8192 1": "twopass",
        "gradform 64 2048 2048 1": "fused2",
        "gradform 1 33 700 1": "twopass",
        # b ceil(n / 256) workgroups: < 512 two passes, < 1024 two row slices (where m >= 4 * 21), else one
        "gradform 511 256 2048 1": "twopass",
        "gradform 512 256 2048 1": "fused2",
        "gradform 1023 256 84 1": "fused2",
        "gradform 1023 256 83 1": "fused1",
        "gradform 1024 256 2048 1": "fused1",
        "gradform 1024 256 2048 0": "twopass",
    })


def test_training_forms(probe):
    probe({
        "train 2 64 256": "h1=1 s1=1 s2=1 roles=1 fuse=1",
        "train 2 65 256": "h1=0 s1=0 s2=1 roles=1 fuse=1",
        "train 2 128 256": "h1=0 s1=0 s2=1 roles=0 fuse=1",        # 2 * 128 + 17 > 256
        "train 2 129 256": "h1=0 s1=0 s2=0 roles=0 fuse=1",
        "train 3 129 256": "h1=0 s1=0 s2=1 roles=0 fuse=1",
        "train 3 1000 256": "h1=0 s1=0 s2=1 roles=0 fuse=1",
        "train 3 64 256": "h1=1 s1=1 s2=1 roles=1 fuse=1",
        # roles while 2 nblk + 17 <= n_cu (17 is odd: 256 itself is never met; 255 is)
        "train 2 119 256": "h1=0 s1=0 s2=1 roles=1 fuse=1",        # 255
        "train 2 120 256": "h1=0 s1=0 s2=1 roles=0 fuse=1",        # 257
        "train 2 119 255": "h1=0 s1=0 s2=1 roles=1 fuse=1",        # at the count
        "train 2 119 254": "h1=0 s1=0 s2=1 roles=0 fuse=1",        # one past it
        # forced
        "train 2 10 256 train_split=0": "h1=0 s1=0 s2=0 roles=0 fuse=1",
        "train 3 10 256 train_split=0": "h1=0 s1=0 s2=1 roles=1 fuse=1",
        "train 2 500 256 train_split=1": "h1=1 s1=1 s2=1 roles=0 fuse=1",
        "train 2 128 256 train_roles=1": "h1=0 s1=0 s2=1 roles=1 fuse=1",
        "train 2 10 256 train_roles=0": "h1=1 s1=1 s2=1 roles=0 fuse=1",
        "train 2 129 256 train_roles=1": "h1=0 s1=0 s2=0 roles=0 fuse=1",
        "train 2 10 256 train_fuse_colsum=0": "h1=1 s1=1 s2=1 roles=1 fuse=0",
    })


def test_environment_is_read_once_with_todays_defaults_and_the_setters_exchange(probe):
    # unset: the defaults; dpf_flow_set_tile16's clamp (7 -> 1, -5 -> -1) and the old value coming back
    probe({"env": "-1 0 -1 0 0 1 | -1 0 0 0 | 1 1 | -1 -1 1 ; set -1 1 -1 | 1 0"})
    probe({"env": "1 2 0 4 2 0 | 0 16 8 4 | 0 1 | 1 0 0 ; set 1 1 -1 | 1 0"},
          env={"DPF_FLOW_TILE16": "1", "DPF_FLOW16_CW": "2", "DPF_FLOW16_SPLIT": "0", "DPF_FLOW_WAVES": "4", "DPF_FLOW_LPB": "2",
               "DPF_FLOW_SKEW": "0", "DPF_NN_SMALL": "0", "DPF_NN_KSW": "16", "DPF_NN_KS": "8", "DPF_NNM_QW": "4",
               "DPF_EMD_MATRIX": "0", "DPF_TRAIN_SPLIT": "1", "DPF_TRAIN_ROLES": "0", "DPF_TRAIN_FUSE_COLSUM": "0"})
    # DPF_EMD_MATRIX is off only when its FIRST character is '0'; the setter's default is on either way
    for value, on in (("0", 0), ("0x", 0), ("00", 0), ("1", 1), ("", 1), ("false", 1), ("10", 1)):
        probe({"env": f"-1 0 -1 0 0 1 | -1 0 0 0 | {on} 1 | -1 -1 1 ; set -1 1 -1 | 1 0"}, env={"DPF_EMD_MATRIX": value})
