"""The no-scratch rule of tools/mfma_overlap_check.py (--no-scratch PREFIX) as a command of its own, for an object's CHECK_<name>
line in csrc/Makefile: fails if a kernel whose name contains PREFIX touches scratch memory -- and if the listing holds no such
kernel at all, so that a renamed kernel cannot leave the rule without a subject.
    python3 tools/no_scratch_check.py PREFIX file.s"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mfma_overlap_check                                                                    # noqa: E402


def main(argv):
    prefix, path = argv
    kernels = [m.group(1) for m in (re.match(r"^(\S+):\s", line) for line in open(path)) if m and not m.group(1).startswith(".") and prefix in m.group(1)]
    bad = mfma_overlap_check.scan(path, no_scratch=prefix)[2]
    print("%s: %d kernels named *%s*, %s" % (path, len(kernels), prefix, "scratch instructions among them" if bad else "no scratch instruction"))
    for k, l in bad:
        print("   %s: %s" % (k[:60], l))
    if not kernels:
        print("   no kernel of that name: nothing was checked")
    return 1 if bad or not kernels else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
