"""ISA gate of the eval FiLM conditioner (csrc/flow.hip: film_kernel): in the instantiations that promise ONE global round trip
(film_kernel<NB, true, C>) every global load must stand in front of the first wait on the vector-memory counter, and nothing
may spill.  The property rests on how the compiler places loads, so it is checked on the assembly of every build.
    python3 tools/film_loads_check.py flow.s"""
import re
import sys

text = open(sys.argv[1]).read().split("\n")
bad = seen = 0
for i, line in enumerate(text):
    m = re.match(r"^(_ZN\S*film_kernelILi\d+ELb1ELi\d+E\S*):", line)
    if not m:
        continue
    seen += 1
    before = after = scratch = 0
    waited = False
    for ins in text[i + 1:]:
        ins = ins.strip()
        if ins.startswith(".Lfunc_end"):
            break
        op = ins.split()[0] if ins.split() else ""
        if op == "s_waitcnt" and "vmcnt" in ins:
            waited = True
        elif op.startswith("global_load"):
            before, after = before + (not waited), after + waited
        elif op.startswith("scratch_"):
            scratch += 1
    print("%s: %s: %d global loads in front of the first vmcnt wait, %d behind it, %d scratch instructions" % (sys.argv[1], m.group(1), before, after, scratch))
    bad += (after > 0) + (scratch > 0) + (before == 0)
if seen != 6:
    print("%s: expected the 6 one-round-trip instantiations of film_kernel, found %d" % (sys.argv[1], seen))
    bad += 1
sys.exit(1 if bad else 0)
