"""Per-kernel comparison of two hipcc -save-temps device .s files:  isa_diff.py A.s B.s

Prints SAME / DIFF and both instruction counts for every kernel, and exits 1 on any DIFF.  Labels, comments and
.loc / .file / .cfi / .p2align directives are ignored.  Branch targets are local label names, so a kernel that gains a
basic block differs at every later branch; the first differing lines are printed."""
import re
import sys


def kernels(path):
    lines = open(path).readlines()
    funcs = set(re.findall(r"^\s*\.type\s+(\w+),@function", "".join(lines), re.M))     # not the data objects
    out, name = {}, None
    for l in lines:
        l = re.sub(r"\s*(;|//).*", "", l).strip()
        m = re.match(r"((?:_Z|k_)\w+):$", l)      # mangled names, and the extern "C" kernels of hideseek.hip
        if m and m.group(1) in funcs:
            name = m.group(1)
            out[name] = []
        elif l.startswith(".Lfunc_end"):
            name = None
        elif name and l and not l.endswith(":") and not re.match(r"\.(loc|file|cfi\w*|p2align)\b", l):
            out[name].append(" ".join(l.split()))
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for k in sorted(set(a) | set(b)):
    x, y = a.get(k), b.get(k)
    same = x == y
    bad += not same
    print("%-4s %6s %6s  %s" % ("SAME" if same else "DIFF", "-" if x is None else len(x), "-" if y is None else len(y), k))
    if not same and x is not None and y is not None:
        i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        for p, q in list(zip(x[i:], y[i:]))[:3]:
            print("       @%d  %-50s | %s" % (i, p, q))
sys.exit(1 if bad else 0)
