#!/usr/bin/env python3
"""Before/after table of the kernels' resource usage, from two logs of

    hipcc --offload-arch=gfx950 <the Makefile's HIPFLAGS> -Rpass-analysis=kernel-resource-usage ... 2> LOG

(one of the parent commit, one of this tree).  Kernels are matched by their demangled names (a new form of a trace kernel is a new value of Form,
rt3_kernel_common.hpp, and renames no existing kernel).  Prints one line per kernel, `a -> b` where a figure changed, NEW for kernels the parent
does not have, and ends with the number of existing kernels that gained scratch or lost occupancy (exit code 1 if there is one).

    python tools/kernel_resources.py PARENT.log TREE.log > profiles/radiance_kernel_resources.log

--brief leaves out the kernels whose figures did not change (the last line still counts them): the log of a change that adds forms and moves nothing.
"""
import re
import shutil
import subprocess
import sys

KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?Function Name: (\S+)", line)       # (the location comes before or after "remark:", by compiler version)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def demangled(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return list(names)
    return subprocess.run([tool] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()


def key(d):
    d = re.sub(r"^void ", "", re.sub(r"\(anonymous namespace\)::", "", d))
    depth = 0
    for i in range(len(d) - 1, -1, -1):                               # drop the parameter list: the last balanced (...) — an enum argument, (Form)2, stays
        depth += (d[i] == ")") - (d[i] == "(")
        if depth == 0:
            return d[:i] if d.endswith(")") else d
    return d


def table(path):
    raw = parse(path)
    return {key(d): raw[n] for n, d in zip(raw, demangled(raw))}


def main():
    brief = "--brief" in sys.argv[1:]
    paths = [x for x in sys.argv[1:] if x != "--brief"]
    a, b = table(paths[0]), table(paths[1])
    print("kernel | " + " | ".join(KEYS) + "     (parent -> this tree; one figure: unchanged)")
    worse = []
    for n in sorted(set(a) | set(b)):
        if n not in b:
            print("GONE %s" % n)
            continue
        x, y = a.get(n, b[n]), b[n]
        cells = [y.get(k, "?") if x.get(k) == y.get(k) else "%s -> %s" % (x.get(k), y.get(k)) for k in KEYS]
        tag = "" if n in a else "NEW "
        if n in a and (int(y[KEYS[3]]) > int(x[KEYS[3]]) or int(y[KEYS[4]]) < int(x[KEYS[4]])):
            worse.append(n)
            tag = "WORSE "
        if not brief or n not in a or x != y:
            print("%s%s | %s" % (tag, n, " | ".join(cells)))
    print("existing kernels: %d, new kernels: %d, existing kernels with a changed figure: %d, with new scratch or lower occupancy: %d"
          % (len(set(a) & set(b)), len(set(b) - set(a)), sum(1 for n in set(a) & set(b) if any(a[n].get(k) != b[n].get(k) for k in KEYS)), len(worse)))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
