#!/usr/bin/env python3
"""Are the functions of two device listings the same code under other names?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Iinclude -S --cuda-device-only -o X.s raytracer-3_amd/csrc/rt3_device.hip
    python tools/isa_identity.py PARENT.s TREE.s [--enum Form=Render,RenderRef,Query,List,Rays] > profiles/trace_form_isa_identity.log

(the flags of tools/cvt_isa_check.py; one listing of the parent commit, one of this tree).  For a change that renames kernels and must not touch their
code — a template parameter list spelled another way.  Each listing is split into functions; in a function's instruction stream and in its .amdhsa_*
block every mangled symbol becomes a placeholder and the local labels lose the numbers that count functions (.LBB46_3 -> .LBB_3), and the two are hashed.
Functions of equal hash are paired, several of one hash in the order of their sorted names.  Prints `tree's name <- parent's name` per function
(demangled, without the parameter list, a name of more than 200 characters cut short; --enum NAME=A,B,.. spells the values of an enum template argument) and ends with the counts; exit code 1 if a
function of either side has no partner.

A side may be several listings, A.s,B.s — a unit that was split in two: their functions are taken together, and a function both listings hold (a kernel
of a header both units include) counts once per listing, as `name @B.s` from the second on.
"""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys

BEGIN = re.compile(r"^([A-Za-z_$][\w.$]*):\s*; @")
SYMBOL = re.compile(r"\b_Z[\w.$]+")
BLOCK = re.compile(r"(\.L[A-Za-z_]+?)\d+(_\d+)\b")                  # numbered per function and block: the function's number goes
OTHER = re.compile(r"\.L[A-Za-z_]+?\d+\b")                           # numbered through the file (.Lpost_getpc7): renumbered in order of appearance


def functions(path):
    """name -> hash of (instruction stream, .amdhsa_ block), symbols and label numbers normalised."""
    out, name, body, kd, in_kd = {}, None, [], collections.defaultdict(list), None
    for line in open(path, errors="replace"):
        m = BEGIN.match(line)
        if m:
            name, body = m.group(1), []
            continue
        s = line.split(";")[0].strip()
        if not s:
            continue
        if s.startswith(".amdhsa_kernel "):
            in_kd = s.split()[1]
        elif s == ".end_amdhsa_kernel":
            in_kd = None
        elif in_kd:
            kd[in_kd].append(SYMBOL.sub("SYM", s))
        elif name and s.startswith(".Lfunc_end"):
            seen = {}
            out[name] = [OTHER.sub(lambda m: ".L%d" % seen.setdefault(m.group(0), len(seen)), b) for b in body]
            name = None
        elif name and not s.startswith(".section") and not s.startswith(".p2align"):
            body.append(BLOCK.sub(r"\1\2", SYMBOL.sub("SYM", s)))
    if name:
        sys.exit("%s: function %s does not end" % (path, name))
    return {n: hashlib.sha256("\n".join(b + ["--"] + kd.get(n, [])).encode()).hexdigest() for n, b in out.items()}, set(kd)


def demangled(names, enums):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    text = subprocess.run([tool], input="\n".join(n.split(" @")[0] for n in names), capture_output=True, text=True, check=True).stdout.splitlines() if tool and names else list(names)
    out = {}
    for n, d in zip(names, text):
        d = re.sub(r"^void ", "", d.replace("(anonymous namespace)::", ""))
        if d.endswith(")"):                                          # drop the parameter list: the last balanced (...)
            depth, i = 0, len(d)
            while i > 0:
                i -= 1
                depth += (d[i] == ")") - (d[i] == "(")
                if depth == 0:
                    break
            d = d[:i]
        for enum, values in enums.items():
            d = re.sub(r"\(%s\)(\d+)" % re.escape(enum), lambda m: "%s::%s" % (enum, values[int(m.group(1))]) if int(m.group(1)) < len(values) else m.group(0), d)
        d = d if len(d) <= 200 else "%s...[%d more characters]" % (d[:160], len(d) - 160)
        out[n] = d + n[len(n.split(" @")[0]):]
    return out


def listings(paths):
    """functions() over the listings of one side, A.s,B.s,...: a name a later listing repeats becomes `name @listing`."""
    table, kernels = {}, set()
    for path in paths.split(","):
        t, k = functions(path)
        for n, h in t.items():
            key = n if n not in table else "%s @%s" % (n, os.path.basename(path))
            table[key] = h
            if n in k:
                kernels.add(key)
    return table, kernels


def main():
    args, enums = [], {}
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--enum":
            k, v = next(it).split("=")
            enums[k] = v.split(",")
        else:
            args.append(a)
    if len(args) != 2:
        sys.exit(__doc__)
    (pa, pa_k), (tr, tr_k) = listings(args[0]), listings(args[1])
    by_hash = collections.defaultdict(lambda: ([], []))
    for side, table in enumerate((pa, tr)):
        for n, h in table.items():
            by_hash[h][side].append(n)
    names = demangled(sorted(set(pa) | set(tr)), enums)
    pairs, lone_p, lone_t = [], [], []
    for old, new in by_hash.values():
        old.sort(); new.sort()
        k = min(len(old), len(new))
        pairs += zip(new[:k], old[:k])
        lone_p += old[k:]; lone_t += new[k:]
    for new, old in sorted(pairs, key=lambda p: names[p[0]]):
        print("%s <- %s%s" % (names[new], names[old] if new != old else "(the same name)", "" if new in tr_k else "   (not a kernel)"))
    for n in sorted(lone_p):
        print("UNPAIRED in the parent: %s" % names[n])
    for n in sorted(lone_t):
        print("UNPAIRED in the tree: %s" % names[n])
    print("functions: parent %d, tree %d; kernels: parent %d, tree %d; paired %d, of them renamed %d; unpaired: parent %d, tree %d"
          % (len(pa), len(tr), len(pa_k), len(tr_k), len(pairs), sum(1 for n, o in pairs if n != o), len(lone_p), len(lone_t)))
    return 1 if lone_p or lone_t else 0


if __name__ == "__main__":
    sys.exit(main())
