#!/usr/bin/env python3
"""Development aid: are the kernels of two hipcc --save-temps assembly files the same instructions?  Per kernel the
instruction lines are compared in order - comments, directives and block labels' numbers apart - and the kernels are matched
by their mangled names with the template parameter pack of mode D's kernels (`J...E`, and the pack in the argument list)
taken out where it is empty or one Terms, so that a file from before the pack existed compares with one from after; a kernel
of any other pack (TermsObjective) keeps its name and is counted among the new file's only.  Prints what differs and how many
kernels are identical; exit status 1 unless every kernel of OLD is in NEW and identical.  The particle filter's kernels
(csrc/acmpc_pf*.hip) take argument structs that were in the one unit's anonymous namespace and are in acmpc::pf since its
split: that namespace is taken out of their names likewise.

usage: hipcc <the library's flags + the unit's own> -c csrc/acmpc_dynamic.hip -o unit.o --save-temps     (at both commits, in two
       directories; mode D: each of the five csrc/acmpc_dynamic*.hip against its own counterpart)
       python3 tools/asm_same.py OLD/acmpc_dynamic-hip-amdgcn-amd-amdhsa-gfx950.s NEW/acmpc_dynamic-hip-amdgcn-amd-amdhsa-gfx950.s
       python3 tools/asm_same.py OLD/unit.s NEW/part_a.s NEW/part_b.s ...     (a unit split into several, ONE flag set: the same
                                                                               mangled name under other flags is another kernel)"""
import difflib
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = []
        for line in m.group(2).split("\n"):
            line = re.sub(r";.*", "", line).strip()
            if line.startswith(".LBB"):
                body.append(re.sub(r"\d+_", "N_", line))
            elif line and not line.startswith("."):
                body.append(re.sub(r"\.LBB\d+_", ".LBBN_", line))
        name = re.sub(r"DpK?T\d*_", "", re.sub(r"J(?:NS_5TermsE)?E(E+v)", r"\1", m.group(1)))
        if "N5acmpc2pf" in name:   # the particle filter's argument structs: acmpc::pf::GridArgs was (anonymous namespace)::GridArgs
            name = name.replace("N5acmpc2pf", "NS_").replace("NS1_", "NS_")
        out[name] = body
    return out


def main():
    old, new = kernels(sys.argv[1]), {}
    same = 0
    for path in sys.argv[2:]:   # one unit split into several: the kernels of all NEW files together
        for name, body in kernels(path).items():
            if new.setdefault(name, body) != body:
                print("TWICE, and not the same, among the new files:", name)
                same -= 1
    for name, body in old.items():
        if name not in new:
            print("MISSING", name)
        elif body == new[name]:
            same += 1
        else:
            delta = [l for l in difflib.unified_diff(body, new[name], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
            print("DIFFERENT %s: %d lines against %d, %d differ" % (name, len(body), len(new[name]), len(delta)))
            print("\n".join("    " + l for l in delta[:12]))
    print("%d of %d kernels identical (%d in the new file%s)" % (same, len(old), len(new), "s" if len(sys.argv) > 3 else ""))
    return 0 if same == len(old) else 1


if __name__ == "__main__":
    sys.exit(main())
