#!/usr/bin/env python3
"""Development aid: opcode histogram of every innermost loop (a label that a later branch of the same kernel jumps
back to, with no other such label in between) of one kernel in a hipcc --save-temps .s file.  With --outer: of every loop
that HAS loops inside it, less the instructions of those - a step loop whose trip now and then runs a loop of its own.
With --rotated: innermost loops as without it, those that close with an unconditional s_branch included (a loop with its
exit test at its head, such as mode D's sub-step loop inside the step loop).
usage: isa_loops.py file.s <mangled-name-substring> [--json] [--outer | --rotated]"""
import collections
import json
import re
import sys


def loops(path, needle, outer=False, rotated=False):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and needle in l and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    body = lines[start + 1:end + 1]
    where = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", l.strip())
        if m:
            where[m.group(1)] = i
    found = []
    for i, l in enumerate(body):
        t = l.strip().split()
        # (a rotated loop - exit test at its head - closes with an unconditional s_branch: the step loops that --outer is for)
        closes = t[0].startswith("s_cbranch") or ((outer or rotated) and t[0] == "s_branch") if t else False
        if len(t) == 2 and closes and t[1] in where and where[t[1]] < i:
            found.append((where[t[1]], i, t[1]))
    # (a backward branch between the flow blocks of a scalar if-chain - s_setprio by quarter of the horizon - is not a loop
    # of the arithmetic: ranges without a vector instruction do not count)
    def has_valu(f):
        return any(l.strip().startswith("v_") for l in body[f[0]:f[1] + 1])
    found = [f for f in found if has_valu(f)]
    def nested(f):
        return [o for o in found if o is not f and f[0] <= o[0] and o[1] <= f[1]]
    chosen = [f for f in found if bool(nested(f)) == outer]
    out = []
    for f in chosen:
        lo, hi, label = f
        skip = set()
        for o in nested(f):
            skip.update(range(o[0], o[1] + 1))
        ops = []
        for i in range(lo, hi + 1):
            if i in skip:
                continue
            t = body[i].strip()
            if not t or t.startswith(";") or t.startswith(".") or re.match(r"^\.?LBB\w+:", t):
                continue
            ops.append(t.split()[0])
        out.append((label, collections.Counter(ops)))
    return out


if __name__ == "__main__":
    result = loops(sys.argv[1], sys.argv[2], outer="--outer" in sys.argv, rotated="--rotated" in sys.argv)
    if "--json" in sys.argv:
        print(json.dumps({label: dict(h) for label, h in result}, indent=1))
    else:
        for label, h in result:
            valu = sum(c for o, c in h.items() if o.startswith("v_"))
            print("%s: %d instructions, %d VALU, %d LDS, %d SALU" % (
                label, sum(h.values()), valu, sum(c for o, c in h.items() if o.startswith("ds_")),
                sum(c for o, c in h.items() if o.startswith("s_"))))
            print("   " + ", ".join("%s x%d" % kv for kv in h.most_common(60)))
