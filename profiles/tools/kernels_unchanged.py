#!/usr/bin/env python3
"""Per kernel: is the body in `new` the body in `old`, block numbers and comments aside?"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            line = re.sub(r";.*", "", line).rstrip()
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            if line.strip():
                body.append(line)
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
same = differ = 0
for name, body in sorted(old.items()):
    if name not in new:
        print("MISSING", name)
        differ += 1
    elif new[name] != body:
        print("DIFFERS", name, len(body), len(new[name]))
        differ += 1
    else:
        same += 1
print("same", same, "differ", differ, "only in new", sorted(set(new) - set(old)))
