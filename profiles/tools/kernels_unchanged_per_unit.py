#!/usr/bin/env python3
"""kernels_unchanged.py for every unit of two builds, one line per unit, with the resources of each kernel.

usage: kernels_unchanged_per_unit.py OLD NEW   (directories that hold <unit>.s, the device assembly of a unit: hipcc's
-save-temps=obj output or --cuda-device-only -S, compiled with the Makefile's flags for that unit)

Per unit: the verdict of kernels_unchanged.py, then whether the resources that the compiler states behind every kernel of
the assembly (the `; Kernel info:` block: SGPRs, VGPRs, AGPRs, scratch, LDS, occupancy - what
-Rpass-analysis=kernel-resource-usage prints as remarks) are equal, over the kernels that both builds have."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and name and m.group(1) in KEYS:
            out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return out


old_dir, new_dir = sys.argv[1], sys.argv[2]
units = sorted(name[:-2] for name in os.listdir(new_dir) if name.endswith(".s"))
for unit in units:
    old, new = os.path.join(old_dir, unit + ".s"), os.path.join(new_dir, unit + ".s")
    if not os.path.exists(old):
        print("%s: only in new (%d kernels)" % (unit, len(resources(new))))
        continue
    lines = subprocess.run([sys.executable, os.path.join(HERE, "kernels_unchanged.py"), old, new], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    a, b = resources(old), resources(new)
    shared = sorted(set(a) & set(b))
    unequal = [name for name in shared if a[name] != b[name]]
    remarks = "resources equal (%d kernels)" % len(shared) if not unequal else "RESOURCES DIFFER: " + " ".join(unequal)
    print("%s: %s ; %s" % (unit, lines[-1], remarks))
    for line in lines[:-1]:
        print("    " + line)
