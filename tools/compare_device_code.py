#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds kernel by kernel.

    tools/compare_device_code.py --old OLD.o [OLD.o ...] --new NEW.o [NEW.o ...] [--out report.txt]

For a change that moves kernels between translation units or rewrites only
host code: the multiset of kernel names over all objects of either side must
be equal, and each kernel must have the same instruction text (encoding and
address comments dropped, branch targets relative to the kernel's start) and
the same resource numbers in the code-object metadata (VGPRs, AGPRs, SGPRs,
spills, private segment, LDS).  The code objects are extracted and
disassembled by tools/isa_check.py's disassemble() / kernels(); this script
only hashes and compares.  Exit status 1 on any difference.
"""
from __future__ import annotations

import argparse
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check  # noqa: E402

RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size",
             "kernarg_segment_size", "uses_dynamic_stack")
TARGET = re.compile(r"<([^>+]+)(\+0x[0-9a-f]+)?>")


def text_hash(name, body):
    """Instruction text of one function: the part before the `// addr: encoding`
    comment, and a branch's target as an offset into the function itself."""
    h = hashlib.sha256()
    # (the disassembler prints "..." for the zero fill between two functions: placement, not code)
    body = [(a, t) for a, t in body if t != "..."]
    for _, txt in body:
        ins = txt.split("//")[0].strip()
        m = TARGET.search(txt)
        if m:
            ins += " -> " + ("." if m.group(1) == name else m.group(1)) + (m.group(2) or "")
        h.update(ins.encode() + b"\n")
    return h.hexdigest()[:16], len(body)


def metadata(co):
    """{kernel symbol: {resource: value}} from the code object's metadata note."""
    notes = subprocess.run([f"{isa_check.LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    col, out, cur = None, {}, None
    entries = []
    for line in notes.splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        c = len(m.group(1)) + (2 if m.group(2) else 0)
        if col is None and m.group(3) == "symbol":
            col = c  # the kernel entries' own keys sit at this column; the arguments' further in
        entries.append((c, bool(m.group(2)), m.group(3), m.group(4).strip().strip("'")))
    for c, first, key, val in entries:
        if c != col:
            continue
        if first:
            cur = {}
        if cur is None:
            continue
        cur[key] = val
        if key == "symbol":
            out[val[:-3] if val.endswith(".kd") else val] = cur
    return out


def side(objs):
    """{function name: [(text hash, instructions, resources or None, object)]} over the objects."""
    fn = collections.defaultdict(list)
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            dis = isa_check.disassemble(obj, tmp)
            if not dis:
                continue
            md = metadata(os.path.join(tmp, "dev.co"))
            for name, _, body in isa_check.kernels(dis):
                res = md.get(name)
                fn[name].append((*text_hash(name, body), res and tuple(res.get(r, "") for r in RESOURCES),
                                 os.path.basename(obj)))
    return fn


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    old, new = side(a.old), side(a.new)
    lines, bad = [], 0
    names = sorted(set(old) | set(new))
    kernels = [n for n in names if any(e[2] is not None for e in old.get(n, []) + new.get(n, []))]
    same = 0
    for n in names:
        o, w = old.get(n, []), new.get(n, [])
        if len(o) != len(w):
            bad += 1
            lines.append(f"COUNT   {n}: {len(o)} old ({[e[3] for e in o]}), {len(w)} new ({[e[3] for e in w]})")
            continue
        # a name defined in several objects (weak template instantiations): compare as multisets
        key = lambda e: (e[0], e[1], e[2] or ())  # (a function that is no kernel has no resources)
        if sorted(map(key, o)) == sorted(map(key, w)):
            same += 1
            continue
        bad += 1
        for eo, ew in zip(sorted(o, key=key), sorted(w, key=key)):
            if eo[:2] != ew[:2]:
                lines.append(f"TEXT    {n}: {eo[1]} instructions {eo[0]} ({eo[3]}) -> {ew[1]} {ew[0]} ({ew[3]})")
            if eo[2] != ew[2]:
                moved = [f"{r} {a} -> {b}" for r, a, b in zip(RESOURCES, eo[2] or (), ew[2] or ()) if a != b]
                lines.append(f"RESOURCE {n}: {', '.join(moved)}")
    head = [f"old objects: {' '.join(os.path.basename(x) for x in a.old)}",
            f"new objects: {' '.join(os.path.basename(x) for x in a.new)}",
            f"functions in the device code: {len(names)} names ({sum(len(v) for v in old.values())} old, "
            f"{sum(len(v) for v in new.values())} new definitions), of them kernels: {len(kernels)}",
            f"identical (instruction text and resource numbers {', '.join(RESOURCES)}): {same} of {len(names)}",
            f"exceptions: {bad}"]
    report = "\n".join(head + lines) + "\n"
    sys.stdout.write(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(report)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
