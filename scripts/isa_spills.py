#!/usr/bin/env python3
"""Where one kernel's gfx950 assembly (scripts/isa_of.sh writes the .s) goes back to memory or to spill lanes for values it
could not keep in registers, per loop as scripts/isa_loops.py names them:
    scripts/isa_spills.py /tmp/isa_of.s [more.s ...]
  * scalar loads (s_load_*) and what they read from: `kernarg` if the base is the kernel-argument pointer s[0:1];
  * scratch instructions;
  * SGPR spill lanes: v_writelane stores, and v_readlane restores from the registers those stores write.
Every scalar load and scratch instruction at loop depth >= 2 is listed with its line."""
import collections
import re
import sys


def loops(path):
    """(line number, text, loop header, depth) of every instruction"""
    cur, depth = "(no loop)", {"(no loop)": 0}
    for ln, line in enumerate(open(path), 1):
        t = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):\s*;\s*(.*)$", t)
        if m:
            lab, com = m.group(1), m.group(2)
            if "Loop Header" in com and "Depth=" in com and "in Loop" not in com:
                cur = lab
                depth[cur] = int(re.search(r"Depth=(\d+)", com).group(1))
            else:
                m2 = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", com)
                if m2:
                    cur = ".L" + m2.group(1)
                    depth[cur] = int(m2.group(2))
                else:
                    cur = "(no loop)"
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        yield ln, t, cur, depth[cur]


def report(path):
    text = open(path).read()
    spill_regs = set(re.findall(r"v_writelane_b32 (v\d+),", text))
    by_depth = collections.defaultdict(collections.Counter)
    listed = []
    for ln, t, loop, d in loops(path):
        op = t.split()[0]
        if op.startswith("s_load"):
            kind = "kernarg load" if re.search(r", s\[0:1\],", t) else "scalar load"
        elif op.startswith("scratch_"):
            kind = "scratch"
        elif op.startswith("v_writelane"):
            kind = "spill store"
        elif op.startswith("v_readlane") and re.match(r"v_readlane_b32 s\d+, (v\d+),", t).group(1) in spill_regs:
            kind = "spill restore"
        else:
            continue
        by_depth[d][kind] += 1
        if d >= 2 and kind in ("kernarg load", "scalar load", "scratch"):
            listed.append("  %6d %-12s depth %d  %s" % (ln, loop, d, t))
    scratch = re.search(r"private_segment_fixed_size (\d+)", text)
    print("%s: scratch %s bytes per lane, SGPR spill registers %s" % (path, scratch.group(1) if scratch else "?", ", ".join(sorted(spill_regs)) or "none"))
    kinds = ("kernarg load", "scalar load", "scratch", "spill store", "spill restore")
    print("  %-6s" % "depth" + "".join("%15s" % k for k in kinds))
    for d in sorted(by_depth):
        print("  %-6d" % d + "".join("%15d" % by_depth[d][k] for k in kinds))
    print("  %-6s" % "all" + "".join("%15d" % sum(by_depth[d][k] for d in by_depth) for k in kinds))
    print("\n".join(listed))


for p in sys.argv[1:]:
    report(p)
