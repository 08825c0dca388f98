#!/usr/bin/env python
"""Operand-delivery instructions of one loop of a kernel in a hipcc -S
listing, chosen by its rank in size (0: the largest; in a step kernel the
substep loop is rank 0 and the PGS iteration pair rank 1): VALU in all,
v_accvgpr_read/write, v_mov, every ds_* opcode by name (so the reads by
width), s_nop, s_waitcnt.  Static counts: every gated block is counted once.

    python scripts/isa_loop_ops.py <unit.s> [kernel label prefix] [rank]"""
import collections
import json
import re
import sys

path = sys.argv[1]
kernel = sys.argv[2] if len(sys.argv) > 2 else None
lines, on = [], kernel is None
for line in open(path):
    if kernel and line.startswith(kernel):
        on = True
    if on:
        if line.startswith(".Lfunc_end") and kernel:
            break
        lines.append(line)
labels, instrs = {}, []
for line in lines:
    m = re.match(r"^(\.LBB\w+):", line)
    if m:
        labels[m.group(1)] = len(instrs)
        continue
    t = line.strip().split()
    if t and not t[0].startswith((";", ".")) and not t[0].endswith(":"):
        instrs.append(t)
loops = []
for i, t in enumerate(instrs):
    if t[0].startswith(("s_cbranch", "s_branch")) and len(t) > 1 and t[1] in labels and labels[t[1]] <= i:
        loops.append((i + 1 - labels[t[1]], labels[t[1]], i + 1))
loops.sort(reverse=True)
n, a, b = loops[int(sys.argv[3]) if len(sys.argv) > 3 else 0]
ops = collections.Counter(t[0] for t in instrs[a:b])
out = {"loop_instructions": n,
       "valu": sum(v for k, v in ops.items() if k.startswith("v_") and not k.startswith("v_accvgpr")),
       "v_pk": sum(v for k, v in ops.items() if k.startswith("v_pk_")),
       "v_accvgpr_read": ops.get("v_accvgpr_read_b32", 0), "v_accvgpr_write": ops.get("v_accvgpr_write_b32", 0),
       "v_readlane_writelane": sum(v for k, v in ops.items() if k.startswith(("v_readlane", "v_writelane"))),
       "v_mov": sum(v for k, v in ops.items() if k.startswith("v_mov")),
       "s_nop": ops.get("s_nop", 0), "s_waitcnt": ops.get("s_waitcnt", 0),
       "ds": {k: v for k, v in sorted(ops.items()) if k.startswith("ds_")}}
print(json.dumps(out))
