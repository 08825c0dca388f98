#!/usr/bin/env python
"""Device assembly of every compile unit of build.UNITS, for comparing two
source trees (no GPU): each unit's exact compile line with
--offload-device-only -S, written to <out_dir>/<unit>.s.

    python scripts/device_asm.py <csrc dir> <out dir>

Point it at the csrc of two checkouts and compare the directories with
`diff -r -I __hip_cuid_ a b`: __hip_cuid_ is a per-unit hash of the source
text and differs after any edit.  Identical files mean identical registers,
scratch, LDS and instructions.  It only writes files."""
import concurrent.futures as cf
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))
from pandasim import build as B  # noqa: E402


def main(csrc, out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(out_dir, exist_ok=True)

    def asm(unit):
        name, src, defs = unit
        cmd = [hipcc, *B.FLAGS, *defs, "--offload-device-only", "-S",
               "-o", os.path.join(out_dir, name + ".s"), os.path.join(csrc, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return name, r.returncode, r.stderr

    failed = 0
    with cf.ThreadPoolExecutor(B._jobs()) as ex:
        for name, rc, err in ex.map(asm, B.UNITS):
            print(name, "ok" if rc == 0 else "failed:\n" + err[-2000:], flush=True)
            failed += rc != 0
    return 1 if failed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
