#!/usr/bin/env python
"""Register, scratch and LDS use of every step, motion, render, point-cloud and replay kernel of a built object or
library, from the code objects' AMDGPU metadata (no GPU needed).

usage: python scripts/kernel_resources.py [lib or .o ...] [--json out.json]
(default: the product library's objects under pandasim/build/libpandasim/)
"""
from __future__ import annotations

import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size")


def code_objects(path: str, tmp: str) -> list:
    """Device code objects of a host object/library (clang-offload-bundler)."""
    out = os.path.join(tmp, os.path.basename(path) + ".gfx950")
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={path}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={out}"], capture_output=True)
    if r.returncode == 0 and os.path.getsize(out) > 0:
        return [out]
    # a linked library: extract the fat binary's bundles
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={out}.fatbin", path, os.devnull],
                       capture_output=True)
    if r.returncode != 0:
        return []
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={out}.fatbin",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={out}"], capture_output=True)
    return [out] if r.returncode == 0 else []


def kernels(co: str) -> dict:
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    # One record per entry of amdhsa.kernels: its keys come sorted, so a kernel's
    # .agpr_count and .group_segment_fixed_size stand before its .name.  A record
    # starts at a list item of the kernels' own indent (their .args sit deeper).
    res, rec, indent, inside = {}, None, None, False

    def close(r):
        if r and "k_" in r.get("name", ""):
            res[r.pop("name")] = r

    for line in txt.splitlines():
        if "amdhsa.kernels:" in line:
            inside, indent = True, None
            continue
        if not inside:
            continue
        m = re.match(r"(\s*)- \.", line)
        if m and (indent is None or len(m.group(1)) == indent):
            indent = len(m.group(1))
            close(rec)
            rec = {}
        elif re.match(r"\s{0,%d}\S" % (indent or 0), line) and not m:
            close(rec)  # left the kernels list
            rec, inside = None, False
            continue
        if rec is None or (len(line) - len(line.lstrip())) > (indent or 0) + 2:
            continue  # a key of an argument
        m = re.match(r"\s*(?:- )?\.name:\s+(\S+)", line)
        if m:
            rec["name"] = m.group(1)
        for f in FIELDS:
            m = re.match(r"\s*(?:- )?" + re.escape(f) + r":\s+(\d+)", line)
            if m:
                rec[f[1:]] = int(m.group(1))
    close(rec)
    return res


def demangle(name: str) -> str:
    r = subprocess.run(["c++filt", name], capture_output=True, text=True)
    return r.stdout.strip().replace("(anonymous namespace)::", "").split("(")[0]


def main(argv):
    out_json = None
    if "--json" in argv:
        i = argv.index("--json")
        out_json = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    paths = argv or sorted(glob.glob(os.path.join(ROOT, "panda-lang-manip_amd", "pandasim", "build", "libpandasim",
                                                  "step_*.o")) +
                          glob.glob(os.path.join(ROOT, "panda-lang-manip_amd", "pandasim", "build", "libpandasim",
                                                 "motion_*.o")) +
                          [os.path.join(ROOT, "panda-lang-manip_amd", "pandasim", "build", "libpandasim", n)
                           for n in ("render_kernels.o", "cloud_kernels.o", "group_kernels.o", "propagate_kernels.o", "mlp_kernels.o", "decode_kernels.o",
                                     "keypoint_kernels.o", "label_kernels.o")])
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for p in paths:
            for co in code_objects(p, tmp):
                for k, v in kernels(co).items():
                    if any(n in k for n in ("k_step", "k_sim_step", "k_motion", "k_render", "k_deproject", "k_cloud", "k_replay")):
                        table[demangle(k)] = v
    for k, v in sorted(table.items()):
        print(f"{k:40s} vgpr {v.get('vgpr_count', 0):3d} agpr {v.get('agpr_count', 0):3d} "
              f"scratch {v.get('private_segment_fixed_size', 0):4d} B  spill v {v.get('vgpr_spill_count', 0):3d} "
              f"s {v.get('sgpr_spill_count', 0):3d}  lds {v.get('group_segment_fixed_size', 0)}")
    if out_json:
        json.dump(table, open(out_json, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
