#!/usr/bin/env python
"""Device assembly of every compile unit of build.UNITS, for comparing two
source trees (no GPU): each unit's exact compile line with
--offload-device-only -S, written to <out_dir>/<unit>.s.

    python scripts/device_asm.py [--variant prof] [-DNAME ...] <csrc dir> <out dir>
    python scripts/device_asm.py --kernels <asm dir> <out dir>

Point it at the csrc of two checkouts and compare the directories with
`diff -r -I __hip_cuid_ a b`: __hip_cuid_ is a per-unit hash of the source
text and differs after any edit.  Identical files mean identical registers,
scratch, LDS and instructions.  A unit whose source the csrc dir does not
have (a tree from before the unit existed) is skipped and named.  --variant
adds build.VARIANTS' flags, -D... any further define (the diagnostic builds).

--kernels is the per-kernel mode, for kernels that moved from one unit to
another: it splits every <asm dir>/*.s into one file per kernel, named by the
demangled kernel name (a kernel instantiated in several units gets
`@<unit>` appended), holding the function from its label to its end label,
its .amdhsa_kernel descriptor block and its metadata entry.  The same
`diff -r` then compares two trees whichever unit a kernel sits in.  One thing
is rewritten on the way: the function's ordinal within its unit, which the
compiler puts into local labels and the comments that name them
(.LBB<n>_<k>, BB<n>_<k>, .Lfunc_begin<n>, .Lfunc_end<n>, .LJTI<n>_<k>),
becomes `N` (with the blanks between such a label and its comment, whose
column moves with the label's width, made one), and .Ltmp labels are
renumbered from 0 within the kernel; nothing else of the text is touched.
It only writes files."""
import concurrent.futures as cf
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))
from pandasim import build as B  # noqa: E402


def main(csrc, out_dir, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(out_dir, exist_ok=True)

    def asm(unit):
        name, src, defs = unit
        if not os.path.exists(os.path.join(csrc, src)):
            return name, None, ""
        cmd = [hipcc, *B.FLAGS, *extra, *defs, "--offload-device-only", "-S",
               "-o", os.path.join(out_dir, name + ".s"), os.path.join(csrc, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return name, r.returncode, r.stderr

    failed = 0
    with cf.ThreadPoolExecutor(B._jobs()) as ex:
        for name, rc, err in ex.map(asm, B.UNITS):
            print(name, "skipped: no such source in this tree" if rc is None
                  else "ok" if rc == 0 else "failed:\n" + err[-2000:], flush=True)
            failed += bool(rc)
    return 1 if failed else 0


def _demangle(names):
    if not names:
        return {}
    filt = os.environ.get("CXXFILT", "c++filt")
    out = subprocess.run([filt, *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def split_kernels(text):
    """{mangled kernel name: its text} of one unit's assembly."""
    lines = text.split("\n")
    kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    # metadata entries: the items of amdhsa.kernels, each from its `  - .` line
    # to the next item or the end of the list
    meta, item = {}, None
    in_list = False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            in_list, item = True, None
            continue
        if in_list:
            if ln.startswith("  - "):
                item = []
            elif not ln.startswith("    "):
                in_list, item = False, None
                continue
            if item is not None:
                item.append(ln)
                m = re.match(r"\s+\.name:\s+(\S+)", ln)
                if m:
                    meta[m.group(1)] = item
    parts = {}
    for k in kernels:
        # label .. end label (the descriptor block sits between them), then the
        # resource symbols and the "; Kernel info" comments that follow
        a = next(i for i, ln in enumerate(lines) if ln.startswith(k + ":"))
        end = next(i for i in range(a, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        assert any(lines[i].strip() == ".end_amdhsa_kernel" for i in range(a, end)), k
        end = next(i for i in range(end, len(lines)) if lines[i].startswith("; Kernel info"))
        while end + 1 < len(lines) and lines[end + 1].startswith(";"):
            end += 1
        txt = "\n".join(lines[a:end + 1] + meta[k]) + "\n"
        txt = re.sub(r"(?<![A-Za-z0-9_])(\.LBB|\.LJTI|BB)\d+_(?=\d)", r"\1N_", txt)
        txt = re.sub(r"(?m)^(\.LBBN_\d+:) +;", r"\1 ;", txt)  # the comment column moves with the label's width
        txt = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1N", txt)
        tmps = {}
        txt = re.sub(r"\.Ltmp(\d+)", lambda m: ".Ltmp%d" % tmps.setdefault(m.group(1), len(tmps)), txt)
        parts[k] = txt
    return parts


def kernels_mode(asm_dir, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    found = []  # (demangled, unit, text)
    for f in sorted(os.listdir(asm_dir)):
        if not f.endswith(".s"):
            continue
        with open(os.path.join(asm_dir, f)) as fh:
            parts = split_kernels(fh.read())
        names = _demangle(list(parts))
        found += [(names[k], f[:-2], t) for k, t in parts.items()]
    count = {}
    for name, _, _ in found:
        count[name] = count.get(name, 0) + 1
    for name, unit, txt in found:
        fn = re.sub(r"[^A-Za-z0-9_<>,=().-]+", "_", name) + ("@" + unit if count[name] > 1 else "") + ".s"
        with open(os.path.join(out_dir, fn), "w") as fh:
            fh.write(txt)
        print(f"{unit}\t{name}", flush=True)
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--kernels":
        sys.exit(kernels_mode(os.path.abspath(args[1]), os.path.abspath(args[2])))
    extra = []
    while args and args[0].startswith("-"):
        if args[0] == "--variant" and len(args) > 1:
            extra += B.VARIANTS[args[1]]
            args = args[2:]
        elif args[0].startswith("-D"):
            extra.append(args.pop(0))
        else:
            sys.exit(__doc__)
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(os.path.abspath(args[0]), os.path.abspath(args[1]), extra))
