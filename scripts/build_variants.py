#!/usr/bin/env python
"""Build experimental libpandasim variants (extra compiler flags) into
scripts/bin/variants/ for scripts/time_variants.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))
from pandasim import build as B  # noqa: E402

VARIANTS = {
    "base": [],
    "maxilp": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
    "bias0": ["-mllvm", "-amdgpu-schedule-metric-bias=0"],
    "unroll_off": ["-mllvm", "-amdgpu-unroll-threshold-private=0"],
    "ilp_min": ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"],
    "no_early_if": ["-mllvm", "-amdgpu-early-ifcvt=0"],
    # IEEE mode off: drops the v_max x,x,x canonicalisations before min/max
    # (68 of ~3000 instructions in the Push PGS loop); NaN handling only
    "ieee_off": ["-fno-honor-nans", "-mno-amdgpu-ieee"],
    "no_unclust": ["-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"],
    # group-kernel miscompute bisection: every object at -O1
    # (the later flag wins over the library's -O3)
    "o1": ["-O1"],
    "prealloc": ["-mllvm", "-amdgpu-prealloc-sgpr-spill-vgprs=1"],
    "nodppc": ["-mllvm", "-amdgpu-dpp-combine=0"],
    # the group solver's row dump (scripts/row_dump.py): the product's objects
    # (every one at -O3) with the dump compiled in
    "dump": ["-DPS_DEBUG_ROW_DUMP"],
}


# variants that change the per-unit flags of build.UNITS instead
def _on(pred, flags):
    return lambda units: [(n, s, defs + (flags if pred(n) else [])) for n, s, defs in units]


def _groups(n):
    return n.endswith("_groups")


def _stack(n):
    return n.startswith("step_t4_")


UNIT_VARIANTS = {
    # scheduler and register-allocator options on the group objects only
    "groups_rev": _on(_groups, ["-mllvm", "-greedy-reverse-local-assignment"]),
    "groups_maxilp": _on(_groups, ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    "groups_minreg": _on(_groups, ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
    "groups_nu": _on(_groups, ["-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]),
    # on Stack's one-lane objects only
    "stack_itermin": _on(_stack, ["-mllvm", "-amdgpu-sched-strategy=iterative-minreg"]),
    "stack_nu": _on(_stack, ["-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]),
}


def main(names):
    out_dir = os.path.join(ROOT, "scripts", "bin", "variants")
    os.makedirs(out_dir, exist_ok=True)
    product_units = list(B.UNITS)
    for n in names:
        out = os.path.join(out_dir, f"lib_{n}.so")
        B.UNITS = UNIT_VARIANTS[n](product_units) if n in UNIT_VARIANTS else product_units
        try:
            B.build(variant="", extra=VARIANTS.get(n, []), out=out, verbose=False)
            print(n, "ok")
        except Exception as e:  # a variant that does not compile is reported, not fatal
            print(n, "failed:", e)


if __name__ == "__main__":
    main(sys.argv[1:] or list(VARIANTS) + list(UNIT_VARIANTS))
