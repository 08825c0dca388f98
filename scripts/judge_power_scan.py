#!/usr/bin/env python
"""Power of the parity classifier on the CPU: the class
counts of the GPU tests' teacher-forced workloads when the "GPU" is the oracle
in fp32-like arithmetic with a deliberate model error (tests/judge_power.py),
and the smallest error of each kind that still yields 'beyond' samples.

  python scripts/judge_power_scan.py > profiles/r05_judge_power.jsonl

What the resting-stack escape of the GPU tests' verdict costs
(parity_judge.at_pgs_resolution): the smallest error of cube 2's mass and of
the cube-cube friction at which the whole verdict of Stack stack_push
(parity_judge.contact_workload_failures) still fails, bisected once with the
escape and once with no beyond sample excused.

  python scripts/judge_power_scan.py verdict > profiles/judge_verdict_thresholds.log
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import judge_power as J  # noqa: E402

CASES = [
    # (task, control, workload, mutations)
    ("reach", "ee", "random", ["none", "motor_kp_x1.01", "link_damping_0.045"]),
    ("push", "ee", "push", ["link_damping_0.045"]),
    ("reach", "joints", "random", ["none", "motor_kp_x1.01", "link_damping_0.045"]),
    ("push", "ee", "random", ["none", "motor_kp_x1.01", "link_damping_0.045", "cube_mass_x1.02",
                              "cube_friction_0.51", "finger_box_+0.5mm"]),
    ("pick_and_place", "ee", "random", ["none", "motor_kp_x1.01", "link_damping_0.045", "finger_box_+0.5mm"]),
    ("push", "ee", "push", ["none", "cube_mass_x1.02", "cube_friction_0.51", "finger_box_+0.5mm"]),
    ("pick_and_place", "ee", "push", ["none", "cube_mass_x1.02", "cube_friction_0.51", "finger_box_+0.5mm"]),
    ("slide", "ee", "push", ["none", "cube_mass_x1.02", "cube_friction_0.51", "finger_box_+0.5mm"]),
]

# effect-size ladders: the smallest value of each kind with beyond samples
LADDERS = [
    ("push", "ee", "random", "motor_kp_scale", [1.0003, 1.001, 1.003]),
    ("reach", "ee", "random", "link_damping", [0.08, 0.2, 0.5]),
    ("push", "ee", "push", "link_damping", [0.045, 0.06, 0.1, 0.2]),
    ("push", "ee", "push", "object_mass", [1.001, 1.003, 1.01]),
    ("push", "ee", "push", "object_friction", [1.001, 1.003, 1.01]),
    ("push", "ee", "push", "finger_box_grow", [0.00002, 0.00005, 0.0001, 0.0002]),
]


def run(task, control, workload, name, B):
    t = time.time()
    counts, worst, effect, visible = J.classify_workload(task, control, workload, name, B=B)
    rec = {"task": task, "control": control, "workload": workload, "mutation": name, "envs": B, "counts": counts,
           "worst_not_tight": {k: float(f"{v:.3g}") for k, v in worst.items()},
           "mutation_effect_fp64": {k: float(f"{v:.3g}") for k, v in effect.items()},
           "samples_effect_beyond_tight": visible, "seconds": round(time.time() - t, 1)}
    print(json.dumps(rec), flush=True)
    return counts


VERDICT_KINDS = {"cube2_mass": lambda f: ("config", "object2_mass", f),
                 "pair_friction": lambda f: ("pair_friction_scale", f)}


def verdict_thresholds(kind, B, lo=1e-4, hi=2e-2, rounds=7):
    """Bisects, in log(factor - 1) between `lo` (the verdict must pass) and
    `hi` (it must fail), the error at which the verdict of Stack stack_push
    stops failing: with the escape, and with none excused.  Both bisections
    share the stand-in runs.  The verdict need not be monotonic in the error;
    every run is printed."""
    runs = {}

    def fails(eps, escape):
        if eps not in runs:
            t = time.time()
            r = J.judge_workload("stack", "ee", "stack_push", VERDICT_KINDS[kind](1.0 + eps), B=B)
            runs[eps] = (r, round(time.time() - t, 1))
        r, secs = runs[eps]
        excuse = J.at_pgs_resolution if escape else (lambda task, errs, rest: False)
        f, excused, unexcused = J.workload_verdict("stack", r, excuse=excuse)
        print(json.dumps({"kind": kind, "factor": round(1.0 + eps, 7), "escape": escape, "envs": B, "counts": r["counts"],
                          "excused": len(excused), "unexcused": len(unexcused), "past_loose": len(r["past_loose"]),
                          "fired": [x.split(":")[0] for x in f], "seconds": secs}), flush=True)
        return bool(f)

    out = {}
    for escape in (True, False):
        a, b = lo, hi
        assert not fails(a, escape) and fails(b, escape), (kind, escape)
        for _ in range(rounds):
            m = math.exp(0.5 * (math.log(a) + math.log(b)))
            a, b = (a, m) if fails(m, escape) else (m, b)
        out[escape] = (a, b)
        print(json.dumps({"kind": kind, "escape": escape, "verdict_passes_at_factor": round(1.0 + a, 7),
                          "verdict_fails_at_factor": round(1.0 + b, 7)}), flush=True)
    return out


def main():
    B = int(os.environ.get("JUDGE_POWER_ENVS", "64"))
    if sys.argv[1:2] == ["verdict"]:
        for kind in sys.argv[2:] or list(VERDICT_KINDS):
            verdict_thresholds(kind, B)
        return
    for task, control, workload, muts in CASES:
        for m in muts:
            run(task, control, workload, m, B)
    for task, control, workload, kind, values in LADDERS:
        for v in values:
            if kind in ("object_mass", "object_friction"):
                J.MUTATIONS[f"{kind}_x{v}"] = ("config", kind, v)
            else:
                J.MUTATIONS[f"{kind}_{v}"] = (kind, v)
            name = f"{kind}_x{v}" if kind in ("object_mass", "object_friction") else f"{kind}_{v}"
            run(task, control, workload, name, B)


if __name__ == "__main__":
    main()
