#!/usr/bin/env python
"""Why the teacher-forced release of tests/test_motion_cpu.py uses a small
width: per scene, 40 envs from the schedule's resets run the first 8 control
steps of release(1), of grasp and of release(RELEASE_TF_WIDTH) in the fp64
oracle alone; per control step it prints how many envs leave
parity_judge.TOL when the step is repeated with one fp32 ulp of state noise,
and the last env's finger width after the step.  No GPU needed.

usage: python scripts/motion_release_probe.py > profiles/motion_release_probe.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "panda-lang-manip_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import oracle as O  # noqa: E402
import test_motion_cpu as T  # noqa: E402

N_ENVS, N_STEPS = 40, 8


def main():
    print(f"envs leaving TOL under 1 ulp of state noise, of {N_ENVS}, per control step 1..{N_STEPS}; "
          "then the width after each step (last env)")
    for task in T.SCENES:
        cfg = O.config(task, control="ee")
        envs = []
        for i in range(N_ENVS):
            e = O.new_env(cfg)
            O.reset(cfg, e, seed=T.SCHED_SEED + i)
            envs.append(e)
        for phase, blocked, w in (("release(1)", False, 1.0), ("grasp", True, 1.0),
                                  (f"release({T.RELEASE_TF_WIDTH})", False, T.RELEASE_TF_WIDTH)):
            per, wid = [0] * N_STEPS, [0.0] * N_STEPS
            for i, e in enumerate(envs):
                plan = T.oracle_plan_hold(w)
                for s in range(1, N_STEPS + 1):
                    per[s - 1] += T._outside(cfg, task, e, plan, s, blocked, 1 + i)
                    wid[s - 1] = e.q[7] + e.q[8]
            print(f"{task:15s} {phase:14s} {per} {[round(x, 4) for x in wid]}")


if __name__ == "__main__":
    main()
