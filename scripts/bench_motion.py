#!/usr/bin/env python
"""Time of one Cartesian move: a 0.3 m move (20 control steps) on
PandaPickAndPlace, fused (ps_plan_move + one ps_motion_run) or unfused (the
composition through entry points that predate the primitives: per control step
ps_link_state, ps_inverse_kinematics, control_joints' row writes, ps_sim_step,
with the waypoint arithmetic in torch).  The unfused mode runs on any build
(PANDASIM_LIB names it), so it gives the baseline of a library without the
primitives.

Per batch size the move is warmed up, then timed --rounds times from the same
state with device events (the state copy-back is outside the timed window);
the line reports the median, min and max of the rounds and the launches per
move: the ABI calls are counted; the torch kernels are an estimate from the code,
not a count (control_joints writes 45 rows per control step, the waypoint and
finger arithmetic is about 12 ops), and the field's name says so.

usage: python scripts/bench_motion.py --mode fused|unfused [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

BATCHES = (4096, 65536)
STEPS = 20
JOINTS = [0, 1, 2, 3, 4, 5, 6, 9, 10]
FORCES = [87.0, 87.0, 87.0, 87.0, 12.0, 120.0, 120.0, 170.0, 170.0]


def fused_move(sim, plan, goal, quat):
    sim.plan_move(plan, goal, quat)
    sim.motion_run(plan, STEPS)


def unfused_move(sim, goal, quat, torch):
    start = sim.get_link_position("panda", 11)
    width = sim.get_joint_angle("panda", 9) + sim.get_joint_angle("panda", 10)
    delta = (goal - start) / STEPS
    for i in range(1, STEPS + 1):
        pos = sim.get_link_position("panda", 11)
        action = (start + delta * i - pos).clamp(-1.0, 1.0)
        target = pos + action
        target[:, 2] = target[:, 2].clamp(min=0.0)
        arm = sim.inverse_kinematics("panda", 11, target, quat)[:, :7]
        half = ((sim.get_joint_angle("panda", 9) + sim.get_joint_angle("panda", 10) + width.clamp(-1.0, 1.0)) / 2)
        sim.control_joints("panda", JOINTS, torch.cat([arm, half[:, None], half[:, None]], -1), FORCES)
        sim.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("fused", "unfused"), required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pandasim.envs import PandaVecEnv

    if not torch.cuda.is_available():
        raise SystemExit("bench_motion: needs a GPU (no CPU fallback)")
    lines = []
    for B in BATCHES:
        env = PandaVecEnv("pick_and_place", "sparse", "ee", B, "cuda", autoreset=False)
        env.reset(seed=1)
        sim = env.sim
        state0 = sim.state.clone()
        calls = {"n": 0}
        inner = sim._call

        def counted(name, *a, inner=inner):
            calls["n"] += 1
            return inner(name, *a)

        sim._call = counted
        start = sim.get_link_position("panda", 11)
        goal = (start + torch.tensor([-0.18, 0.24, 0.0], device="cuda")).contiguous()  # |.| = 0.3 m
        quat = sim.euler_xyz_to_quat(torch.tensor([-180.0, 0.0, 20.0], device="cuda").expand(B, 3)).contiguous()
        plan = sim.motion_plan() if args.mode == "fused" else None
        move = (lambda: fused_move(sim, plan, goal, quat)) if args.mode == "fused" else \
            (lambda: unfused_move(sim, goal, quat, torch))
        times = []
        for r in range(args.warmup + args.rounds):
            sim.state.copy_(state0)
            calls["n"] = 0
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            move()
            t1.record()
            t1.synchronize()
            launches = calls["n"]
            if r >= args.warmup:
                times.append(t0.elapsed_time(t1))
        if plan is not None:
            assert int(plan.num_steps.min()) == int(plan.num_steps.max()) == STEPS == int(plan.done.min())
        moved = float((sim.get_link_position("panda", 11) - start).norm(dim=1).mean())
        line = {"mode": args.mode, "library": os.path.basename(os.environ.get("PANDASIM_LIB", "libpandasim.so")),
                "env_id": "PandaPickAndPlace-v3", "num_envs": B, "control_steps": STEPS, "rounds": args.rounds,
                "ms_per_move": {"median": statistics.median(times), "min": min(times), "max": max(times)},
                "abi_launches_per_move": launches,
                "torch_kernels_per_move_estimated": 0 if args.mode == "fused" else STEPS * (45 + 12) + 4,
                "mean_ee_travel_m": moved}
        print(json.dumps(line), flush=True)
        lines.append(line)
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
