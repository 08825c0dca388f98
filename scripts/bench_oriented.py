#!/usr/bin/env python
"""Cost of the target orientation in the fused step: PandaVecEnv.step with
`orientation` given (ps_step_oriented) against the plain step (ps_step), in
one process, timed with device events.

Per workload both variants are warmed up, then timed in alternating windows
of --steps steps each (--rounds windows per variant, the same seeded actions
for both); the line reports each variant's median and spread of the window
means and the ratio of the medians.  The orientations are a device tensor of
per-env quaternions (the standard one tilted by up to 15 degrees per axis), so
the timed path holds no conversion.

usage: python scripts/bench_oriented.py [--steps 200] [--rounds 7] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

WORKLOADS = [("PandaPush-v3", 65536, 1), ("PandaReach-v3", 4096, 16)]


def window(env, actions, orn, steps, torch):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(steps):
        if orn is None:
            env.step(actions[k % len(actions)], copy=False)
        else:
            env.step(actions[k % len(actions)], copy=False, orientation=orn)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps  # ms per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import pandasim

    if not torch.cuda.is_available():
        raise SystemExit("bench_oriented: needs a GPU (no CPU fallback)")
    lines = []
    for env_id, B, lanes in WORKLOADS:
        env = pandasim.make(env_id, num_envs=B, lanes_per_env=lanes)
        assert env.lanes_per_env == lanes
        env.reset(seed=1)
        g = torch.Generator(device="cuda")
        g.manual_seed(2)
        actions = [torch.rand(B, env.action_dim, device="cuda", generator=g) * 2 - 1 for _ in range(16)]
        euler = torch.tensor([-180.0, 0.0, 0.0], device="cuda") + (torch.rand(B, 3, device="cuda", generator=g) * 30 - 15)
        orn = env.sim.euler_xyz_to_quat(euler).contiguous()
        for o in (None, orn):
            window(env, actions, o, args.warmup, torch)
        times = {"plain": [], "oriented": []}
        for _ in range(args.rounds):
            times["plain"].append(window(env, actions, None, args.steps, torch))
            times["oriented"].append(window(env, actions, orn, args.steps, torch))
        med = {k: statistics.median(v) for k, v in times.items()}
        line = {"env_id": env_id, "num_envs": B, "lanes_per_env": lanes, "steps_per_window": args.steps,
                "windows": args.rounds,
                "plain_ms_per_step": {"median": med["plain"], "min": min(times["plain"]), "max": max(times["plain"])},
                "oriented_ms_per_step": {"median": med["oriented"], "min": min(times["oriented"]),
                                         "max": max(times["oriented"])},
                "oriented_over_plain": med["oriented"] / med["plain"],
                "plain_env_steps_per_s": B / med["plain"] * 1e3,
                "oriented_env_steps_per_s": B / med["oriented"] * 1e3}
        print(json.dumps(line), flush=True)
        lines.append(line)
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
