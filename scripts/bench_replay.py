#!/usr/bin/env python
"""Time and memory of the device-resident HER replay (pandasim.HerReplay) on
PandaPush-v3 at 65 536 envs and T = 100 slots, each part beside the same steps
written in torch ops on the same GPU:

  store   HerReplay.add per env step (one launch), beside the step's own time in
          the same run, against one indexed copy per field into field-major
          [T, B, dim] tensors, the cur_len update, and the back-fill as one
          masked torch.where over the whole [T, B] ep_end (the sync-free way to
          write a per-env, variable-length run in torch; a Python loop over
          the finished envs would need a host read of the done flags).
  sample  HerReplay.sample at M = 4 096 and 262 144 (prefix sum, search, gather,
          relabel and reward in one call) against torch.randint / rand,
          advanced-indexing gathers from the field-major tensors and
          env.compute_reward, given the ring's ep_end and cur_len.

Medians of --rounds timed rounds after --warmup, device events, with min and
max; achieved bytes per second against the algorithmic bytes (row * B per
store, row * M per sample); the buffers' bytes and the peak allocation of one
sample of each kind.

A sample's time is one whole call between two events: its three launches and
the allocation of its fourteen output tensors are inside, so at M = 4 096 the
figures are the call's latency, not the gather kernel's throughput (the keys
say "call").  The torch sampler is not the same distribution either: it draws
the env uniformly and then one of its valid slots, which leaves out the prefix
sum and the search; the ratio is against that cheaper composition.

usage: python scripts/bench_replay.py [--rounds 7] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

B, T, FILL, PER_ROUND = 65536, 100, 110, 10
BATCHES = (4096, 262144)
NAMES = ("obs", "ag", "dg", "action", "next_obs", "next_ag", "reward", "terminated", "ep_end")


def stats(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from pandasim import HerReplay
    from pandasim.envs import PandaVecEnv

    if not torch.cuda.is_available():
        raise SystemExit("bench_replay: needs a GPU (no CPU fallback)")
    dev = "cuda"
    env = PandaVecEnv("push", "sparse", "ee", B, dev, autoreset=True)
    buf = HerReplay(env, T)
    row_bytes = buf.layout.row_floats * 4
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def action():
        return torch.rand(B, env.action_dim, device=dev, generator=g) * 2 - 1

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), out

    obs, _ = env.reset(seed=1)
    buf.begin(obs)
    for _ in range(FILL):
        a = action()
        buf.add(a, *env.step(a, copy=False))
    torch.cuda.synchronize()

    # ------------------------------------------------ the torch composition's ring
    tt = {n: buf.field(n).clone() for n in NAMES}  # field-major [T, B, dim]
    tt["ep_end"], tt["terminated"] = tt["ep_end"][..., 0].contiguous(), tt["terminated"][..., 0].contiguous()
    tt["reward"] = tt["reward"][..., 0].contiguous()
    cur_len = buf.cur_len.clone()
    O, G = env.obs_dim, env.goal_dim
    pend = [buf.pending[:, :O].clone(), buf.pending[:, O:O + G].clone(), buf.pending[:, O + G:O + 2 * G].clone()]
    slots = torch.arange(T, device=dev)[:, None]
    torch_ring_bytes = sum(t.numel() * t.element_size() for t in tt.values()) + cur_len.numel() * 4 + \
        sum(p.numel() * 4 for p in pend)

    def torch_store(pos, a, o, r, te, tr, info):
        tt["obs"][pos].copy_(pend[0]); tt["ag"][pos].copy_(pend[1]); tt["dg"][pos].copy_(pend[2])  # noqa: E702
        tt["action"][pos].copy_(a)
        tt["next_obs"][pos].copy_(info["final_observation"]); tt["next_ag"][pos].copy_(info["final_achieved_goal"])  # noqa: E702
        tt["reward"][pos].copy_(r); tt["terminated"][pos].copy_(te)  # noqa: E702
        tt["ep_end"][pos].fill_(-1)
        cur_len.add_(1).clamp_(max=T)
        done = (te | tr).bool()
        age = (pos - slots) % T
        close = done[None, :] & (age < cur_len[None, :])
        tt["ep_end"].copy_(torch.where(close, pos, tt["ep_end"]))
        cur_len.masked_fill_(done, 0)
        pend[0].copy_(o["observation"]); pend[1].copy_(o["achieved_goal"]); pend[2].copy_(o["desired_goal"])  # noqa: E702

    def torch_sample(M, pos_next, stored):
        b = torch.randint(0, B, (M,), device=dev)
        v = stored - cur_len[b]
        j = (torch.rand(M, device=dev) * v).long()
        t = ((pos_next - stored) % T + j) % T
        e = tt["ep_end"][t, b].long()
        relabel = torch.rand(M, device=dev) < 0.8
        n = (e - t) % T + 1
        gs = (t + (torch.rand(M, device=dev) * n).long()) % T
        next_ag = tt["next_ag"][t, b]
        dg = torch.where(relabel[:, None], tt["next_ag"][gs, b], tt["dg"][t, b])
        r, ok = env._reward_and_success(next_ag, dg)
        reward = torch.where(relabel, r, tt["reward"][t, b])
        return (tt["obs"][t, b], tt["ag"][t, b], dg, tt["action"][t, b], tt["next_obs"][t, b], next_ag, reward,
                tt["terminated"][t, b], ok, relabel, b, t, gs)

    # ----------------------------------------------------------- step and store
    step_ms, store_ms, tstore_ms = [], [], []
    for r in range(args.warmup + args.rounds):
        acc = [0.0, 0.0, 0.0]
        for _ in range(PER_ROUND):
            a = action()
            ms, out = timed(lambda: env.step(a, copy=False))
            acc[0] += ms
            pos = buf.pos
            acc[1] += timed(lambda: buf.add(a, *out))[0]
            acc[2] += timed(lambda: torch_store(pos, a, *out))[0]
        if r >= args.warmup:
            step_ms.append(acc[0] / PER_ROUND)
            store_ms.append(acc[1] / PER_ROUND)
            tstore_ms.append(acc[2] / PER_ROUND)
    same_ring = all(torch.equal(buf.field(n).reshape(tt[n].shape), tt[n]) for n in NAMES) and \
        torch.equal(buf.cur_len, cur_len)
    store, tstore, step = stats(store_ms), stats(tstore_ms), stats(step_ms)
    result = {"env_id": "PandaPush-v3", "num_envs": B, "capacity_steps": T, "rounds": args.rounds,
              "steps_per_round": PER_ROUND, "row_bytes": row_bytes, "replay_bytes": buf.nbytes,
              "torch_ring_bytes": torch_ring_bytes,
              "step_ms": step, "store_ms": store, "torch_store_ms": tstore,
              "store_over_step": store["median"] / step["median"],
              "store_over_torch": store["median"] / tstore["median"],
              "store_algorithmic_bytes": row_bytes * B,
              "store_GBps": row_bytes * B / store["median"] / 1e6,
              "torch_store_same_ring": bool(same_ring),
              "sample_timing": "one whole call between two events (three launches and fourteen output allocations "
                               "inside): call latency at small M",
              "torch_sample_distribution": "env uniform, then one of its valid slots (no prefix sum, no search): not "
                                           "uniform over transitions, and cheaper",
              "samples": []}
    print(json.dumps({k: v for k, v in result.items() if k != "samples"}), flush=True)

    # ------------------------------------------------------------------- sample
    for M in BATCHES:
        ours, theirs = [], []
        for r in range(args.warmup + args.rounds):
            ms_a = timed(lambda: buf.sample(M))[0]
            ms_b = timed(lambda: torch_sample(M, buf.pos, buf.stored))[0]
            if r >= args.warmup:
                ours.append(ms_a)
                theirs.append(ms_b)
        peaks = {}
        for name, fn in (("kernel", lambda: buf.sample(M)), ("torch", lambda: torch_sample(M, buf.pos, buf.stored))):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del out
        a, b = stats(ours), stats(theirs)
        line = {"M": M, "sample_ms": a, "torch_sample_ms": b, "sample_over_torch": a["median"] / b["median"],
                "sample_algorithmic_bytes": row_bytes * M, "sample_call_GBps": row_bytes * M / a["median"] / 1e6,
                "transitions_per_s_of_the_call": M / a["median"] * 1e3, "peak_bytes_of_one_sample": peaks,
                "n_valid": buf.valid_count()}
        print(json.dumps(line), flush=True)
        result["samples"].append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
