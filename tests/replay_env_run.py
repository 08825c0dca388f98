"""The HER replay buffer fed by the env (tests/test_gpu_replay.py): run_env, and,
run as a program, the comparison of a run on a side stream with one on the
default stream -- in a process of its own, so that the side stream does not
stay live in the test process."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "panda-lang-manip_amd") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

DEV = "cuda:0"


def run_env(stream=None, steps=120, B=64, T=60):
    """PandaPush-v3 with auto-reset, step(copy=False) and add every step, then a
    sample; the step outputs are cloned after each add.  Everything is enqueued
    on `stream` (the current one if None), a side stream behind a delay that
    keeps it busy while the host enqueues."""
    from pandasim import HerReplay
    from pandasim.envs import PandaVecEnv

    env = PandaVecEnv("push", "sparse", "ee", B, DEV, autoreset=True)
    buf = HerReplay(env, T)
    g = torch.Generator(device="cpu")
    g.manual_seed(11)
    actions = (torch.rand(steps, B, env.action_dim, generator=g) * 2 - 1).to(DEV)
    torch.cuda.synchronize()
    trace = []
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if stream is not None and hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(20_000_000)
        obs, _ = env.reset(seed=5)
        buf.begin(obs)
        first = tuple(obs[k].clone() for k in ("observation", "achieved_goal", "desired_goal"))
        for s in range(steps):
            o, r, te, tr, info = env.step(actions[s], copy=False)
            buf.add(actions[s], o, r, te, tr, info)
            trace.append([x.clone() for x in (o["observation"], o["achieved_goal"], o["desired_goal"],
                                              info["final_observation"], info["final_achieved_goal"], r, te, tr)])
        batch = buf.sample(512)
    torch.cuda.synchronize()
    return env, buf, actions, first, trace, batch


def main():
    _, buf0, _, _, trace0, batch0 = run_env()
    _, buf1, _, _, trace1, batch1 = run_env(stream=torch.cuda.Stream())
    assert int(batch0.n_valid.item()) > 0
    n = buf0.layout.prefix_offset  # ring, cur_len and pending (the rest is the scan's workspace)
    assert torch.equal(buf1.buf[:n], buf0.buf[:n]), "ring"
    assert all(torch.equal(x, y) for a, b in zip(trace0, trace1) for x, y in zip(a, b)), "step outputs"
    assert all(torch.equal(x, y) for x, y in zip(batch0, batch1)), "batch"
    print("side stream == default stream")


if __name__ == "__main__":
    main()
