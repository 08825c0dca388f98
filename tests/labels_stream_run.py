"""The policy's labels and losses on a side stream (tests/test_gpu_labels.py), run
as a program in a process of its own, so that the side stream does not stay
live in the test process (tests/test_gpu_streams.py counts its own).

The inputs of every call are written by work queued on the same stream just
before it, behind a delay that keeps the stream busy while the host enqueues:
a call that ran anywhere else would read the zeros the buffers held before.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "panda-lang-manip_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
B, N, NC = 3, 1500, 4


def run(sim, staged, stream=None):
    """label_cloud -> a perfect head -> policy_loss and decode_waypoints, all on
    `stream` (the current one if None); the inputs are copied into zeroed
    buffers on that stream first."""
    bufs = [torch.zeros_like(t) for t in staged]
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if stream is not None and hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(20_000_000)
        for b, t in zip(bufs, staged):
            b.copy_(t)
        points, waypoints, quats = bufs
        lab = sim.label_cloud(points, waypoints, quats)
        head = torch.zeros(B, N, NC + 14, device=DEV)
        head.scatter_(2, lab.cls.long().unsqueeze(-1), 10.0)
        head[..., NC:] = lab.target
        loss = sim.policy_loss(head, lab.cls, lab.target, NC, return_confusion=True)
        dec = sim.decode_waypoints(head, lab.xyz, NC, lab.centroid, lab.scale)
        out = [lab.cls, lab.target, lab.xyz, lab.centroid, lab.scale, loss.sums, loss.counts, loss.confusion,
               loss.cls_loss, dec.waypoints, dec.quats, dec.counts]
        out = [t.clone() for t in out]
    torch.cuda.synchronize()
    return out


def main():
    from pandasim.sim import PandaSim

    rng = np.random.default_rng(21)
    points = rng.uniform([-0.3, -0.3, 0.0], [0.3, 0.3, 0.2], (B, N, 3)).astype(np.float32)
    waypoints = rng.uniform([-0.1, -0.1, 0.02], [0.1, 0.1, 0.15], (B, 2, 3)).astype(np.float32)
    quats = rng.normal(size=(B, 2, 4)).astype(np.float32)
    staged = [torch.from_numpy(a).to(DEV) for a in (points, waypoints, quats)]
    sim = PandaSim("reach", num_envs=B, device=DEV)
    base = run(sim, staged)
    side = run(sim, staged, torch.cuda.Stream())
    assert int(base[6][:, 1].min()) > 0 and int(base[6][:, 2].min()) > 0, "both sets are populated"
    names = ("cls", "target", "xyz", "centroid", "scale", "sums", "counts", "confusion", "cls_loss", "waypoints",
             "quats", "decoded counts")
    for name, x, y in zip(names, base, side):
        assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), name
    print("side stream == default stream")


if __name__ == "__main__":
    main()
