#!/usr/bin/env python
"""The policy's demonstration labels and losses (PandaSim.label_cloud on a
given normalisation, PandaSim.policy_loss) at the reference's shape: 256 clouds
of 5 000 points, nc = 4, head rows of ld = 18, each beside the same steps
written in torch ops on the same GPU.

labels   ps_cloud_waypoint_labels alone (the normalisation is handed over, as
         evaluate_policy hands segment_cloud's) against torch: two squared
         distances, two masks, the class, the normalised waypoints, the masked
         offsets and quaternions, one torch.cat.
loss     ps_cloud_policy_loss with the means of policy_loss against torch:
         log_softmax in f64, the gather of the true class, the masked L1 sums,
         argmax and its comparison, per cloud (no confusion matrix on either
         side).

Per entry: ms as the median of --rounds rounds of --reps back-to-back calls
between two device events (per call), after --warmup rounds; the fastest and
slowest round; the peak of torch.cuda.max_memory_allocated above what was
allocated before the call; and the achieved bytes/s against the bytes the
algorithm needs (84 B per point for the labels: 24 read, 60 written; 132 B per
point for the loss: a head row of 72, a target row of 56, the class of 4).
Prints one JSON line; --out writes it to a file.

usage: python scripts/bench_labels.py [--batch 256] [--points 5000] [--rounds 7] [--warmup 2] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

NC, LD, RADIUS = 4, 18, 0.125
LABEL_BYTES, LOSS_BYTES = 84, 132


def timed(fn, rounds, warmup, reps, nbytes):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            keep = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
        del keep
    med = statistics.median(ms)
    return {"ms": round(med, 4), "spread_ms": [round(min(ms), 4), round(max(ms), 4)], "peak_bytes": int(peak),
            "algorithmic_GBps": round(nbytes / (med * 1e-3) / 1e9, 1)}


def torch_labels(points, xyz, centroid, scale, waypoints, quats, r2):
    import torch

    d = points[:, :, None, :] - waypoints[:, None, :, :]          # [B, N, 2, 3]
    inside = (d * d).sum(-1) <= r2                                 # [B, N, 2]
    cls = (inside[..., 0].to(torch.int32) + 2 * inside[..., 1].to(torch.int32))
    wn = (waypoints - centroid[:, None, :]) / scale[:, None, None]
    off = torch.where(inside[..., None], xyz[:, :, None, :] - wn[:, None, :, :], torch.zeros((), device=xyz.device))
    rot = torch.where(inside[..., None], quats[:, None, :, :].expand(-1, xyz.shape[1], -1, -1),
                      torch.zeros((), device=xyz.device))
    return cls, torch.cat([off.flatten(2), rot.flatten(2)], -1)


def torch_loss(head, cls, target):
    import torch

    valid = cls >= 0
    true = cls.clamp(min=0).long()
    logp = torch.log_softmax(head[..., :NC].double(), -1)
    nll = torch.where(valid, -logp.gather(-1, true[..., None])[..., 0], torch.zeros((), dtype=torch.float64,
                                                                                    device=head.device)).sum(1)
    in0 = valid & ((true == 1) | (true == 3))
    in1 = valid & ((true == 2) | (true == 3))
    diff = (head[..., NC:NC + 14].double() - target.double()).abs()
    sums = torch.stack([nll, (diff[..., 0:3].sum(-1) * in0).sum(1), (diff[..., 3:6].sum(-1) * in1).sum(1),
                        (diff[..., 6:10].sum(-1) * in0).sum(1), (diff[..., 10:14].sum(-1) * in1).sum(1)], 1)
    right = valid & (head[..., :NC].argmax(-1) == true)
    counts = torch.stack([valid.sum(1), in0.sum(1), in1.sum(1), right.sum(1)], 1)
    s, c = sums.sum(0), counts.sum(0).double()
    return sums, counts, s[0] / c[0], (s[1] + s[2]) / (3 * (c[1] + c[2])), (s[3] + s[4]) / (4 * (c[1] + c[2])), c[3] / c[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from pandasim.sim import PandaSim

    B, N, dev = a.batch, a.points, "cuda:0"
    sim = PandaSim("reach", num_envs=B, device=dev)
    g = torch.Generator(device="cpu")
    g.manual_seed(1)
    lo, hi = torch.tensor([-0.3, -0.3, 0.0]), torch.tensor([0.3, 0.3, 0.2])
    points = (torch.rand(B, N, 3, generator=g) * (hi - lo) + lo).to(dev)
    waypoints = (torch.rand(B, 2, 3, generator=g) * 0.2 - 0.1 + torch.tensor([0.0, 0.0, 0.1])).to(dev)
    quats = torch.randn(B, 2, 4, generator=g).to(dev)
    first = sim.label_cloud(points, waypoints, quats, RADIUS)

    class Group:
        xyz, centroid, scale = first.xyz, first.centroid, first.scale

    head = torch.randn(B, N, LD, generator=g).to(dev)
    r2 = float(np.float32(RADIUS) * np.float32(RADIUS))
    out = {"shape": {"B": B, "N": N, "nc": NC, "ld": LD}, "rounds": a.rounds, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0),
           "algorithmic_bytes": {"labels": LABEL_BYTES * B * N, "loss": LOSS_BYTES * B * N}}
    out["labels"] = {
        "hip": timed(lambda: sim.label_cloud(points, waypoints, quats, RADIUS, group=Group), a.rounds, a.warmup, a.reps,
                     LABEL_BYTES * B * N),
        "torch": timed(lambda: torch_labels(points, first.xyz, first.centroid, first.scale, waypoints, quats, r2),
                       a.rounds, a.warmup, a.reps, LABEL_BYTES * B * N)}
    out["loss"] = {
        "hip": timed(lambda: sim.policy_loss(head, first.cls, first.target, NC), a.rounds, a.warmup, a.reps,
                     LOSS_BYTES * B * N),
        "torch": timed(lambda: torch_loss(head, first.cls, first.target), a.rounds, a.warmup, a.reps,
                       LOSS_BYTES * B * N)}
    # the two sides compute the same thing
    t_cls, t_target = torch_labels(points, first.xyz, first.centroid, first.scale, waypoints, quats, r2)
    res, ref = sim.policy_loss(head, first.cls, first.target, NC), torch_loss(head, first.cls, first.target)
    out["agreement"] = {
        "cls_differing": int((t_cls != first.cls).sum()),
        "target_max_abs_diff": float((t_target - first.target).abs().max()),
        "counts_equal": bool(torch.equal(res.counts.long(), ref[1])),
        "sums_max_rel_diff": float(((res.sums - ref[0]).abs() / ref[0].abs().clamp(min=1e-300)).max()),
        "cls_loss": [float(res.cls_loss), float(ref[2])], "accuracy": [float(res.accuracy), float(ref[5])]}
    for k in ("labels", "loss"):
        out[k]["torch_over_hip"] = round(out[k]["torch"]["ms"] / out[k]["hip"]["ms"], 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
