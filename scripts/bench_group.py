#!/usr/bin/env python
"""The PointNet++ front end (PandaSim.group_cloud, one ps_cloud_set_abstraction
call) against a torch restatement of the same four steps on the same GPU: the
first layer of model_cls_off_rot.py (512 centres, radii 0.1 / 0.2 / 0.4 with
32 / 64 / 128 samples) on B clouds of 5 000 points with 3 feature channels.

fused  normalise, farthest point sampling, the three ball queries in one walk
       over the points, the three groups: four kernels.
torch  what pointnet2_utils.py does, written here from its description:
       pc_normalize; farthest point sampling as a loop of npoint dependent
       iterations of torch ops; per radius a [B, S, N] distance matrix
       (-2ab + a^2 + b^2), an i64 index tensor of that shape, its sort, the
       padding with the first index; the index_points gathers and the centring.

Per batch size and path: ms per call as the median of --runs timed runs
(device events around one call, after a warm-up call), the fastest and slowest
run, and the peak of torch.cuda.max_memory_allocated above what was allocated
before the path ran.  A path that cannot allocate is recorded as such.  Both
start farthest point sampling from the same indices; the script also reports
whether the two paths' fps_idx agree (they need not: the torch path's
distances are not the kernels' bit for bit where torch fuses or reorders).
Prints one JSON line; --out writes it to a file.

usage: python scripts/bench_group.py [--batches 64 256] [--runs 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

NPOINT, RADII, NSAMPLES = 512, (0.1, 0.2, 0.4), (32, 64, 128)


def torch_path(points, feats, start):
    import torch

    B, N, _ = points.shape
    centroid = points.mean(1, keepdim=True)
    xyz = points - centroid
    xyz = xyz / xyz.pow(2).sum(-1).sqrt().amax(1).clamp_min(1e-30).view(B, 1, 1)
    rows = torch.arange(B, device=points.device)
    fps = torch.zeros(B, NPOINT, dtype=torch.long, device=points.device)
    distance = torch.full((B, N), 1e10, device=points.device)
    farthest = start.long()
    for i in range(NPOINT):
        fps[:, i] = farthest
        c = xyz[rows, farthest, :].view(B, 1, 3)
        dist = ((xyz - c) ** 2).sum(-1)
        distance = torch.minimum(distance, dist)
        farthest = distance.max(-1)[1]
    new_xyz = xyz[rows.view(B, 1), fps]
    grouped = []
    for radius, k in zip(RADII, NSAMPLES):
        sqr = -2 * torch.matmul(new_xyz, xyz.permute(0, 2, 1))
        sqr += (new_xyz ** 2).sum(-1).view(B, NPOINT, 1)
        sqr += (xyz ** 2).sum(-1).view(B, 1, N)
        idx = torch.arange(N, dtype=torch.long, device=points.device).view(1, 1, N).repeat(B, NPOINT, 1)
        idx[sqr > radius ** 2] = N
        idx = idx.sort(dim=-1)[0][:, :, :k]
        first = idx[:, :, 0].view(B, NPOINT, 1).repeat(1, 1, k)
        mask = idx == N
        idx[mask] = first[mask]
        del sqr, mask, first
        g_xyz = xyz[rows.view(B, 1, 1), idx] - new_xyz.view(B, NPOINT, 1, 3)
        grouped.append(torch.cat([feats[rows.view(B, 1, 1), idx], g_xyz], -1))
    return fps, grouped


def measure(fn, runs):
    import torch

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        keep = fn()  # warm-up: kernel load, allocator
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            keep = fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    except torch.OutOfMemoryError as e:
        return {"error": "out of memory: " + str(e).splitlines()[0]}, None
    peak = torch.cuda.max_memory_allocated() - base
    return {"ms_per_call": round(statistics.median(ms), 3), "spread_ms": [round(min(ms), 3), round(max(ms), 3)],
            "runs_ms": [round(m, 3) for m in ms], "peak_bytes": int(peak)}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from pandasim.sim import PandaSim

    out = {"metric": "ms per batch of clouds: PandaSim.group_cloud vs a torch restatement of pointnet2_utils' steps",
           "n_points": a.points, "npoint": NPOINT, "radii": RADII, "nsamples": NSAMPLES, "feature_channels": 3,
           "runs": a.runs, "device": torch.cuda.get_device_name(0), "batches": []}
    for B in a.batches:
        sim = PandaSim("reach", num_envs=B, device="cuda:0")
        g = torch.Generator(device="cuda")
        g.manual_seed(B)
        # a table-like slab of points, as the observation's crop leaves them
        points = (torch.rand(B, a.points, 3, device="cuda", generator=g) - 0.5) * torch.tensor([0.7, 0.7, 0.15],
                                                                                                device="cuda")
        feats = torch.randint(0, 256, (B, a.points, 3), device="cuda", generator=g).float()
        start = torch.randint(0, a.points, (B,), device="cuda", generator=g, dtype=torch.int32)
        f, fused = measure(lambda: sim.group_cloud(points, feats, NPOINT, RADII, NSAMPLES, start=start), a.runs)
        fused_fps = fused.fps_idx.long().clone()
        del fused
        torch.cuda.empty_cache()
        t, ref = measure(lambda: torch_path(points, feats, start), a.runs)
        row = {"batch": B, "fused": f, "torch": t}
        if ref is not None:
            row["speedup"] = round(t["ms_per_call"] / f["ms_per_call"], 2)
            row["peak_ratio"] = round(f["peak_bytes"] / max(t["peak_bytes"], 1), 5)
            row["fps_idx_equal_clouds"] = int((ref[0] == fused_fps).all(-1).sum())
        row["fused_clouds_per_s"] = round(1e3 * B / f["ms_per_call"], 1)
        out["batches"].append(row)
        del ref, sim
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
