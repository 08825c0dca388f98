#!/usr/bin/env python
"""PointNet++ feature propagation (PandaSim.propagate_features, one
ps_cloud_feature_propagation launch) beside the two-call path
(ps_cloud_three_nn, then ps_cloud_interpolate, idx and weight through global
memory) and beside a torch restatement of what pointnet2_utils.py's
PointNetFeaturePropagation.forward does before its conv layers, on the same
GPU, at the shapes of the reference's segmentation model:

fp1  N 5 000, S 512, D1 9, D2 128
fp2  N 512, S 128, D1 320, D2 256

torch  a [B, N, S] distance matrix (-2ab + a^2 + b^2), its full sort (values
       and i64 indices of that shape), the first three, the reciprocal
       weights, the index_points gather [B, N, 3, D2], the weighted sum, the
       concatenation.

Per shape, batch size and path: ms per call as the median of --runs timed runs
(device events around one call, after a warm-up call), the fastest and slowest
run, and the peak of torch.cuda.max_memory_allocated above what was allocated
before the path ran.  A path that cannot allocate is recorded as such.  Prints
one JSON line; --out writes it to a file.

usage: python scripts/bench_propagate.py [--batches 64 256] [--runs 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

SHAPES = {"fp1": (5000, 512, 9, 128), "fp2": (512, 128, 320, 256)}  # N, S, D1, D2


def torch_path(xyz1, xyz2, points1, points2):
    import torch

    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    dists = -2 * torch.matmul(xyz1, xyz2.permute(0, 2, 1))
    dists += (xyz1 ** 2).sum(-1).view(B, N, 1)
    dists += (xyz2 ** 2).sum(-1).view(B, 1, S)
    dists, idx = dists.sort(dim=-1)
    dists, idx = dists[:, :, :3], idx[:, :, :3]
    recip = 1.0 / (dists + 1e-8)
    weight = recip / recip.sum(dim=2, keepdim=True)
    rows = torch.arange(B, device=xyz1.device).view(B, 1, 1)
    interp = (points2[rows, idx] * weight.view(B, N, 3, 1)).sum(dim=2)
    return torch.cat([points1, interp], dim=-1)


def composed_path(sim, xyz1, xyz2, points1, points2):
    import torch

    from pandasim.sim import _ptr

    B, N, _ = xyz1.shape
    S, D1, D2 = xyz2.shape[1], points1.shape[2], points2.shape[2]
    idx = torch.empty(B, N, 3, dtype=torch.int32, device=xyz1.device)
    weight = torch.empty(B, N, 3, dtype=torch.float32, device=xyz1.device)
    out = torch.empty(B, N, D1 + D2, dtype=torch.float32, device=xyz1.device)
    sim._call("ps_cloud_three_nn", sim._ctx, _ptr(xyz1), N, _ptr(xyz2), S, _ptr(idx), _ptr(weight), sim._stream())
    sim._call("ps_cloud_interpolate", sim._ctx, _ptr(points1), D1, _ptr(points2), D2, N, S, _ptr(idx), _ptr(weight),
              _ptr(out), sim._stream())
    return out


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
            keep = None  # one result alive at a time: the peak is one call's
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
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from pandasim.sim import PandaSim

    out = {"metric": "ms per batch of clouds: PandaSim.propagate_features vs the two ABI calls composed vs a torch "
                     "restatement of PointNetFeaturePropagation.forward's interpolation",
           "runs": a.runs, "device": torch.cuda.get_device_name(0), "rows": []}
    for shape in a.shapes:
        N, S, D1, D2 = SHAPES[shape]
        for B in a.batches:
            sim = PandaSim("reach", num_envs=B, device="cuda:0")
            g = torch.Generator(device="cuda")
            g.manual_seed(B)
            xyz1 = (torch.rand(B, N, 3, device="cuda", generator=g) - 0.5) * torch.tensor([0.7, 0.7, 0.15],
                                                                                         device="cuda")
            xyz2 = xyz1[:, torch.randperm(N, device="cuda", generator=g)[:S]].contiguous()  # coarse = some dense
            points1 = torch.randn(B, N, D1, device="cuda", generator=g)
            points2 = torch.randn(B, S, D2, device="cuda", generator=g)
            out_bytes = B * N * (D1 + D2) * 4
            f, fused = measure(lambda: sim.propagate_features(xyz1, xyz2, points2, points1), a.runs)
            c, comp = measure(lambda: composed_path(sim, xyz1, xyz2, points1, points2), a.runs)
            same = bool(torch.equal(fused, comp))
            del comp
            torch.cuda.empty_cache()
            t, ref = measure(lambda: torch_path(xyz1, xyz2, points1, points2), a.runs)
            row = {"shape": shape, "N": N, "S": S, "D1": D1, "D2": D2, "batch": B, "output_bytes": out_bytes,
                   "fused": f, "composed": c, "torch": t, "fused_equals_composed": same,
                   # the caching allocator may round a large block up to a multiple of 2 MiB
                   "fused_peak_is_its_output": out_bytes <= f["peak_bytes"] <= -(-out_bytes // (2 << 20)) * (2 << 20),
                   "fused_over_composed": round(f["ms_per_call"] / c["ms_per_call"], 3),
                   "fused_GBps_of_output": round(out_bytes / f["ms_per_call"] / 1e6, 1)}
            if ref is not None:
                row["speedup_over_torch"] = round(t["ms_per_call"] / f["ms_per_call"], 2)
                row["peak_ratio_to_torch"] = round(f["peak_bytes"] / max(t["peak_bytes"], 1), 5)
                row["max_abs_difference_to_torch"] = float((ref - fused).abs().max())
            out["rows"].append(row)
            del ref, fused, sim
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
