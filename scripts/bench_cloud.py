#!/usr/bin/env python
"""Fused multi-view point-cloud observation (ps_point_cloud) against the
composition it fuses, on one GPU: Push, the four grasp views, 480x480,
K = 5 000 points per env.

fused    PandaSim.point_cloud: three kernels over a bit-mask workspace.
unfused  per view ps_render + ps_deproject_image (points f64, valid; no
         pixels_2d) into preallocated [V, B, ...] buffers, then per env a torch
         mask over the concatenated views, nonzero, a uniform draw with
         replacement and a gather: the ragged indexing render() leaves to the
         caller.

Per batch size: clouds/s as the median of --runs timed runs of --reps calls
each (wall clock around a device synchronisation, since the unfused path waits
on the host for every env's count), the spread (min, max) of the runs, and the
peak of torch.cuda.max_memory_allocated above what was allocated before the
path first ran.  The views' ps_render + ps_deproject_image alone (no merge, no
draw) are timed too, to separate the kernels from the host-bound merge.  The
fused path also runs alone at --fused-only-batch envs.  Prints
one JSON line; --out writes it to a file.

usage: python scripts/bench_cloud.py [--batches 64 256] [--fused-only-batch 4096] [--runs 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))


def make_sim(env_id, batch):
    import torch

    import pandasim

    env = pandasim.make(env_id, num_envs=batch)
    env.reset(seed=12345)
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    for _ in range(5):
        env.step(torch.rand(batch, env.action_dim, device="cuda", generator=g) * 2 - 1, copy=False)
    return env


def unfused_path(sim, views, W, H, K, merge=True):
    """The composition, with its buffers allocated inside (they are its
    footprint); merge=False stops after the views' render + deproject."""
    import torch

    from pandasim.sim import _ptr

    B, V, n = sim.num_envs, len(views), W * H
    points = torch.empty(V, B, n, 3, dtype=torch.float64, device="cuda")
    valid = torch.empty(V, B, n, dtype=torch.uint8, device="cuda")
    rgb = []
    for v, kw in enumerate(views):
        view, proj, tran = sim.get_cam2world_transforms(W, H, **kw)
        depth, img = sim.get_camera_image(W, H, view, proj)
        T = (C.c_double * 16)(*tran.reshape(-1).tolist())
        sim._call("ps_deproject_image", sim._ctx, _ptr(depth), T, W, H, _ptr(points[v]), _ptr(valid[v]), None,
                  sim._stream())
        rgb.append(img.reshape(B, n, 3))
    if not merge:
        return points, valid
    rgb = torch.stack(rgb)  # [V, B, n, 3]
    keep = valid.bool().permute(1, 0, 2).reshape(B, V * n)  # views concatenated per env
    out_p = torch.zeros(B, K, 3, dtype=torch.float32, device="cuda")
    out_c = torch.zeros(B, K, 3, dtype=torch.uint8, device="cuda")
    for b in range(B):
        idx = keep[b].nonzero().squeeze(1)
        m = idx.numel()
        if m == 0:
            continue
        src = idx[(torch.rand(K, device="cuda") * m).long().clamp_(max=m - 1)]
        v, p = src // n, src % n
        out_p[b] = points[v, b, p].float()
        out_c[b] = rgb[v, b, p]
    return out_p, out_c


def measure(fn, batch, runs, reps):
    import torch

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()  # warm-up: kernel load, and whatever the path keeps allocated (the fused workspace)
    rates = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        rates.append(batch * reps / (time.perf_counter() - t0))
    peak = torch.cuda.max_memory_allocated() - base
    return {"clouds_per_s": round(statistics.median(rates), 1), "spread": [round(min(rates), 1), round(max(rates), 1)],
            "runs": [round(r, 1) for r in rates], "ms_per_call": round(1e3 * batch / statistics.median(rates), 3),
            "peak_bytes": int(peak)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-id", default="PandaPush-v3")
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--fused-only-batch", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import pandasim

    views, W, H, K = list(pandasim.GRASP_VIEWS), a.size, a.size, a.points
    out = {"metric": "point clouds/s: fused ps_point_cloud vs per-view render + deproject + torch merge and draw",
           "env_id": a.env_id, "views": len(views), "width": W, "height": H, "n_points": K, "runs": a.runs,
           "reps_per_run": a.reps, "device": torch.cuda.get_device_name(0), "batches": []}
    for B in a.batches:
        env = make_sim(a.env_id, B)
        sim = env.sim
        seed = [0]

        def fused():
            seed[0] += 1
            return sim.point_cloud(views, n_points=K, width=W, height=H, seed=seed[0])

        f = measure(fused, B, a.runs, a.reps)
        sim._cloud_ws = None  # the unfused path runs without the fused path's workspace
        torch.cuda.empty_cache()
        u = measure(lambda: unfused_path(sim, views, W, H, K), B, a.runs, a.reps)
        r = measure(lambda: unfused_path(sim, views, W, H, K, merge=False), B, a.runs, a.reps)
        row = {"batch": B, "fused": f, "unfused": u, "unfused_render_deproject_only": r,
               "speedup": round(f["clouds_per_s"] / u["clouds_per_s"], 2),
               "peak_ratio": round(f["peak_bytes"] / max(u["peak_bytes"], 1), 5),
               "workspace_bytes": int(pandasim.lib().ps_cloud_workspace_bytes(B, len(views), W, H))}
        row["fused_not_slower"] = f["clouds_per_s"] >= u["clouds_per_s"]
        row["fused_peak_below_a_tenth"] = f["peak_bytes"] < 0.1 * u["peak_bytes"]
        out["batches"].append(row)
        env.close()
        del env, sim
        torch.cuda.empty_cache()
    if a.fused_only_batch:
        B = a.fused_only_batch
        env = make_sim(a.env_id, B)
        f = measure(lambda: env.sim.point_cloud(views, n_points=K, width=W, height=H, seed=1), B, a.runs, a.reps)
        out["fused_only"] = {"batch": B, "fused": f,
                             "workspace_bytes": int(pandasim.lib().ps_cloud_workspace_bytes(B, len(views), W, H))}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
