#!/usr/bin/env python
"""The shared MLP with max-pool (PandaSim.abstract_features / shared_mlp, f32
MFMA) at the shapes of the reference's first set-abstraction layer and its last
feature-propagation layer, beside the composed path and beside the reference's
own layers in torch on the same GPU:

sa1  N 5 000, S 512, D 6, three scales K (32, 64, 128) with widths
     [32, 32, 64], [64, 64, 128], [64, 96, 128] -> [B, 512, 320]
     fused     one ps_cloud_group_mlp per scale, rows gathered in the kernel
     composed  ps_cloud_group then ps_cloud_mlp per scale (the grouped tensor
               through global memory)
     torch     index gathers, Conv2d + BatchNorm2d (eval, f32) + ReLU on
               [B, C, K, S], torch.max over K, torch.cat
sa2  N 512 (sa1's centres), S 128, D 320, two scales K (64, 128) with widths
     [128, 128, 256], [128, 196, 256] -> [B, 128, 512]; fused and torch only
     (ps_cloud_group stops at D = 16)
fp1  N 5 000 rows of 137 channels, widths [128, 128] -> [B, 5 000, 128]
     fused     one ps_cloud_mlp (there is nothing to compose)
     torch     Conv1d + BatchNorm1d (eval, f32) + ReLU on [B, C, N]

--precision float32 bfloat16 measures the library's paths in each precision in
the same session (CloudMlp(..., precision=...): ps_cloud_mlp_bfloat /
ps_cloud_group_mlp_bfloat for bfloat16), one row per precision; torch is
measured once per shape and batch, in the first precision's row.

Per shape, batch size and path: ms per call as the median of --runs timed runs
(device events around one call, after a warm-up call), the fastest and slowest
run, the peak of torch.cuda.max_memory_allocated above what was allocated
before the path ran, and for the library's paths the achieved TFLOP/s (2 FLOP
per multiply-add of the layers) against the 157.3 TFLOP/s f32 matrix peak
(bfloat16: the 2 516.6 TFLOP/s bf16 one).
Prints one JSON line; --out writes it to a file.

usage: python scripts/bench_mlp.py [--batches 64 256] [--shapes sa1 sa2 fp1] [--precision float32 bfloat16]
                                   [--runs 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "panda-lang-manip_amd"))

PEAK_TFLOPS = 157.3
PEAKS = {"float32": PEAK_TFLOPS, "bfloat16": 16 * PEAK_TFLOPS}  # the bf16 MFMA issues at 16 times the f32 one's rate
SA1 = dict(N=5000, S=512, D=6, K=(32, 64, 128), widths=([32, 32, 64], [64, 64, 128], [64, 96, 128]))
SA2 = dict(N=512, S=128, D=320, K=(64, 128), widths=([128, 128, 256], [128, 196, 256]))
FP1 = dict(N=5000, C0=137, widths=[128, 128])


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


def reference_layers(c_in, widths, dims, gen):
    """The reference's conv + batch-norm stack in eval(), f32, on the GPU, with
    seeded non-trivial statistics."""
    import torch
    from torch import nn

    conv, bn = (nn.Conv2d, nn.BatchNorm2d) if dims == 2 else (nn.Conv1d, nn.BatchNorm1d)
    convs, bns = [], []
    for c_out in widths:
        convs.append(conv(c_in, c_out, 1))
        bns.append(bn(c_out))
        with torch.no_grad():
            bns[-1].weight.copy_(torch.rand(c_out, generator=gen) + 0.5)
            bns[-1].bias.copy_(torch.randn(c_out, generator=gen) * 0.3)
            bns[-1].running_mean.copy_(torch.randn(c_out, generator=gen) * 0.5)
            bns[-1].running_var.copy_(torch.rand(c_out, generator=gen) * 1.5 + 0.5)
        c_in = c_out
    return nn.ModuleList(convs).eval(), nn.ModuleList(bns).eval()


def folded(convs, bns, precision="float32"):
    from pandasim import CloudMlp, fold_batchnorm

    return CloudMlp([(*fold_batchnorm(c.weight, c.bias, b.weight, b.bias, b.running_mean, b.running_var, b.eps), True)
                     for c, b in zip(convs, bns)], "cuda", precision=precision)


def flops_of(rows, c_in, widths):
    total = 0
    for c_out in widths:
        total += 2 * rows * c_in * c_out
        c_in = c_out
    return total


def torch_sa1(xyz, feats, centre, gidx, stacks):
    import torch
    import torch.nn.functional as F

    B = xyz.shape[0]
    rows = torch.arange(B, device=xyz.device).view(B, 1, 1)
    new_xyz = xyz[rows[:, :, 0], centre.long()]
    outs = []
    with torch.no_grad():
        for gi, (convs, bns) in zip(gidx, stacks):
            gi = gi.long()
            g = torch.cat([feats[rows, gi], xyz[rows, gi] - new_xyz[:, :, None, :]], dim=-1).permute(0, 3, 2, 1)
            for conv, bn in zip(convs, bns):
                g = F.relu(bn(conv(g)))
            outs.append(torch.max(g, 2)[0])
        return torch.cat(outs, dim=1).permute(0, 2, 1)


def torch_fp1(rows, stack):
    import torch
    import torch.nn.functional as F

    with torch.no_grad():
        x = rows.permute(0, 2, 1)
        for conv, bn in zip(*stack):
            x = F.relu(bn(conv(x)))
        return x.permute(0, 2, 1)


def with_rates(m, flops, precision="float32"):
    if "ms_per_call" in m:
        m["tflops"] = round(flops / m["ms_per_call"] / 1e9, 2)
        key = "share_of_f32_matrix_peak" if precision == "float32" else "share_of_bf16_matrix_peak"
        m[key] = round(m["tflops"] / PEAKS[precision], 4)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--shapes", nargs="*", default=["sa1", "fp1"], choices=["sa1", "sa2", "fp1"])
    ap.add_argument("--precision", nargs="*", default=["float32"], choices=["float32", "bfloat16"])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from pandasim.sim import PandaSim

    out = {"metric": "ms per batch of clouds: the shared MLP with max-pool fused (rows gathered in the kernel) vs "
                     "composed (ps_cloud_group, then ps_cloud_mlp) vs the reference's conv + batch-norm layers in "
                     "torch (eval, f32)", "runs": a.runs, "device": torch.cuda.get_device_name(0),
           "f32_matrix_peak_tflops": PEAK_TFLOPS, "bf16_matrix_peak_tflops": PEAKS["bfloat16"], "rows": []}
    cpu = torch.Generator().manual_seed(1)
    for shape in a.shapes:
        for B in a.batches:
            sim = PandaSim("reach", num_envs=B, device="cuda:0")
            g = torch.Generator(device="cuda")
            g.manual_seed(B)
            if shape in ("sa1", "sa2"):
                P = SA1 if shape == "sa1" else SA2
                N, S, D, Ks, widths = P["N"], P["S"], P["D"], P["K"], P["widths"]
                xyz = (torch.rand(B, N, 3, device="cuda", generator=g) - 0.5) * torch.tensor([0.7, 0.7, 0.15],
                                                                                            device="cuda")
                feats = torch.randn(B, N, D, device="cuda", generator=g)
                centre = torch.randint(0, N, (B, S), device="cuda", generator=g, dtype=torch.int32)
                gidx = [torch.randint(0, N, (B, S, k), device="cuda", generator=g, dtype=torch.int32).sort(-1)[0]
                        for k in Ks]
                stacks = [tuple(m.cuda() for m in reference_layers(D + 3, w, 2, cpu)) for w in widths]
                flops = sum(flops_of(B * S * k, D + 3, w) for k, w in zip(Ks, widths))
                shape_row = {"shape": shape, "N": N, "S": S, "D": D, "K": list(Ks), "widths": [list(w) for w in widths]}
            else:
                N, C0, widths = FP1["N"], FP1["C0"], FP1["widths"]
                rows = torch.randn(B, N, C0, device="cuda", generator=g)
                stack = tuple(m.cuda() for m in reference_layers(C0, widths, 1, cpu))
                flops = flops_of(B * N, C0, widths)
                shape_row = {"shape": shape, "N": N, "C0": C0, "widths": list(widths)}
            for i, prec in enumerate(a.precision):
                c, same, t, ref = None, None, None, None
                if shape == "fp1":
                    mlp = folded(*stack, prec)
                    f, fused = measure(lambda: sim.shared_mlp(rows, mlp), a.runs)
                    if i == 0:
                        t, ref = measure(lambda: torch_fp1(rows, stack), a.runs)
                else:
                    mlps = [folded(*st, prec) for st in stacks]
                    f, fused = measure(lambda: sim.abstract_features(xyz, feats, centre, gidx, mlps, fused=True), a.runs)
                    if D <= 16:
                        c, comp = measure(lambda: sim.abstract_features(xyz, feats, centre, gidx, mlps, fused=False),
                                          a.runs)
                        same = bool(torch.equal(fused, comp))
                        del comp
                        torch.cuda.empty_cache()
                    if i == 0:
                        t, ref = measure(lambda: torch_sa1(xyz, feats, centre, gidx, stacks), a.runs)
                row = dict(shape_row, precision=prec)
                out_bytes = fused.numel() * 4
                row.update({"batch": B, "gflop_per_cloud": round(flops / B / 1e9, 3), "output_bytes": out_bytes,
                            "fused": with_rates(f, flops, prec),
                            "composed": None if c is None else with_rates(c, flops, prec),
                            "torch": t, "fused_equals_composed": same})
                if c is not None:
                    row["fused_over_composed"] = round(f["ms_per_call"] / c["ms_per_call"], 3)
                if ref is not None:
                    row["speedup_over_torch"] = round(t["ms_per_call"] / f["ms_per_call"], 2)
                    row["peak_ratio_to_torch"] = round(f["peak_bytes"] / max(t["peak_bytes"], 1), 5)
                    row["max_abs_difference_to_torch"] = float((ref - fused).abs().max())
                    row["max_abs_of_torch"] = float(ref.abs().max())
                out["rows"].append(row)
                del ref, fused
                torch.cuda.empty_cache()
            del sim
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
