"""Generate the golden vectors of the shared MLP with max-pool from the
reference's own envs/inference/models/pointnet2_utils.py on torch CPU.

Run where the reference is present (the GPU machine does not have it):
    python tests/golden/make_mlp_golden.py

The yardsticks are the reference's classes with their learned layers, in
.eval() and .double(): seeded conv weights and non-trivial batch-norm running
statistics (var in 0.5..2, mean and beta not 0), every parameter a float32
value, so the f64 run is the exact-arithmetic result of f32 data.  The clouds
are make_group_golden.make_cloud clouds.  farthest_point_sample and
query_ball_point of the module are wrapped while it runs and what they
returned is stored, so a test feeds the same indices and no ball-query
ambiguity enters.

Cases (2 clouds each):
  msg  PointNetSetAbstractionMsg: N 300, S 16, radii (0.2, 0.4), K (8, 16),
       D 6, widths [[32, 32, 64], [64, 96, 128]]       -> out [2, 16, 192]
  all  PointNetSetAbstraction(group_all): N 40, D 29 (rows are xyz then the
       features, 32 channels), widths [64, 128, 256]   -> out [2, 1, 256]
  fp   PointNetFeaturePropagation: N 70, one coarse point (the repeat branch:
       the rows are points1 [40] then points2 [5] exactly), widths [64, 32]
                                                       -> out [2, 70, 32]

Per case: the inputs (f32), the indices (i32), per layer conv_w, conv_b and
the batch norm's gamma, beta, mean, var (f32) with its eps, and the f64 output
in [B, rows, channels] layout.

Output: tests/golden/mlp_golden.npz (data only).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_group_golden import REF, make_cloud  # noqa: E402

OUT = os.path.join(HERE, "mlp_golden.npz")
NB = 2
MSG = dict(n=300, s=16, radii=(0.2, 0.4), k=(8, 16), d=6, widths=[[32, 32, 64], [64, 96, 128]])
ALL = dict(n=40, d=29, widths=[64, 128, 256])
FP = dict(n=70, d1=40, d2=5, widths=[64, 32])


def randomise(torch, convs, bns, gen):
    """Non-trivial batch-norm statistics; returns the layers' raw parameters."""
    layers = []
    for conv, bn in zip(convs, bns):
        c = bn.num_features
        with torch.no_grad():
            bn.weight.copy_(torch.rand(c, generator=gen) + 0.5)
            bn.bias.copy_(torch.randn(c, generator=gen) * 0.3)
            bn.running_mean.copy_(torch.randn(c, generator=gen) * 0.5)
            bn.running_var.copy_(torch.rand(c, generator=gen) * 1.5 + 0.5)
        layers.append(dict(conv_w=conv.weight.detach().numpy().reshape(conv.out_channels, conv.in_channels).copy(),
                           conv_b=conv.bias.detach().numpy().copy(), gamma=bn.weight.detach().numpy().copy(),
                           beta=bn.bias.detach().numpy().copy(), mean=bn.running_mean.numpy().copy(),
                           var=bn.running_var.numpy().copy(), eps=np.float64(bn.eps)))
    for layer in layers:
        assert all(v.dtype == np.float32 for k, v in layer.items() if k != "eps")
    return layers


def store(out, prefix, layers):
    for k, layer in enumerate(layers):
        for name, v in layer.items():
            out[f"{prefix}_l{k}_{name}"] = v


def main():
    import torch

    spec = importlib.util.spec_from_file_location("ref_pointnet2_utils", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261022)
    torch.manual_seed(20261022)
    gen = torch.Generator().manual_seed(7)
    out = {}
    t = lambda a: torch.from_numpy(a.astype(np.float64)).permute(0, 2, 1)  # noqa: E731

    # ---- msg
    c = MSG
    xyz = np.stack([make_cloud(rng, c["n"], None) for _ in range(NB)])
    feats = rng.normal(size=(NB, c["n"], c["d"])).astype(np.float32)
    sa = ref.PointNetSetAbstractionMsg(c["s"], list(c["radii"]), list(c["k"]), c["d"], c["widths"])
    per_scale = [randomise(torch, sa.conv_blocks[i], sa.bn_blocks[i], gen) for i in range(len(c["k"]))]
    sa = sa.double().eval()
    seen = {"fps": [], "ball": []}
    fps0, ball0 = ref.farthest_point_sample, ref.query_ball_point

    def fps(*a, **k):
        # the reference's sampler keeps its distances in f32: it takes the f32 cloud
        seen["fps"].append(fps0(a[0].float(), *a[1:], **k))
        return seen["fps"][-1]

    def ball(*a, **k):
        seen["ball"].append(ball0(*a, **k))
        return seen["ball"][-1]

    ref.farthest_point_sample, ref.query_ball_point = fps, ball
    try:
        with torch.no_grad():
            _, got = sa(t(xyz), t(feats))
    finally:
        ref.farthest_point_sample, ref.query_ball_point = fps0, ball0
    assert len(seen["fps"]) == 1 and len(seen["ball"]) == len(c["k"])
    out["msg_xyz"], out["msg_feats"] = xyz, feats
    out["msg_centre_idx"] = seen["fps"][0].numpy().astype(np.int32)
    for i, gi in enumerate(seen["ball"]):
        out[f"msg_group_idx{i}"] = gi.numpy().astype(np.int32)
        assert out[f"msg_group_idx{i}"].shape == (NB, c["s"], c["k"][i])
        store(out, f"msg_s{i}", per_scale[i])
    out["msg_out"] = got.permute(0, 2, 1).contiguous().numpy()
    assert out["msg_out"].shape == (NB, c["s"], sum(w[-1] for w in c["widths"])) and out["msg_out"].dtype == np.float64

    # ---- all
    c = ALL
    xyz = np.stack([make_cloud(rng, c["n"], None) for _ in range(NB)])
    feats = rng.normal(size=(NB, c["n"], c["d"])).astype(np.float32)
    sa = ref.PointNetSetAbstraction(None, None, None, c["d"] + 3, c["widths"], True)
    layers = randomise(torch, sa.mlp_convs, sa.mlp_bns, gen)
    sa = sa.double().eval()
    with torch.no_grad():
        _, got = sa(t(xyz), t(feats))
    out["all_xyz"], out["all_feats"] = xyz, feats
    store(out, "all", layers)
    out["all_out"] = got.permute(0, 2, 1).contiguous().numpy()
    assert out["all_out"].shape == (NB, 1, c["widths"][-1])

    # ---- fp
    c = FP
    xyz1 = np.stack([make_cloud(rng, c["n"], None) for _ in range(NB)])
    xyz2 = xyz1[:, :1].copy()
    points1 = rng.normal(size=(NB, c["n"], c["d1"])).astype(np.float32)
    points2 = rng.normal(size=(NB, 1, c["d2"])).astype(np.float32)
    fp = ref.PointNetFeaturePropagation(c["d1"] + c["d2"], c["widths"])
    layers = randomise(torch, fp.mlp_convs, fp.mlp_bns, gen)
    fp = fp.double().eval()
    with torch.no_grad():
        got = fp(t(xyz1), t(xyz2), t(points1), t(points2))
    out["fp_points1"], out["fp_points2"] = points1, points2
    store(out, "fp", layers)
    out["fp_out"] = got.permute(0, 2, 1).contiguous().numpy()
    assert out["fp_out"].shape == (NB, c["n"], c["widths"][-1])

    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
