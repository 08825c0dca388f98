"""Generate the golden vectors of the PointNet++ feature propagation from the
reference's own envs/inference/models/pointnet2_utils.py on torch CPU.

Run where the reference is present (the GPU machine does not have it):
    python tests/golden/make_propagate_golden.py

The yardstick is the reference's class without weights:
PointNetFeaturePropagation(in_channel, mlp=[]) has no conv layer, so forward
returns exactly cat([points1, interpolated_points]) (permuted).  It runs in
float64: the f64 result is the golden, free of the sort ambiguity that the f32
rounding of the reference's -2ab + a^2 + b^2 form has where a distance is
truly 0.

The clouds are make_group_golden.make_cloud clouds (all points distinct), the
coarse points the reference's farthest_point_sample of them, torch.randint
replaced while it runs as in make_group_golden.py.  Features are small whole
numbers stored as i8, coarse indices as i16, the output as f64 [NB, N, D1+D2].

Cases (2 clouds each):
  A  N 300,  S 64,  D1 0, D2 8    S not a multiple of 64
  B  N 1000, S 128, D1 5, D2 8    points1 present, fp2-like
  C  N 128,  S 1,   D1 3, D2 16   the repeat branch
  D  N 7,    S 3,   D1 0, D2 1    exactly three coarse points; N below a wave
  E  N 5000, S 512, D1 0, D2 4    fp1's geometry; several blocks per cloud

Per dense point `ambiguous` says whether the direct f32 squared distances to
its 3rd and 4th nearest coarse point lie within 4e-6 of each other (the ball
query's band): there the f64 reference and an f32 implementation may pick
another third neighbour.  The script refuses a golden in which more than 5 %
of the rows of any case are ambiguous.  `nn` is the reference's three nearest
(i16, in its f64 order).

Output: tests/golden/propagate_golden.npz (data only).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_group_golden import AMBIGUOUS_BAND, MAX_SKIPPED, REF, make_cloud  # noqa: E402

OUT = os.path.join(HERE, "propagate_golden.npz")
CASES = {  # name: (N, S, D1, D2)
    "A": (300, 64, 0, 8),
    "B": (1000, 128, 5, 8),
    "C": (128, 1, 3, 16),
    "D": (7, 3, 0, 1),
    "E": (5000, 512, 0, 4),
}
NB = 2


def direct_d2(xyz1, xyz2):
    """[N, 3], [S, 3] f32 -> [N, S] f32, every product and sum rounded."""
    d = xyz1[:, None, :] - xyz2[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def main():
    import torch

    spec = importlib.util.spec_from_file_location("ref_pointnet2_utils", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261021)
    out = {}
    for name, (n, s, d1, d2) in CASES.items():
        xyz1 = np.stack([make_cloud(rng, n, None) for _ in range(NB)])
        start = rng.integers(0, n, size=NB).astype(np.int64)
        randint = torch.randint
        torch.randint = lambda *a, **k: torch.from_numpy(start)
        try:
            fps = ref.farthest_point_sample(torch.from_numpy(xyz1), s).numpy()
        finally:
            torch.randint = randint
        assert fps.shape == (NB, s) and (fps[:, 0] == start).all()
        xyz2 = np.stack([xyz1[b][fps[b]] for b in range(NB)])
        points2 = rng.integers(-100, 101, size=(NB, s, d2)).astype(np.int8)
        points1 = rng.integers(-100, 101, size=(NB, n, d1)).astype(np.int8)
        fp = ref.PointNetFeaturePropagation(in_channel=d1 + d2, mlp=[]).double()
        assert len(fp.mlp_convs) == 0
        t = lambda a: torch.from_numpy(a.astype(np.float64)).permute(0, 2, 1)  # noqa: E731
        with torch.no_grad():
            got = fp(t(xyz1), t(xyz2), t(points1) if d1 else None, t(points2))
        got = got.permute(0, 2, 1).contiguous().numpy()
        assert got.shape == (NB, n, d1 + d2) and got.dtype == np.float64
        amb = np.zeros((NB, n), bool)
        nn = np.zeros((NB, n, 3), np.int16)
        if s > 1:
            for b in range(NB):
                d = np.sort(direct_d2(xyz1[b], xyz2[b]).astype(np.float64), axis=1)
                if s > 3:
                    amb[b] = d[:, 3] - d[:, 2] < AMBIGUOUS_BAND
                a, c = xyz1[b].astype(np.float64), xyz2[b].astype(np.float64)
                sq = ref.square_distance(torch.from_numpy(a)[None], torch.from_numpy(c)[None])
                nn[b] = sq.sort(dim=-1)[1][0, :, :3].numpy().astype(np.int16)
        share = amb.mean()
        print(f"case {name}: {int(amb.sum())} of {amb.size} rows ambiguous ({100 * share:.2f} %)")
        assert share <= MAX_SKIPPED, "choose other clouds: too many ambiguous rows"
        out[f"{name}_xyz1"], out[f"{name}_coarse_idx"] = xyz1, fps.astype(np.int16)
        out[f"{name}_points2"], out[f"{name}_points1"] = points2, points1
        out[f"{name}_out"], out[f"{name}_ambiguous"], out[f"{name}_nn"] = got, amb, nn
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
