"""Generate the golden vectors of the PointNet++ front end from the reference's
own envs/inference/models/pointnet2_utils.py (farthest_point_sample,
query_ball_point, index_points) on torch CPU.

Run where the reference is present (the GPU machine does not have it):
    python tests/golden/make_group_golden.py

farthest_point_sample draws its first index with torch.randint; while it runs,
torch.randint is replaced by a function returning the recorded start indices,
nothing else of the reference is touched.  The grouped tensor is what
PointNetSetAbstractionMsg.forward builds before its permute:
cat([index_points(feats, idx), index_points(xyz, idx) - new_xyz], -1).

Cases (3 clouds each; clouds are pc_normalize'd so the first layer's radii mean
what they mean in the reference):
  A  N 257, S 64, 100 distinct points, scales (0.2, 16), (0.4, 32)
  B  N 1000, S 128, 300 distinct points, the first layer's three scales
  C  N 64, S 64, 20 distinct points, no ball query
  D1 N 1, S 1;  D2 N 2, S 2
  E  N 5000, S 512, the first layer's three scales

Per ball-query row `ambiguous` says whether any point's direct f32 squared
distance lies within 4e-6 of r^2 (there the reference's -2ab + a^2 + b^2
expansion may round to the other side); the script refuses a golden in which
more than 5 % of the rows of any case and scale are ambiguous.

The grouped tensors of the larger cases exceed what a committed file may hold
(case E's alone is 9.6 MB), so the file records of every grouped tensor a
64-bit hash per (cloud, centre) row over the bit patterns of its
nsample * (D + 3) floats (row_hash below, checked over every element) and the
tensor itself for the centres grouped_centres(S).  Features are whole numbers
0..255 (colours as floats) stored as u8, group indices as i16.

Output: tests/golden/group_golden.npz (data only).
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/panda_gym/envs/inference/models/pointnet2_utils.py"
OUT = os.path.join(HERE, "group_golden.npz")
FIRST_LAYER = ((0.1, 32), (0.2, 64), (0.4, 128))
CASES = {  # name: (N, S, distinct points or None, scales)
    "A": (257, 64, 100, ((0.2, 16), (0.4, 32))),
    "B": (1000, 128, 300, FIRST_LAYER),
    "C": (64, 64, 20, ()),
    "D1": (1, 1, None, ()),
    "D2": (2, 2, None, ()),
    "E": (5000, 512, None, FIRST_LAYER),
}
NB, NFEAT, AMBIGUOUS_BAND, MAX_SKIPPED = 3, 4, 4e-6, 0.05


def grouped_centres(s: int) -> np.ndarray:
    """The centres whose grouped rows are recorded in full: 4, evenly spaced."""
    return np.unique(np.linspace(0, s - 1, 4).astype(np.int64))


def row_hash(grouped: np.ndarray) -> np.ndarray:
    """[B, S, K, C] f32 -> [B, S] u64: sum over a row's K * C bit patterns of
    bits * (2 * position + 1) * 0x9E3779B97F4A7C15 (mod 2^64)."""
    b, s = grouped.shape[:2]
    bits = np.ascontiguousarray(grouped, np.float32).view(np.uint32).reshape(b, s, -1).astype(np.uint64)
    w = (2 * np.arange(bits.shape[2], dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return (bits * w).sum(-1, dtype=np.uint64)


def make_cloud(rng, n, distinct):
    """A slab with a box on it, pc_normalize'd in f32; with `distinct`, n draws
    with replacement from that many points.  The slab of the 5 000-point case
    is thick (0.25 against 0.02): in a thin one 6.5 % of its rows at radius 0.1
    had a point within the ambiguous band, above the 5 % the golden may skip."""
    m = distinct or n
    pts = rng.uniform(-1.0, 1.0, size=(m, 3)) * np.array([0.35, 0.35, 0.25 if n >= 5000 else 0.02])
    box = rng.random(m) < 0.4
    pts[box] = rng.uniform(-1.0, 1.0, size=(int(box.sum()), 3)) * np.array([0.06, 0.06, 0.06]) + [0.05, -0.1, 0.08]
    pts = pts.astype(np.float32)
    if distinct:
        pts = pts[rng.integers(0, m, size=n)]
    pts = pts - pts.mean(0, dtype=np.float32)
    scale = np.sqrt((pts ** 2).sum(1)).max()
    return (pts / scale if scale > 0 else pts).astype(np.float32)


def direct_d2(xyz, centre):
    d = xyz - centre
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def main():
    import torch

    spec = importlib.util.spec_from_file_location("ref_pointnet2_utils", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20261020)
    out = {}
    for name, (n, s, distinct, scales) in CASES.items():
        xyz = np.stack([make_cloud(rng, n, distinct) for _ in range(NB)])
        start = rng.integers(0, n, size=NB).astype(np.int32)
        feats = rng.integers(0, 256, size=(NB, n, NFEAT)).astype(np.uint8)
        txyz, tfeats = torch.from_numpy(xyz), torch.from_numpy(feats.astype(np.float32))
        randint = torch.randint
        torch.randint = lambda *a, **k: torch.from_numpy(start.astype(np.int64))
        try:
            fps = ref.farthest_point_sample(txyz, s)
        finally:
            torch.randint = randint
        assert fps.shape == (NB, s) and bool((fps[:, 0] == torch.from_numpy(start.astype(np.int64))).all())
        new_xyz = ref.index_points(txyz, fps)
        out[f"{name}_xyz"], out[f"{name}_start"], out[f"{name}_feats"] = xyz, start, feats
        out[f"{name}_fps_idx"] = fps.numpy().astype(np.int32)
        out[f"{name}_scales"] = np.array(scales, np.float64).reshape(-1, 2)
        for k, (radius, nsample) in enumerate(scales):
            idx = ref.query_ball_point(radius, nsample, txyz, new_xyz)
            g_xyz = ref.index_points(txyz, idx) - new_xyz.view(NB, s, 1, 3)
            grouped = torch.cat([ref.index_points(tfeats, idx), g_xyz], dim=-1).numpy()
            r2 = np.float32(radius * radius)
            amb = np.zeros((NB, s), bool)
            for b in range(NB):
                for c in range(s):
                    d2 = direct_d2(xyz[b], xyz[b, int(fps[b, c])])
                    amb[b, c] = bool((np.abs(d2.astype(np.float64) - float(r2)) < AMBIGUOUS_BAND).any())
            share = amb.mean()
            print(f"case {name} radius {radius}: {int(amb.sum())} of {amb.size} rows ambiguous ({100 * share:.2f} %)")
            assert share <= MAX_SKIPPED, "choose other clouds: too many ambiguous rows"
            assert int(idx.max()) < n
            out[f"{name}_group_idx_{k}"] = idx.numpy().astype(np.int16)
            out[f"{name}_ambiguous_{k}"] = amb
            out[f"{name}_grouped_hash_{k}"] = row_hash(grouped)
            out[f"{name}_grouped_rows_{k}"] = grouped[:, grouped_centres(s)].astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
