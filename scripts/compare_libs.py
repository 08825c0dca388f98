"""Bit-for-bit comparison of two libpandasim builds: every task (ee and
joints control) at B envs for K steps with the same seeded resets and
actions, each library in its own process (PANDASIM_LIB); prints per task the
number of state floats that differ and the largest difference.  For changes
meant to keep the arithmetic (instruction selection, data placement).
MODE "images" compares the camera entry points instead (ps_render,
ps_deproject_image, ps_deproject_pixels): per task, after K steps, 16 envs at
64x48 from three cameras and 2 envs at 480x480 from one -- depth, rgb, points,
valid, pixels_2d and the deprojection of a pixel list.
MODE "mlp" compares the shared MLP's four entry points (ps_cloud_mlp,
ps_cloud_group_mlp and their _bfloat twins) on seeded normal data, where the
bfloat16 tests only assert a bound: through PandaSim.shared_mlp and
abstract_features(fused=True) at batches of 2 and 7, row shapes on both sides
of every tile, k-step, k-chunk and wave-count boundary of the two kernels, and
gathered rows written at a column offset into a wider, pre-filled tensor.
"all" does the three.
Usage: python scripts/compare_libs.py LIB_A LIB_B [B] [K] [steps|images|mlp|all]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.join(os.environ["ROOT"], "panda-lang-manip_amd"))
from pandasim.envs import PandaVecEnv
B, K = int(os.environ["B"]), int(os.environ["K"])
out = {}
LANES = int(os.environ.get("LANES", "0"))
MODE = os.environ.get("MODE", "steps")
CAMS = [((0, 0, 0), 1.4, 45, -30, 0), ((-0.1, 0.1, 0), 0.9, 90, -70, 0), ((0, 0, 0.1), 0.6, 135, -30, 0)]
for task in ("reach", "push", "pick_and_place", "slide", "flip", "stack") if MODE in ("images", "all") else ():
    for n, w, h, cams in ((16, 64, 48, CAMS), (2, 480, 480, CAMS[2:])):
        env = PandaVecEnv(task, "sparse", "ee", n, "cuda", autoreset=False)
        env.reset(seed=7)
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        for k in range(K):
            env.step(torch.rand(n, env.action_dim, device="cuda", generator=g) * 2 - 1)
        for ci, cam in enumerate(cams):
            r = env.sim.render(w, h, *cam)
            _, _, tran = env.sim.get_cam2world_transforms(w, h, *cam)
            pix = torch.stack([torch.arange(0, w, 3), torch.arange(0, w, 3) % h], 1)
            r["deproject"] = env.sim.deproject(r["depth"], pix, tran, width=w, height=h)
            for name in ("depth", "colors", "points", "valid", "pixels_2d", "deproject"):
                out[f"{task}_{w}x{h}_cam{ci}_{name}"] = r[name].cpu().numpy()
for task in ("reach", "push", "pick_and_place", "slide", "flip") + (("stack",) if LANES <= 1 else ()):
    for control in ("ee", "joints") if MODE in ("steps", "all") else ():
        env = PandaVecEnv(task, "sparse", control, B, "cuda", lanes_per_env=LANES)
        env.reset(seed=7)
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        for k in range(K):
            a = torch.rand(B, env.action_dim, device="cuda", generator=g) * 2 - 1
            env.step(a)
        out[f"{task}_{control}"] = env.sim.f[:, :B].cpu().numpy()
# (R, C0, widths, pools): both sides of the 32/64-row tile, the 16-k step, the 512-k chunk, every wave count, groups
# longer than one and two tiles
MLP_ROWS = [(1, 1, [1], (1,)), (33, 9, [33], (1,)), (65, 45, [196, 1], (5,)), (130, 9, [32, 96, 196, 1000], (1, 130)),
            (256, 9, [64, 64], (128,)), (70, 515, [96, 33], (1, 70)), (40, 2051, [512, 512, 1024], (40,))]
MLP_GATHERED = [(0, 12), (6, 33), (16, 65), (320, 5)]  # (D, K) of N = 200 points, S = 21 centres
def mlp_of(rng, c_in, widths, prec):
    from pandasim import CloudMlp
    layers = []
    for c_out in widths:
        layers.append(((rng.normal(size=(c_out, c_in)) / np.sqrt(c_in)).astype(np.float32),
                       (rng.normal(size=c_out) * 0.2).astype(np.float32), True))
        c_in = c_out
    return CloudMlp(layers, "cuda", precision=prec)
for nb in (2, 7) if MODE in ("mlp", "all") else ():
    from pandasim.sim import PandaSim, _ptr
    sim = PandaSim("reach", num_envs=nb, device="cuda:0")
    for prec, suffix in (("float32", ""), ("bfloat16", "_bfloat")):
        rng = np.random.default_rng(nb)  # the same data in both precisions
        for R, C0, widths, pools in MLP_ROWS:
            rows = torch.from_numpy(rng.normal(size=(nb, R, C0)).astype(np.float32)).cuda()
            mlp = mlp_of(rng, C0, widths, prec)
            for pool in pools:
                key = f"mlp_{prec}_B{nb}_R{R}_C{C0}_w{'-'.join(map(str, widths))}_pool{pool}"
                out[key] = sim.shared_mlp(rows, mlp, pool=pool).cpu().numpy()
        for D, K in MLP_GATHERED:
            N, S, pad, off = 200, 21, 11, 5
            xyz = torch.from_numpy(rng.normal(size=(nb, N, 3)).astype(np.float32)).cuda()
            feats = torch.from_numpy(rng.normal(size=(nb, N, D)).astype(np.float32)).cuda() if D else None
            centre = torch.from_numpy(rng.integers(0, N, size=(nb, S)).astype(np.int32)).cuda()
            gidx = torch.from_numpy(rng.integers(0, N, size=(nb, S, K)).astype(np.int32)).cuda()
            mlp = mlp_of(rng, D + 3, [32, 96, 40], prec)
            out[f"mlp_{prec}_B{nb}_gathered_D{D}_K{K}"] = sim.abstract_features(xyz, feats, centre, [gidx], [mlp],
                                                                               fused=True).cpu().numpy()
            # the entry point itself at a column offset of a wider tensor: a write outside its columns shows too
            wide = torch.full((nb, S, 40 + pad), -12345.5, device="cuda")
            sim._call("ps_cloud_group_mlp" + suffix, sim._ctx, _ptr(xyz), _ptr(feats), N, D, _ptr(centre), S, _ptr(gidx),
                      K, mlp.array, len(mlp), _ptr(wide), 40 + pad, off, sim._stream())
            out[f"mlp_{prec}_B{nb}_gathered_D{D}_K{K}_offset{off}"] = wide.cpu().numpy()
np.savez(os.environ["OUT"], **out)
'''


def run(lib, path, B, K, mode):
    env = dict(os.environ, PANDASIM_LIB=os.path.abspath(lib), ROOT=ROOT, OUT=path, B=str(B), K=str(K), MODE=mode)
    subprocess.run([sys.executable, "-c", CHILD], env=env, check=True, timeout=900)
    return dict(np.load(path))


def main():
    a, b = sys.argv[1], sys.argv[2]
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    mode = sys.argv[5] if len(sys.argv) > 5 else "steps"
    with tempfile.TemporaryDirectory() as d:
        ra, rb = run(a, os.path.join(d, "a.npz"), B, K, mode), run(b, os.path.join(d, "b.npz"), B, K, mode)
    same = True
    for k in ra:
        x, y = ra[k].astype(np.float64), rb[k].astype(np.float64)
        neq = ~((x == y) | (np.isnan(x) & np.isnan(y)))
        same &= not neq.any()
        env_major = "_cam" in k or k.startswith("mlp_")  # images and MLP outputs; the state is row-major
        envs = neq.reshape(len(neq), -1).any(1).sum() if env_major else neq.any(0).sum()
        print(f"{k:22s} differing values {int(neq.sum()):8d} of {x.size}  envs {int(envs):5d}  "
              f"max |diff| {float(np.nanmax(np.abs(x - y))) if neq.any() else 0.0:.3e}", flush=True)
    print("bit-identical" if same else "DIFFERENT", os.path.basename(a), os.path.basename(b), f"B={B} K={K} {mode}")


if __name__ == "__main__":
    main()
