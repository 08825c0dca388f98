"""Bit-for-bit comparison of two libpandasim builds: every task (ee and
joints control) at B envs for K steps with the same seeded resets and
actions, each library in its own process (PANDASIM_LIB); prints per task the
number of state floats that differ and the largest difference.  For changes
meant to keep the arithmetic (instruction selection, data placement).
MODE "images" compares the camera entry points instead (ps_render,
ps_deproject_image, ps_deproject_pixels): per task, after K steps, 16 envs at
64x48 from three cameras and 2 envs at 480x480 from one -- depth, rgb, points,
valid, pixels_2d and the deprojection of a pixel list; "all" does both.
Usage: python scripts/compare_libs.py LIB_A LIB_B [B] [K] [steps|images|all]"""
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
for task in ("reach", "push", "pick_and_place", "slide", "flip", "stack") if MODE != "steps" else ():
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
    for control in ("ee", "joints") if MODE != "images" else ():
        env = PandaVecEnv(task, "sparse", control, B, "cuda", lanes_per_env=LANES)
        env.reset(seed=7)
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        for k in range(K):
            a = torch.rand(B, env.action_dim, device="cuda", generator=g) * 2 - 1
            env.step(a)
        out[f"{task}_{control}"] = env.sim.f[:, :B].cpu().numpy()
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
        envs = neq.any(0).sum() if "_cam" not in k else neq.reshape(len(neq), -1).any(1).sum()  # images: env-major
        print(f"{k:22s} differing values {int(neq.sum()):8d} of {x.size}  envs {int(envs):5d}  "
              f"max |diff| {float(np.nanmax(np.abs(x - y))) if neq.any() else 0.0:.3e}", flush=True)
    print("bit-identical" if same else "DIFFERENT", os.path.basename(a), os.path.basename(b), f"B={B} K={K} {mode}")


if __name__ == "__main__":
    main()
