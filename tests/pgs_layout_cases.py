"""The runs behind tests/golden/pgs_lds_layout_<task>.npz: every task in ee
control on the one-lane step kernel, 130 envs (two full waves and a two-lane
tail) and 64 envs (one wave), env i seeded 12345 + i, 25 scripted steps that
load the gripper's contact slots and the objects' ground rows.

scripts/record_pgs_lds_fixtures.py records them (script=True: the actions
come from the policy below and are stored); tests/test_gpu_pgs_lds_layout.py
replays the stored actions and compares every array bit for bit."""
from __future__ import annotations

import os

import numpy as np

TASKS = ("push", "pick_and_place", "slide", "flip", "reach", "stack")
BATCHES = (130, 64)
STEPS = 25
RECORD_AT = (1, 25)
SEED = 12345
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WRID_ROW = 103  # PS_F_WRID: the gripper slots' packed ids, 5 bits per slot (0 = empty)


def fixture_path(task: str) -> str:
    return os.path.join(GOLDEN_DIR, f"pgs_lds_layout_{task}.npz")


def policy(task: str, s: int, ee: np.ndarray, obj: np.ndarray | None, adim: int) -> np.ndarray:
    """Actions [B, adim] of step s from the ee and object positions [B, 3].

    pick_and_place, stack: the descent, close and lift of
    scripts/grasp_success.py (above the cube, down to its centre, close,
    lift), with its phases shortened to fit 25 steps.
    push, slide, flip: drive the (closed) gripper into the object at the
    object's height.  reach: press the fingers onto the table."""
    a = np.zeros((len(ee), adim), np.float32)
    if task in ("pick_and_place", "stack"):
        tgt = obj.copy()
        grip = np.ones(len(ee))
        if s < 7:
            tgt[:, 2] += 0.06
        elif s < 13:
            pass
        elif s < 19:
            grip[:] = -1.0
        else:
            tgt[:, 2] = 0.15
            grip[:] = -1.0
        a[:, :3] = np.clip(10.0 * (tgt - ee), -1, 1)
        a[:, 3] = grip
    elif task == "reach":
        tgt = ee.copy()
        tgt[:, 2] = -0.05
        a[:, :3] = np.clip(10.0 * (tgt - ee), -1, 1)
    else:
        a[:, :3] = np.clip(10.0 * (obj - ee), -1, 1)
        if adim > 3:
            a[:, 3] = -1.0
    return a


def snapshot(env, out) -> dict:
    """The whole state of the batch and what step() returned, as numpy arrays."""
    B = env.num_envs
    obs, r, te, tr, info = out
    return {
        "f": env.sim.f[:, :B].cpu().numpy(), "goal": env.sim.goal[:, :B].cpu().numpy(),
        "rng": env.sim.rng[:, :B].cpu().numpy(), "elapsed": env.sim.elapsed[:B].cpu().numpy(),
        "observation": obs["observation"].cpu().numpy(), "achieved_goal": obs["achieved_goal"].cpu().numpy(),
        "desired_goal": obs["desired_goal"].cpu().numpy(), "reward": r.cpu().numpy(),
        "terminated": te.cpu().numpy(), "truncated": tr.cpu().numpy(), "is_success": info["is_success"].cpu().numpy(),
    }


def run_case(task: str, B: int, actions: np.ndarray | None = None):
    """Steps `task` x B for STEPS steps.  actions None: scripted (recorded and
    returned); else replayed.  Returns ({"s<k>_<name>": array}, actions
    [STEPS, B, adim], slots-in-use count per step [STEPS, B])."""
    import torch

    from pandasim.envs import PandaVecEnv

    env = PandaVecEnv(task, "sparse", "ee", B, "cuda", autoreset=False, lanes_per_env=1)
    assert env.lanes_per_env == 1
    env.reset(seed=SEED)
    scripted = actions is None
    if scripted:
        actions = np.zeros((STEPS, B, env.action_dim), np.float32)
    name = {"reach": None, "stack": "object1"}.get(task, "object")
    arrays, used = {}, np.zeros((STEPS, B), np.int64)
    for s in range(STEPS):
        if scripted:
            ee = env.sim.get_link_position("panda", 11).double().cpu().numpy()
            obj = env.sim.get_base_position(name).double().cpu().numpy() if name else None
            actions[s] = policy(task, s, ee, obj, env.action_dim)
        out = env.step(torch.from_numpy(actions[s]).cuda())
        pack = env.sim.f[WRID_ROW, :B].cpu().numpy().astype(np.int64)
        used[s] = sum(((pack >> (5 * k)) & 31) != 0 for k in range(4))
        if s + 1 in RECORD_AT:
            for k, v in snapshot(env, out).items():
                arrays[f"s{s + 1}_{k}"] = v
    env.close()
    return arrays, actions, used


def bits(a: np.ndarray) -> np.ndarray:
    """The array's bytes, so that a comparison is bit for bit (NaNs, -0.0)."""
    return np.ascontiguousarray(a).view(np.uint8)
