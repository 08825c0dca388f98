"""Shared helpers for the parity tests: move state between the HIP path's SoA
state buffer and the oracle's per-env structs."""
import numpy as np
import oracle as O

TASK_NAMES = ["reach", "push", "pick_and_place", "slide", "stack", "flip"]
OBJECT_ROWS = (63, 76)
# contact-cache rows (include/pandasim.h PS_F_WG0..PS_F_WPN)
WG_ROWS, WR_ROW, WP_ROW, WPPT_ROW, WPN_ROW = (89, 94), 99, 104, 108, 120


def unpack_ids(x):
    """Four 5-bit slot ids of a packed id row (sum id_k 32^k)."""
    v = int(x)
    return [(v >> (5 * k)) & 31 for k in range(4)]


def oracle_config_for(sim_cfg):
    """oracle.Config mirroring a pandasim _lib.Config."""
    cfg = O.config(TASK_NAMES[sim_cfg.task], control="ee" if sim_cfg.control == 0 else "joints",
                   reward="sparse" if sim_cfg.reward == 0 else "dense")
    cfg.block_gripper = sim_cfg.block_gripper
    cfg.has_table, cfg.has_plane = sim_cfg.has_table, sim_cfg.has_plane
    cfg.n_objects, cfg.object_shape = sim_cfg.n_objects, sim_cfg.object_shape
    for k in range(3):
        cfg.base[k] = float(np.float32(sim_cfg.base[k]))
        cfg.object_half[k] = float(np.float32(sim_cfg.object_half[k]))
    for name in ("object_mass", "object2_mass", "object_friction", "table_cx", "table_hx", "table_hy"):
        setattr(cfg, name, float(np.float32(getattr(sim_cfg, name))))
    return cfg


def snapshot(sim):
    """Host copy of the whole batched state (numpy)."""
    B = sim.num_envs
    return {
        "f": sim.f[:, :B].double().cpu().numpy(),
        "goal": sim.goal[:, :B].cpu().numpy(),
        "rng": sim.rng[:, :B].cpu().numpy().view(np.uint64),
        "elapsed": sim.elapsed[:B].cpu().numpy(),
    }


def oracle_env_from(cfg, snap, i):
    env = O.new_env(cfg)
    f = snap["f"][:, i]
    for d in range(9):
        env.q[d], env.qd[d] = f[d], f[9 + d]
        env.m_target[d], env.m_kp[d], env.m_kd[d] = f[18 + d], f[27 + d], f[36 + d]
        env.m_vel[d], env.m_maximp[d] = f[45 + d], f[54 + d]
    for b, r in enumerate(OBJECT_ROWS):
        o = env.obj[b]
        for k in range(3):
            o.pos[k], o.vel[k], o.omg[k] = f[r + k], f[r + 7 + k], f[r + 10 + k]
        for k in range(4):
            o.quat[k] = f[r + 3 + k]
    for k in range(snap["goal"].shape[0]):
        env.goal[k] = snap["goal"][k, i]
    for k in range(snap["rng"].shape[0]):
        env.rng[k] = int(snap["rng"][k, i])
    env.elapsed = int(snap["elapsed"][i])
    k = env.cache
    for b, r in enumerate(WG_ROWS):
        for s, idv in enumerate(unpack_ids(f[r + 4])):
            k.ground_lam[b][s], k.ground_id[b][s] = f[r + s], idv
    for s, idv in enumerate(unpack_ids(f[WR_ROW + 4])):
        k.robot_lam[s], k.robot_id[s] = f[WR_ROW + s], idv
    for s in range(4):
        k.pair_lam[s] = f[WP_ROW + s]
        for j in range(3):
            k.pair_pt[s][j] = f[WPPT_ROW + 3 * s + j]
    k.pair_n = int(f[WPN_ROW])
    return env


# ------------------------------------------------ engine-level query tests
# joint limits per DoF (include/panda_model.h PM_DOF_TABLE): arm 0..6, fingers 7, 8
DOF_LO = np.array([-2.9671, -1.8326, -2.9671, -3.0718, -2.9671, -0.0175, -2.9671, 0.0, 0.0])
DOF_HI = np.array([2.9671, 1.8326, 2.9671, -0.0698, 2.9671, 3.7525, 2.9671, 0.04, 0.04])
NUM_LINKS = 12
NEUTRAL_Q = np.array([0.0, 0.41, 0.0, -1.85, 0.0, 2.26, 0.79, 0.0, 0.0])  # panda.py:36


def f32(x):
    """x rounded to fp32, as float64 (what the state buffer and the C ABI's float arguments hold)."""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def link_sample(n=256, seed=0):
    """(q, qd) [n, 9], rounded to fp32: arm joints U(-2.8, 2.8), fingers
    U(0, 0.04), arm velocities U(-2, 2), finger velocities U(-0.2, 0.2).
    With n = 256, seed = 0 the link orientations reach every branch of
    btMatrix3x3::getRotation on every link >= 1 (tests/test_oracle.py)."""
    rng = np.random.default_rng(seed)
    q, qd = np.zeros((n, 9)), np.zeros((n, 9))
    for i in range(n):  # one configuration at a time: a longer sample starts with a shorter one
        q[i] = np.concatenate([rng.uniform(-2.8, 2.8, 7), rng.uniform(0.0, 0.04, 2)])
        qd[i] = np.concatenate([rng.uniform(-2.0, 2.0, 7), rng.uniform(-0.2, 0.2, 2)])
    return f32(q), f32(qd)


def oracle_env_with(cfg, q, qd=None):
    """A fresh oracle env with the given joint positions (and velocities)."""
    env = O.new_env(cfg)
    for d in range(9):
        env.q[d] = float(q[d])
        env.qd[d] = 0.0 if qd is None else float(qd[d])
    return env


def oracle_link_states(cfg, q, qd, link):
    """O.link_state of every row of q/qd [n, 9] -> pos [n, 3], quat [n, 4], v [n, 3], w [n, 3]."""
    out = [O.link_state(cfg, oracle_env_with(cfg, q[i], qd[i]), link) for i in range(len(q))]
    return tuple(np.array([o[k] for o in out]) for k in range(4))


def quat_to_matrix(q):
    """Rotation matrices [..., 3, 3] of quaternions [..., 4] (x, y, z, w), normalised first."""
    q = np.asarray(q, np.float64)
    x, y, z, w = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def rotation_branch(R):
    """Branch of btMatrix3x3::getRotation that each matrix of R [..., 3, 3]
    takes (3: trace > 0; else i = 0, 1, 2, the largest diagonal entry as Bullet
    compares them) and how far its predicates are from switching: |trace|, and
    below zero also the smallest difference of two diagonal entries."""
    R = np.asarray(R, np.float64)
    m0, m4, m8 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    tr = m0 + m4 + m8
    i = np.where(m0 < m4, np.where(m4 < m8, 2, 1), np.where(m0 < m8, 2, 0))
    branch = np.where(tr > 0.0, 3, i)
    diag = np.minimum(np.minimum(np.abs(m0 - m4), np.abs(m4 - m8)), np.abs(m0 - m8))
    margin = np.where(tr > 0.0, np.abs(tr), np.minimum(np.abs(tr), diag))
    return branch, margin


def quat_err(a, b, same_sign=None):
    """max-component error [n] of quaternions a against b [n, 4], up to sign
    (q and -q are one rotation); where same_sign [n] is set the sign must agree too."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, s = np.abs(a - b).max(-1), np.abs(a + b).max(-1)
    return np.minimum(d, s) if same_sign is None else np.where(same_sign, d, np.minimum(d, s))
