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


# ------------------------------------------------ camera-image tests
# The scenes of tests/test_gpu_render_image.py, whose coverage conditions
# tests/test_render_cpu.py evaluates with the oracle alone.
RENDER_W, RENDER_H, RENDER_B = 64, 48, 3
RENDER_TASKS = ("reach", "push", "slide", "stack")
MIN_STABLE_SHARE, MIN_CASE_PIXELS = 0.70, 20
ROLE_NAMES = ("plane", "table", "object1", "object2", "target1", "target2", "robot", "background")
# one colour per role, all different (object 2 is not object 1's colour, ghost 1 not ghost 0's)
RENDER_RGBA = {"plane": (0.15, 0.2, 0.25, 1.0), "table": (0.95, 0.9, 0.85, 1.0), "object1": (0.1, 0.9, 0.2, 1.0),
               "object2": (0.2, 0.1, 0.9, 1.0), "target1": (0.92, 0.12, 0.31, 0.3), "target2": (0.13, 0.62, 0.88, 0.5),
               "robot": (0.9, 0.8, 0.3, 1.0), "background": (0.78, 0.85, 0.92, 1.0)}
SHAPE_BOX, SHAPE_CYLINDER, VISUAL_SPHERE = 0, 1, 2
OBJECT_AT = np.array([0.05, 0.22, 0.15])  # where the objects and ghosts gather, away from the arm


class RenderVisual:
    """ps_visual's fields as plain arrays of fp32 values (pandasim._lib.Visual on the GPU side)."""

    def __init__(self, shapes, halves, rgba=None, alphas=None):
        cols = dict(RENDER_RGBA if rgba is None else rgba)
        self.rgba = f32([cols[r] for r in ROLE_NAMES])
        if alphas is not None:
            self.rgba[4, 3], self.rgba[5, 3] = f32(alphas)
        self.target_shape = [int(s) for s in shapes]
        self.target_half = f32(halves)


def render_camera(cam, width=RENDER_W, height=RENDER_H):
    import render_oracle as RO

    view, proj, _ = RO.camera(cam["target"], cam["distance"], cam["yaw"], cam["pitch"], cam["roll"], width, height)
    return view, proj


def _random_unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


class RenderScene:
    """One task's fixture: B = 3 states (joints spread over their ranges,
    fingers open and closed, objects lifted with random orientations), a
    ps_visual, ghost poses, the cameras and the cases the scene must show."""

    def __init__(self, task):
        import oracle as O

        self.task = task
        rng = np.random.default_rng(100 + RENDER_TASKS.index(task))
        self.q = f32([[-0.9, 0.41, 0.0, -1.85, 0.0, 2.26, 0.79, 0.04, 0.04],
                      [1.2, -0.8, -1.0, -2.4, 1.5, 1.2, -1.5, 0.0, 0.0],
                      [-2.0, 1.2, 2.0, -0.6, -2.0, 3.2, 2.2, 0.02, 0.035]])
        assert np.all(self.q >= f32(DOF_LO) - 1e-6) and np.all(self.q <= f32(DOF_HI) + 1e-6)
        B = RENDER_B
        self.n_objects = {"reach": 0, "push": 1, "slide": 1, "stack": 2}[task]
        self.obj_pos = np.zeros((B, 2, 3))
        self.obj_pos[:, 0] = OBJECT_AT + np.array([[0.0, 0.0, -0.03], [0.02, -0.01, 0.0], [-0.01, 0.02, 0.04]])
        self.obj_pos[:, 1] = self.obj_pos[:, 0] + np.array([[0.08, 0.02, 0.03], [-0.07, 0.05, -0.02], [0.03, -0.08, 0.02]])
        self.obj_pos = f32(self.obj_pos)
        self.obj_quat = f32(_random_unit_quats(rng, B * 2).reshape(B, 2, 4))
        cfg = O.config(task)
        half = [float(np.float32(cfg.object_half[k])) for k in range(3)]
        ghosts = {"reach": ((VISUAL_SPHERE, SHAPE_BOX), ([0.05, 0.0, 0.0], [0.05, 0.03, 0.02])),
                  "push": ((SHAPE_BOX, SHAPE_CYLINDER), ([0.03, 0.04, 0.02], [0.035, 0.0, 0.06])),
                  "slide": ((SHAPE_CYLINDER, VISUAL_SPHERE), ([0.05, 0.0, 0.015], [0.045, 0.0, 0.0])),
                  "stack": ((SHAPE_BOX, SHAPE_BOX), (half, [0.05, 0.02, 0.04]))}[task]
        self.visual = RenderVisual(*ghosts)
        # ghost 0 between the close cameras and the object, sticking out over whatever is behind;
        # ghost 1 overlapping ghost 0 (env 0), under the table top (env 1), off to the side (env 2)
        t = np.zeros((B, 2, 7))
        toward = np.array([0.26, -0.72, 0.64])  # from the objects to the "object_above" camera
        t[:, 0, :3] = self.obj_pos[:, 0] + 0.05 * toward + np.array([[0.02, 0.0, 0.01], [-0.02, 0.01, 0.0], [0.0, 0.02, -0.015]])
        t[:, 1, :3] = [t[0, 0, :3] + [0.04, 0.01, 0.03], [OBJECT_AT[0], OBJECT_AT[1], -0.08], OBJECT_AT + [-0.12, 0.05, 0.1]]
        t[:, :, 3:] = _random_unit_quats(rng, B * 2).reshape(B, 2, 4)
        self.targets = f32(t)
        at = tuple(float(x) for x in OBJECT_AT)
        self.cameras = [
            dict(name="overview", target=(0.0, 0.0, 0.1), distance=1.0, yaw=45, pitch=-30, roll=30),
            dict(name="side", target=(-0.3, 0.0, 0.3), distance=0.9, yaw=100, pitch=-20, roll=90),
            dict(name="down", target=(-0.2, 0.1, 0.0), distance=0.9, yaw=0, pitch=-90, roll=0),
            dict(name="closeup", target=(-0.45, 0.0, 0.4), distance=0.35, yaw=120, pitch=-25, roll=0),
            dict(name="object_above", target=at, distance=0.2, yaw=20, pitch=-40, roll=0),
            dict(name="object_below", target=at, distance=0.22, yaw=200, pitch=25, roll=0),
            dict(name="object_left", target=at, distance=0.22, yaw=110, pitch=-5, roll=0),
            dict(name="object_right", target=at, distance=0.2, yaw=290, pitch=-65, roll=0),
            dict(name="object_back", target=at, distance=0.2, yaw=330, pitch=10, roll=0),
        ]
        self.closeup = 3
        R = self._role_case
        self.cases = {"plane": R(0), "table": R(1), "robot": R(6), "background": R(7),
                      "ghost 0 over background": lambda im: im["ghost"][..., 0] & (im["role"] == 7),
                      "ghost 1 over background": lambda im: im["ghost"][..., 1] & (im["role"] == 7),
                      "ghost 1 over table": lambda im: im["ghost"][..., 1] & (im["role"] == 1),
                      "ghost 0 over ghost 1": lambda im: im["ghost"][..., 0] & im["ghost"][..., 1],
                      "ghost 0 alone": lambda im: im["ghost"][..., 0] & ~im["ghost"][..., 1],
                      "ghost 1 alone": lambda im: im["ghost"][..., 1] & ~im["ghost"][..., 0],
                      "ghost 1 behind the table": lambda im: (np.isfinite(im["ghost_t"][..., 1]) & ~im["ghost"][..., 1]
                                                              & (im["role"] == 1))}
        if self.n_objects:
            self.cases["object 1"] = R(2)
            self.cases["ghost 0 over object"] = lambda im: im["ghost"][..., 0] & (im["role"] == 2)
            self.cases["ghost 0 behind object"] = lambda im: (np.isfinite(im["ghost_t"][..., 0]) & ~im["ghost"][..., 0]
                                                              & (im["role"] == 2))
            faces = ("side", "cap -z", "cap +z") if task == "slide" else ("+x", "-x", "+y", "-y", "+z", "-z")
            for k, name in enumerate(faces):
                self.cases[f"object 1 face {name}"] = (lambda k: lambda im: (im["role"] == 2) & (im["face"] == k))(k)
        if self.n_objects == 2:
            self.cases["object 2"] = R(3)

    @staticmethod
    def _role_case(role):
        return lambda im: im["role"] == role

    def oracle_cfg(self):
        """The oracle's Config of the task with the fp32 values the HIP path holds."""
        import oracle as O

        cfg = O.config(self.task)
        for k in range(3):
            cfg.base[k], cfg.object_half[k] = float(np.float32(cfg.base[k])), float(np.float32(cfg.object_half[k]))
        for name in ("table_cx", "table_hx", "table_hy"):
            setattr(cfg, name, float(np.float32(getattr(cfg, name))))
        return cfg

    def oracle_env(self, cfg, i):
        env = oracle_env_with(cfg, self.q[i])
        for b in range(2):
            for k in range(3):
                env.obj[b].pos[k] = self.obj_pos[i, b, k]
            for k in range(4):
                env.obj[b].quat[k] = self.obj_quat[i, b, k]
        return env

    def oracle_images(self, cam, width=RENDER_W, height=RENDER_H, visual=None, targets=None):
        """raycast_image of every env through one of self.cameras (or a camera dict)."""
        import render_oracle as RO

        cfg = self.oracle_cfg()
        view, proj = render_camera(cam, width, height)
        visual = self.visual if visual is None else visual
        targets = self.targets if targets is None else targets
        return [RO.raycast_image(cfg, self.oracle_env(cfg, i), view, proj, width, height, visual, targets[i])
                for i in range(RENDER_B)]

    def straddles_near(self, cam, i, near=0.1):
        """Arm primitives of env i whose bounding sphere reaches in front of the near plane of the camera."""
        import render_oracle as RO

        cfg = self.oracle_cfg()
        caps, sph = RO.scene_primitives(cfg, self.oracle_env(cfg, i))
        view, _ = render_camera(cam)
        V = np.asarray(view, np.float64).reshape(4, 4, order="F")
        eye, f = -V[:3, :3].T @ V[:3, 3], -V[2, :3]
        balls = [((a + b) / 2, np.linalg.norm(b - a) / 2 + r) for a, b, r in caps] + list(sph)
        return sum(1 for c, r in balls if (c - eye) @ f - r <= near < (c - eye) @ f + r)


# ghost tests (push scene): every shape in both slots, box and cylinder with their random poses; the
# cylinder's radius and half height differ, and so do all three half extents of the box
GHOST_VARIANTS = {"box+cylinder": ((SHAPE_BOX, SHAPE_CYLINDER), ([0.03, 0.04, 0.02], [0.035, 0.0, 0.06])),
                  "sphere+box": ((VISUAL_SPHERE, SHAPE_BOX), ([0.045, 0.0, 0.0], [0.05, 0.02, 0.035])),
                  "cylinder+sphere": ((SHAPE_CYLINDER, VISUAL_SPHERE), ([0.05, 0.0, 0.015], [0.045, 0.0, 0.0]))}
GHOST_ALPHAS = ((0.3, 0.5), (0.0, 0.0), (1.0, 1.0), (0.3, 1.0), (1.0, 0.3))
GHOST_CAMERAS = ("down", "object_above", "object_below", "object_left", "object_right", "object_back")
GHOST_CASES = ("ghost 0 over background", "ghost 0 over object", "ghost 0 behind object", "ghost 1 behind the table",
               "ghost 0 over ghost 1", "ghost 0 alone", "ghost 1 alone")
# image shapes that change how a 256-pixel tile maps onto rows, and the cameras that spread the arm over many tiles
TILING_SHAPES = ((256, 8), (300, 7), (16, 160), (50, 37), (7, 5))
TILING_CAMERAS = ("side", "closeup",
                  dict(name="arm_column", target=(-0.6, 0.0, 0.3), distance=0.3, yaw=90, pitch=-10, roll=90),
                  dict(name="arm_upper", target=(-0.55, 0.0, 0.45), distance=0.25, yaw=0, pitch=-20, roll=90),
                  dict(name="arm_many", target=(-0.5, 0.0, 0.5), distance=0.3, yaw=180, pitch=-30, roll=0))
MIN_TILING_ROBOT_PIXELS = {(7, 5): 5}  # stable robot pixels over the cameras and envs; 20 at every other shape

_scenes = {}


def render_scene(task):
    if task not in _scenes:
        _scenes[task] = RenderScene(task)
    return _scenes[task]


def check_render_coverage(scene, images_by_camera):
    """The coverage conditions of a scene on its oracle images {camera name:
    [image of env 0, 1, 2]}: the stable share of every image, the stable pixel
    count of every case over the camera set.  -> (shares, counts)."""
    shares = {(name, i): float(im["stable"].mean()) for name, ims in images_by_camera.items() for i, im in enumerate(ims)}
    counts = {case: int(sum((pred(im) & im["stable"]).sum() for ims in images_by_camera.values() for im in ims))
              for case, pred in scene.cases.items()}
    low = {k: round(v, 3) for k, v in shares.items() if v < MIN_STABLE_SHARE}
    few = {k: v for k, v in counts.items() if v < MIN_CASE_PIXELS}
    assert not low, (scene.task, "stable share below 70 %", low)
    assert not few, (scene.task, "cases with fewer than 20 stable pixels", few)
    return shares, counts


def quat_err(a, b, same_sign=None):
    """max-component error [n] of quaternions a against b [n, 4], up to sign
    (q and -q are one rotation); where same_sign [n] is set the sign must agree too."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, s = np.abs(a - b).max(-1), np.abs(a + b).max(-1)
    return np.minimum(d, s) if same_sign is None else np.where(same_sign, d, np.minimum(d, s))
