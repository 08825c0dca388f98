"""Batched counterpart of panda_gym.pybullet.PyBullet (pybullet.py:16-799).

``PandaSim`` owns one structure-of-arrays state buffer (a torch uint8 tensor on
the GPU) for B identical scenes and exposes the subset of the PyBullet wrapper
that the Robot/Task plugins of the hot path call, each method acting on all B
scenes at once.  Compute goes through libpandasim.so (HIP, gfx950); simple
field reads/writes are tensor views of the state buffer.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._lib import _ptr
from .cloudnet import CloudNet

TASKS = {"reach": 0, "push": 1, "pick_and_place": 2, "slide": 3, "stack": 4, "flip": 5}
CONTROLS = {"ee": 0, "joints": 1}
REWARDS = {"sparse": 0, "dense": 1}
JOINT_TO_DOF = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 9: 7, 10: 8}
DT_SUBSTEP = 1.0 / 500
# the four views around the table that the grasp task merges (task_classes/grasp.py:129-132)
GRASP_VIEWS = tuple(dict(distance=0.6, target_position=[0, 0, 0.1], yaw=yaw) for yaw in (0, 135, 245, 300))


class PandaSim(CloudNet):
    """B Panda scenes on one GPU (one process per GPU).  The
    PointNet++ layer over point_cloud()'s observation is the CloudNet mixin."""

    def __init__(self, task: str = "reach", control_type: str = "ee", reward_type: str = "sparse", num_envs: int = 1,
                 device="cuda", n_substeps: int = 20, config: Optional[L.Config] = None):
        if not torch.cuda.is_available():
            raise L.PandasimError("PandaSim needs a ROCm GPU (there is no CPU fallback)")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.n_substeps = int(n_substeps)
        if config is not None:
            self.cfg = config
        elif task is None:
            # empty world, built up by loadURDF/create_* as PyBullet() + Robot/Task constructors do
            self.cfg = L.default_config(0, 0, 0)
            self.cfg.has_table = self.cfg.has_plane = self.cfg.n_objects = 0
            self.cfg.base[0] = 0.0
        else:
            self.cfg = L.default_config(TASKS[task], CONTROLS[control_type], REWARDS[reward_type])
        self._lib = L.lib()
        self._ctx = None
        self._create_ctx()
        # body name -> kind ("robot", "object", "ghost"); objects -> their index
        self._bodies: Dict[str, str] = {"panda": "robot"}
        self.finger_spinning_friction = 0.0  # panda.py:49-50 sets 0.001 (set_spinning_friction)
        self._objects: Dict[str, int] = {}
        names = {0: [], 1: ["object"], 2: ["object1", "object2"]}[self.cfg.n_objects]
        for k, name in enumerate(names):
            self._bodies[name] = "object"
            self._objects[name] = k
        self._ghost_pos: Dict[str, torch.Tensor] = {}
        self._ghost_orn: Dict[str, torch.Tensor] = {}
        # visual-only properties of created bodies (rgba, ghost shape): rendering
        self._rgba: Dict[str, np.ndarray] = {}
        self._ghost_shape: Dict[str, tuple] = {}
        self.layout = L.layout(self.num_envs)
        self.state = torch.zeros(self.layout.total_bytes, dtype=torch.uint8, device=self.device)
        self._bind_views()
        self._saved: Dict[int, torch.Tensor] = {}
        self._ids = itertools.count()
        self._call("ps_init_state", self._ctx, _ptr(self.state), self._stream())

    # ---------------------------------------------------------------- plumbing
    def _create_ctx(self):
        """(Re)create the context for the current scene config.  The state
        buffer's layout depends only on num_envs, so the state survives."""
        if self._ctx:
            self._lib.ps_destroy(self._ctx)
            self._ctx = None
        ctx = C.c_void_p()
        L.check(self._lib.ps_create(C.byref(self.cfg), self.num_envs, self.device.index, C.byref(ctx)),
                what="ps_create")
        self._ctx = ctx

    def _bind_views(self):
        lay, s = self.layout, self.state
        n = lay.stride
        self.f = s[lay.float_offset:lay.float_offset + L.NUM_FLOAT_ROWS * n * 4].view(torch.float32).view(
            L.NUM_FLOAT_ROWS, n)
        self.goal = s[lay.goal_offset:lay.goal_offset + L.MAX_GOAL_DIM * n * 8].view(torch.float64).view(
            L.MAX_GOAL_DIM, n)
        self.rng = s[lay.rng_offset:lay.rng_offset + L.NUM_RNG_ROWS * n * 8].view(torch.int64).view(L.NUM_RNG_ROWS, n)
        self.elapsed = s[lay.elapsed_offset:lay.elapsed_offset + n * 4].view(torch.int32)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name: str, *args):
        with torch.cuda.device(self.device):
            rc = getattr(self._lib, name)(*args)
        L.check(rc, self._ctx, name)

    def rows(self, row: int, count: int) -> torch.Tensor:
        """[B, count] view-copy of float rows (env-major)."""
        return self.f[row:row + count, :self.num_envs].t()

    def set_rows(self, row: int, values: torch.Tensor) -> None:
        values = torch.as_tensor(values, dtype=torch.float32, device=self.device)
        if values.dim() == 1:
            values = values.unsqueeze(0).expand(self.num_envs, -1)
        self.f[row:row + values.shape[1], :self.num_envs] = values.t()

    @property
    def obs_dim(self) -> int:
        return self._lib.ps_obs_dim(self._ctx)

    @property
    def action_dim(self) -> int:
        return self._lib.ps_action_dim(self._ctx)

    @property
    def goal_dim(self) -> int:
        return self._lib.ps_goal_dim(self._ctx)

    @property
    def max_episode_steps(self) -> int:
        return self._lib.ps_max_episode_steps(self._ctx)

    def goals(self) -> torch.Tensor:
        """[B, goal_dim] float64 view-copy of the fused path's goals."""
        return self.goal[:self.goal_dim, :self.num_envs].t()

    @property
    def dt(self) -> float:
        """pybullet.py:47-50: timestep * n_substeps (0.04 s)."""
        return DT_SUBSTEP * self.n_substeps

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.ps_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------- scene construction
    # pybullet.py:507-799.  The scene is compiled into the kernels
    # (include/panda_model.h): these calls accept exactly the bodies of the
    # Reach/Push/PickAndPlace scenes and raise NotImplementedError otherwise.
    @contextlib.contextmanager
    def no_rendering(self):
        """pybullet.py:502-507: GUI rendering toggle; images come from render()."""
        yield

    def place_visualizer(self, target_position=None, distance=None, yaw=None, pitch=None) -> None:
        """pybullet.py:499-508: camera placement; no-op without rendering."""

    def loadURDF(self, body_name: str, fileName: str, basePosition=None, useFixedBase: bool = False,
                 **kwargs) -> None:
        """pybullet.py:522-529: only the fixed-base Franka Panda is modelled."""
        if not str(fileName).endswith("franka_panda/panda.urdf") or not useFixedBase:
            raise NotImplementedError(f"loadURDF({fileName!r}, useFixedBase={useFixedBase}): only the fixed-base "
                                      "franka_panda/panda.urdf is compiled in")
        base = [0.0, 0.0, 0.0] if basePosition is None else [float(x) for x in basePosition]
        for k in range(3):
            self.cfg.base[k] = base[k]
        self._bodies = {n: k for n, k in self._bodies.items() if k != "robot"}
        self._bodies[body_name] = "robot"
        self._create_ctx()

    def create_plane(self, z_offset: float) -> None:
        """pybullet.py:726-739."""
        if abs(z_offset - PLANE_Z) > 1e-12:
            raise NotImplementedError(f"create_plane(z_offset={z_offset}): only z_offset={PLANE_Z} is compiled in")
        self.cfg.has_plane = 1
        self._create_ctx()

    def create_table(self, length: float, width: float, height: float, x_offset: float = 0.0,
                     lateral_friction=None, spinning_friction=None) -> None:
        """pybullet.py:741-771: a static box with its top at z = 0 (default friction)."""
        if lateral_friction is not None or spinning_friction is not None:
            raise NotImplementedError("create_table: only the default table friction is compiled in")
        self.cfg.has_table = 1
        self.cfg.table_cx, self.cfg.table_hx, self.cfg.table_hy = float(x_offset), length / 2, width / 2
        self._create_ctx()

    def _add_object(self, body_name: str, shape: int, half, mass: float, lateral_friction, position) -> None:
        n = self.cfg.n_objects
        fric = 0.5 if lateral_friction is None else float(lateral_friction)
        if n >= 2 or mass <= 0:
            raise NotImplementedError("at most two dynamic objects (Stack) are compiled in")
        f32 = lambda v: [float(np.float32(x)) for x in v]  # the config holds float32
        if n == 1 and (shape != self.cfg.object_shape or f32(half) != list(self.cfg.object_half)
                       or f32([fric]) != [self.cfg.object_friction] or shape != L.SHAPE_BOX):
            raise NotImplementedError("a second object must be a cube like the first (Stack)")
        if shape == L.SHAPE_BOX and max(half) != min(half):
            raise NotImplementedError("boxes must be cubes (isotropic inertia)")
        self.cfg.object_shape = shape
        for k in range(3):
            self.cfg.object_half[k] = float(half[k])
        self.cfg.object_friction = fric
        if n == 0:
            self.cfg.object_mass = float(mass)
        else:
            self.cfg.object2_mass = float(mass)
        self.cfg.n_objects = n + 1
        # the fused-kernel task matching the scene (the plugin path ignores it)
        self.cfg.task = {1: TASKS["slide"] if shape == L.SHAPE_CYLINDER else TASKS["push"], 2: TASKS["stack"]}[n + 1]
        self._bodies[body_name] = "object"
        self._objects[body_name] = n
        self._create_ctx()
        self.set_base_pose(body_name, position, [0.0, 0.0, 0.0, 1.0])

    def create_box(self, body_name: str, half_extents, mass: float, position, rgba_color=None, specular_color=None,
                   ghost: bool = False, lateral_friction=None, spinning_friction=None, texture=None) -> None:
        """pybullet.py:516-582: a dynamic cube (Push/PickAndPlace/Flip; two for Stack) or a ghost marker."""
        self._note_visual(body_name, rgba_color, L.SHAPE_BOX, [float(x) for x in half_extents], ghost)
        if ghost:
            self._add_ghost(body_name, position)
            return
        if spinning_friction:
            raise NotImplementedError("create_box: torsional friction rows (non-zero object spinning friction) "
                                      "are not modelled")
        self._add_object(body_name, L.SHAPE_BOX, [float(x) for x in half_extents], mass, lateral_friction, position)

    def create_cylinder(self, body_name: str, radius: float, height: float, mass: float, position, rgba_color=None,
                        specular_color=None, ghost: bool = False, lateral_friction=None,
                        spinning_friction=None) -> None:
        """pybullet.py:584-623: the upright cylinder of Slide (axis z), or a ghost marker."""
        self._note_visual(body_name, rgba_color, L.SHAPE_CYLINDER, [radius, radius, height / 2], ghost)
        if ghost:
            self._add_ghost(body_name, position)
            return
        if spinning_friction:
            raise NotImplementedError("create_cylinder: torsional friction rows (non-zero object spinning "
                                      "friction) are not modelled")
        self._add_object(body_name, L.SHAPE_CYLINDER, [radius, radius, height / 2], mass, lateral_friction, position)

    def create_sphere(self, body_name: str, radius: float, mass: float, position, rgba_color=None,
                      specular_color=None, ghost: bool = False) -> None:
        """pybullet.py:665-693: ghost target markers only."""
        self._note_visual(body_name, rgba_color, L.VISUAL_SPHERE, [radius, radius, radius], ghost)
        if not ghost:
            raise NotImplementedError("create_sphere: only ghost spheres (targets) are supported")
        self._add_ghost(body_name, position)

    def set_lateral_friction(self, body: str, link: int, lateral_friction: float) -> None:
        """pybullet.py:773-785: the compiled-in gripper proxies carry panda.py:47-48's values."""
        if not (self._bodies.get(body) == "robot" and int(link) in (9, 10) and lateral_friction == 1.0):
            raise NotImplementedError("set_lateral_friction: only the Panda fingers' 1.0 is compiled in")

    def set_spinning_friction(self, body: str, link: int, spinning_friction: float) -> None:
        """pybullet.py:787-799.  A contact's torsional friction coefficient is the
        product of its two bodies' spinning frictions
        (btManifoldResult::calculateCombinedSpinningFriction); every body but
        the fingers keeps Bullet's default 0, so the fingers' value (panda.py:49-50)
        yields no torsional friction row in any contact of these scenes.  A
        non-zero value on another body would create such rows, which the kernels
        do not build: it raises."""
        kind = self._bodies.get(body)
        if kind == "robot" and int(link) in (9, 10):
            self.finger_spinning_friction = float(spinning_friction)
            return
        if kind in ("object", "robot") and float(spinning_friction) == 0.0:
            return
        raise NotImplementedError("set_spinning_friction: torsional friction rows (a non-zero spinning friction "
                                  "on a body other than the fingers) are not modelled")

    def _note_visual(self, body_name, rgba_color, shape, half, ghost) -> None:
        rgba = np.zeros(4) if rgba_color is None else np.asarray(rgba_color, np.float64)  # pybullet.py:536
        self._rgba[body_name] = rgba
        if ghost:
            self._ghost_shape[body_name] = (shape, [float(h) for h in half])

    def _add_ghost(self, body_name: str, position) -> None:
        self._bodies[body_name] = "ghost"
        self._ghost_pos[body_name] = torch.zeros(self.num_envs, 3, dtype=torch.float64, device=self.device)
        self._ghost_orn[body_name] = torch.zeros(self.num_envs, 4, dtype=torch.float64, device=self.device)
        self._ghost_orn[body_name][:, 3] = 1.0
        self.set_base_pose(body_name, position, [0.0, 0.0, 0.0, 1.0])

    def _kind(self, body: str) -> str:
        if body not in self._bodies:
            raise KeyError(f"unknown body {body!r}")
        return self._bodies[body]

    # ----------------------------------------------------- camera images
    # pybullet.py:69-264 (§8(f) rank 4).  Batched: one image per env.
    def get_cam2world_transforms(self, width: int = 480, height: int = 480, target_position=np.zeros(3),
                                 distance: float = 1.4, yaw: float = 45, pitch: float = -30, roll: float = 0):
        """pybullet.py:69-107: (view_matrix, proj_matrix) as pybullet's 16-float
        tuples and tran_pix_world = inv(P @ V) (4, 4) float64."""
        target_position = np.zeros(3) if target_position is None else target_position
        t = (C.c_float * 3)(*[float(x) for x in target_position])
        view, proj, tran = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_double * 16)()
        L.check(self._lib.ps_camera(t, float(distance), float(yaw), float(pitch), float(roll), int(width),
                                    int(height), view, proj, tran), what="ps_camera")
        return tuple(view[:]), tuple(proj[:]), np.array(tran[:], np.float64).reshape(4, 4)

    def _visual(self) -> L.Visual:
        """Colours by role and ghost-target shapes: from the create_* calls of
        the plugin path, else the registered task's _create_scene (tasks/*.py)."""
        v = L.Visual()
        cols = {"plane": (0.15, 0.15, 0.15, 1.0), "table": (0.95, 0.95, 0.95, 1.0), "robot": (0.9, 0.9, 0.92, 1.0),
                "background": (0.78, 0.85, 0.92, 1.0), "object1": (0.1, 0.9, 0.1, 1.0),
                "object2": (0.1, 0.9, 0.1, 1.0), "target1": (0.1, 0.9, 0.1, 0.3), "target2": (0.1, 0.9, 0.1, 0.3)}
        task = self.cfg.task
        half = [float(self.cfg.object_half[k]) for k in range(3)]
        shapes = [(L.SHAPE_BOX, half), (-1, [0.0] * 3)]
        if task == TASKS["reach"]:
            shapes[0] = (L.VISUAL_SPHERE, [0.02] * 3)  # reach.py:31-38
        elif task == TASKS["slide"]:
            shapes[0] = (L.SHAPE_CYLINDER, half)  # slide.py:43-51
        elif task == TASKS["stack"]:  # stack.py:33-61: blue object1/target1, green object2/target2
            cols.update(object1=(0.1, 0.1, 0.9, 1.0), target1=(0.1, 0.1, 0.9, 0.3))
            shapes[1] = (L.SHAPE_BOX, half)
        elif task == TASKS["flip"]:  # flip.py:33-47 (textured cube drawn in its mean colour)
            cols.update(object1=(0.55, 0.55, 0.55, 1.0), target1=(1.0, 1.0, 1.0, 0.5))
        objs = sorted(self._objects.items(), key=lambda kv: kv[1])
        for name, k in objs:
            if name in self._rgba:
                cols[f"object{k + 1}"] = tuple(self._rgba[name])
        ghosts = list(self._ghost_shape.items())
        if ghosts:
            shapes = [(-1, [0.0] * 3), (-1, [0.0] * 3)]
            for g, (name, (shape, h)) in enumerate(ghosts[:2]):
                shapes[g] = (shape, h)
                cols[f"target{g + 1}"] = tuple(self._rgba[name])
        for r, role in enumerate(L.ROLES):
            for k in range(4):
                v.rgba[r][k] = float(cols[role][k])
        for g in range(2):
            v.target_shape[g] = int(shapes[g][0])
            for k in range(3):
                v.target_half[g][k] = float(shapes[g][1][k])
        return v

    def _target_poses(self) -> torch.Tensor:
        """[B, 2, 7] f32 ghost-target poses: the plugin path's set_base_pose
        calls, else the fused path's goals as each task's reset places them
        (reach.py:49, push.py:72, stack.py:97-98, flip.py:66)."""
        B = self.num_envs
        out = torch.zeros(B, 2, 7, dtype=torch.float32, device=self.device)
        out[:, :, 6] = 1.0
        out[:, :, 2] = -100.0
        names = list(self._ghost_shape)[:2]
        if names:
            for g, n in enumerate(names):
                out[:, g, :3] = self._ghost_pos[n].float()
                out[:, g, 3:] = self._ghost_orn[n].float()
            return out
        goals = self.goals().float()
        if self.cfg.task == TASKS["flip"]:
            out[:, 0, :3] = torch.tensor([0.0, 0.0, 3 * 0.04 / 2], device=self.device)
            out[:, 0, 3:] = goals[:, :4]
        else:
            out[:, 0, :3] = goals[:, :3]
            if self.cfg.task == TASKS["stack"]:
                out[:, 1, :3] = goals[:, 3:6]
        return out

    @staticmethod
    def _check_image_size(width: int, height: int) -> None:
        # render() builds its NDC grid with np.mgrid[-1:1:2/n], whose length is
        # ceil(2 / (2/n)): for some n that is n + 1 and the reference's
        # np.stack of the grid with the depth buffer raises
        for n in (width, height):
            if int(math.ceil(2.0 / (2.0 / n))) != n:
                raise ValueError(f"render: np.mgrid[-1:1:2/{n}] has {int(math.ceil(2.0 / (2.0 / n)))} entries, not "
                                 f"{n}; the reference's deprojection cannot stack it with a {n}-pixel axis")

    def get_camera_image(self, width: int, height: int, view_matrix, proj_matrix, rgb: bool = True):
        """getCameraImage (pybullet.py:186-192) of every env: depth [B, h, w]
        f32 (OpenGL window depth) and rgb [B, h, w, 3] u8 (RGB order)."""
        B = self.num_envs
        depth = torch.empty(B, height, width, dtype=torch.float32, device=self.device)
        img = torch.empty(B, height, width, 3, dtype=torch.uint8, device=self.device) if rgb else None
        view = (C.c_float * 16)(*[float(x) for x in view_matrix])
        proj = (C.c_float * 16)(*[float(x) for x in proj_matrix])
        vis = self._visual()
        targets = self._target_poses().contiguous()
        self._call("ps_render", self._ctx, _ptr(self.state), view, proj, int(width), int(height), C.byref(vis),
                   _ptr(targets), _ptr(depth), _ptr(img), self._stream())
        return depth, img

    def render(self, width: int = 480, height: int = 480, target_position=np.zeros(3), distance: float = 1.4,
               yaw: float = 45, pitch: float = -30, roll: float = 0, waypoints=None, env: Optional[int] = None):
        """PyBullet.render (pybullet.py:149-264) for every env.

        env=None: a dict of batched tensors -- rgb [B, h, w, 3] u8 (channels
        swapped as the reference's cv2.cvtColor(BGR2RGB) of pybullet's RGBA
        leaves them), depth [B, h, w] f32, points [B, h*w, 3] f64, valid
        [B, h*w] bool (the reference keeps points[valid[b]] in pixel order),
        colors [B, h*w, 3] u8, pixels_2d [B, h*w, 2] f64, waypoints_proj.
        env=i: the reference's tuple (rgb, depth, points, colors, pixels_2d,
        waypoints_proj) of env i as numpy arrays."""
        self._check_image_size(width, height)
        view, proj, tran = self.get_cam2world_transforms(width, height, target_position, distance, yaw, pitch, roll)
        depth, img = self.get_camera_image(width, height, view, proj)
        B, n = self.num_envs, width * height
        points = torch.empty(B, n, 3, dtype=torch.float64, device=self.device)
        valid = torch.empty(B, n, dtype=torch.uint8, device=self.device)
        pix2d = torch.empty(B, n, 2, dtype=torch.float64, device=self.device)
        T = (C.c_double * 16)(*tran.reshape(-1).tolist())
        self._call("ps_deproject_image", self._ctx, _ptr(depth), T, int(width), int(height), _ptr(points),
                   _ptr(valid), _ptr(pix2d), self._stream())
        waypoints_proj = []
        if waypoints is not None:
            PV = np.matmul(np.asarray(proj).reshape([4, 4], order="F"), np.asarray(view).reshape([4, 4], order="F"))
            for point in waypoints:
                x, y, z, w = np.matmul(PV, np.array([point[0], point[1], point[2], 1]))
                x, y = (x / w + 1) / 2 * width, (y / w + 1) / 2 * height
                waypoints_proj.append([int(x), int(height - y)])
        out = {"rgb": img.flip(-1), "depth": depth, "points": points, "valid": valid.bool(),
               "colors": img.reshape(B, n, 3), "pixels_2d": pix2d, "waypoints_proj": waypoints_proj}
        if env is None:
            return out
        keep = out["valid"][env].cpu().numpy()
        return (out["rgb"][env].cpu().numpy(), out["depth"][env].double().cpu().numpy(),
                out["points"][env].cpu().numpy()[keep], out["colors"][env].cpu().numpy()[keep],
                out["pixels_2d"][env].cpu().numpy()[keep], waypoints_proj)

    def point_cloud(self, views=None, n_points: int = 5000, width: int = 480, height: int = 480, seed: int = 0,
                    crop=None) -> Dict[str, torch.Tensor]:
        """The policies' observation (grasp.py:122-137, generate_dset.py:148-195,
        334): render() from every view, np.vstack of the filtered point
        clouds, an optional crop, np.random.choice(len(points), n_points) --
        fused (ps_point_cloud), for every env, without the per-pixel arrays.

        views: a list of dicts of get_cam2world_transforms' keyword arguments
        (default GRASP_VIEWS); crop: ((lo x, y, z), (hi x, y, z)), an extra
        open box on the world point.  Returns points [B, K, 3] f32, colors
        [B, K, 3] u8 (render()'s colors), source [B, K] i32 (view * width *
        height + pixel of each sample) and count [B] i32 (the merged cloud's
        size; an env with none gets points 0, colors 0, source -1).  The draw
        is a counter-based splitmix64 of `seed`: the same seed repeats it."""
        self._check_image_size(width, height)
        views = GRASP_VIEWS if views is None else list(views)
        if not 1 <= len(views) <= L.CLOUD_MAX_VIEWS:
            raise ValueError(f"point_cloud: {len(views)} views (1 to {L.CLOUD_MAX_VIEWS})")
        if n_points < 1:
            raise ValueError("point_cloud: n_points < 1")
        B, K = self.num_envs, int(n_points)
        cv = (L.CloudView * len(views))()
        for v, kw in zip(cv, views):
            view, proj, tran = self.get_cam2world_transforms(width, height, **kw)
            v.view[:], v.proj[:], v.tran_pix_world[:] = view, proj, tran.reshape(-1).tolist()
        box = None
        if crop is not None:
            box = L.CloudCrop()
            box.lo[:], box.hi[:] = [float(x) for x in crop[0]], [float(x) for x in crop[1]]
        nbytes = self._lib.ps_cloud_workspace_bytes(B, len(views), int(width), int(height))
        if nbytes < 0:
            raise ValueError(f"point_cloud: {len(views)} views of {width}x{height} are more than one call takes")
        ws = getattr(self, "_cloud_ws", None)
        if ws is None or ws.numel() != nbytes:  # cached by size
            ws = self._cloud_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out = {"points": torch.empty(B, K, 3, dtype=torch.float32, device=self.device),
               "colors": torch.empty(B, K, 3, dtype=torch.uint8, device=self.device),
               "source": torch.empty(B, K, dtype=torch.int32, device=self.device),
               "count": torch.empty(B, dtype=torch.int32, device=self.device)}
        vis = self._visual()
        targets = self._target_poses().contiguous()
        self._call("ps_point_cloud", self._ctx, _ptr(self.state), cv, len(views), int(width), int(height),
                   C.byref(vis), _ptr(targets), None if box is None else C.byref(box), K,
                   int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(out["points"]), _ptr(out["colors"]), _ptr(out["source"]),
                   _ptr(out["count"]), _ptr(ws), self._stream())
        return out

    def _cloud_view(self, width: int, height: int, view) -> L.CloudView:
        cv = L.CloudView()
        vm, pm, tran = self.get_cam2world_transforms(width, height, **dict(view))
        cv.view[:], cv.proj[:], cv.tran_pix_world[:] = vm, pm, tran.reshape(-1).tolist()
        return cv

    def keypoint_features(self, points, keypoints, view, colors=None, count=None, radius: int = 3,
                          threshold: float = 0.1, values=None, width: int = 480, height: int = 480,
                          return_targets: bool = False):
        """The keypoint conditioning of the reference's inp_dim = 7 policies
        (run_policy.py:202-285, take_rgbd) -- fused (ps_cloud_keypoint_features),
        for every env, without rendering the keypoint view: per keypoint the
        pixels within `radius` of it (pix2pix_neighborhood, clipped to the
        image), their world points (deproject), and a cloud point is marked
        when the nearest of them is closer than `threshold`
        (point2point_neighborhood).  The channel is values[k] of the last
        keypoint that marks the point, else 0: the reference's 1.0 for the
        start keypoint, then 2.0 for the end keypoint.

        points [B, K, 3] f32 and colors None or [B, K, 3] u8 (point_cloud()'s),
        keypoints [B, n_kp, 2] or [n_kp, 2] integers (column, row) in `view`
        (a dict of get_cam2world_transforms' keyword arguments), 1 <= n_kp <= 4;
        a keypoint whose disc lies outside the image marks nothing, and so does
        one with a negative coordinate (the way to say "absent").  count None or [B] i32 (point_cloud()'s): an env
        whose count is 0 gets zero rows.  values defaults to
        (1.0, 2.0, 3.0, 4.0)[:n_kp].  Returns feats [B, K, 4] f32 (the colours
        as floats 0..255, then the channel; [B, K, 1] without colours), what
        segment_cloud takes as `colors` of a seven-channel net; with
        return_targets also targets [B, n_kp, P, 3] f64, the patches' world
        points (NaN for a pixel outside the image)."""
        self._check_image_size(width, height)
        B, dev = self.num_envs, self.device
        points = torch.as_tensor(points, device=dev)
        keypoints = torch.as_tensor(np.asarray(keypoints) if not torch.is_tensor(keypoints) else keypoints, device=dev)
        if colors is not None:
            colors = torch.as_tensor(colors, device=dev)
        if count is not None:
            count = torch.as_tensor(count, device=dev)
        K, n_kp, radius, threshold, values = keypoint_features_args(B, points, keypoints, colors, count, radius,
                                                                    threshold, values)
        if keypoints.dim() == 2:
            keypoints = keypoints.unsqueeze(0).expand(B, -1, -1)
        keypoints = keypoints.to(torch.int32).contiguous()
        points = points.contiguous()
        colors = None if colors is None else colors.contiguous()
        count = None if count is None else count.contiguous()
        cv = self._cloud_view(width, height, view)
        ld = 1 if colors is None else 4
        feats = torch.empty(B, K, ld, dtype=torch.float32, device=dev)
        targets = (torch.empty(B, n_kp, patch_size(radius), 3, dtype=torch.float64, device=dev)
                   if return_targets else None)
        vis = self._visual()
        poses = self._target_poses().contiguous()
        self._call("ps_cloud_keypoint_features", self._ctx, _ptr(self.state), C.byref(cv), int(width), int(height),
                   C.byref(vis), _ptr(poses), _ptr(keypoints), n_kp, radius, threshold, (C.c_float * n_kp)(*values),
                   _ptr(points), _ptr(colors), _ptr(count), K, _ptr(feats), ld, 0, _ptr(targets), self._stream())
        return (feats, targets) if return_targets else feats

    def keypoint_cloud(self, keypoints, views=None, keypoint_view=None, n_points: int = 5000, width: int = 480,
                       height: int = 480, radius: int = 3, threshold: float = 0.1, values=None, seed: int = 0,
                       crop=None) -> Dict[str, torch.Tensor]:
        """take_rgbd's observation for every env: point_cloud(views, ...) and
        keypoint_features of that cloud with its count.  keypoint_view
        defaults to views[0], the view take_rgbd picks its keypoints in.
        Returns point_cloud's dict plus feats [B, K, 4] f32 and cond [B, K] f32
        (the channel alone, a view of feats): predict_waypoints(net, out["points"],
        out["feats"]) runs a seven-channel CloudSegNet on it."""
        views = GRASP_VIEWS if views is None else list(views)
        out = self.point_cloud(views, n_points, width, height, seed, crop)
        kv = views[0] if keypoint_view is None else keypoint_view
        out["feats"] = self.keypoint_features(out["points"], keypoints, kv, out["colors"], out["count"], radius,
                                              threshold, values, width, height)
        out["cond"] = out["feats"][..., 3]
        return out

    def project_to_pixels(self, points, width: int = 480, height: int = 480, **view) -> torch.Tensor:
        """render()'s waypoints_proj for every env, on the device: world points
        [B, n, 3] (or [n, 3], the same for every env) -> [B, n, 2] i32
        (column, row) in the view of get_cam2world_transforms(width, height,
        **view).  How a keypoint is got from an object's position."""
        vm, pm, _ = self.get_cam2world_transforms(width, height, **view)
        points = torch.as_tensor(points, device=self.device)
        if points.dim() == 2:
            points = points.unsqueeze(0).expand(self.num_envs, -1, -1)
        if points.dim() != 3 or points.shape[0] != self.num_envs or points.shape[2] != 3:
            raise ValueError(f"project_to_pixels: points must be [{self.num_envs}, n, 3], got {tuple(points.shape)}")
        return project_to_pixels(points, vm, pm, width, height)

    def deproject(self, depth, pixels, tran_pix_world, width: int = 480, height: int = 480) -> torch.Tensor:
        """PyBullet.deproject (pybullet.py:109-146) per env: depth [B, h, w]
        (or one [h, w] image for every env), pixels [n, 2] or [B, n, 2]
        (column, row) -> world points [B, n, 3] float64."""
        B = self.num_envs
        depth = torch.as_tensor(depth, device=self.device).to(torch.float32)
        if depth.dim() == 2:
            depth = depth.unsqueeze(0).expand(B, -1, -1)
        depth = depth.contiguous()
        pixels = torch.as_tensor(np.asarray(pixels) if not torch.is_tensor(pixels) else pixels,
                                 device=self.device).to(torch.int32)
        if pixels.dim() == 2:
            pixels = pixels.unsqueeze(0).expand(B, -1, -1)
        pixels = pixels.contiguous()
        if depth.shape != (B, height, width) or pixels.shape[0] != B or pixels.shape[2] != 2:
            raise ValueError(f"deproject: depth {tuple(depth.shape)} / pixels {tuple(pixels.shape)} do not match "
                             f"{B} envs of {height}x{width}")
        if pixels.numel() and (int(pixels[..., 0].min()) < 0 or int(pixels[..., 0].max()) >= width
                               or int(pixels[..., 1].min()) < 0 or int(pixels[..., 1].max()) >= height):
            raise IndexError("deproject: pixel outside the image")  # numpy's depth[rows, cols] raises too
        n = pixels.shape[1]
        points = torch.empty(B, n, 3, dtype=torch.float64, device=self.device)
        T = (C.c_double * 16)(*np.asarray(tran_pix_world, np.float64).reshape(-1).tolist())
        self._call("ps_deproject_pixels", self._ctx, _ptr(depth), _ptr(pixels), int(n), T, int(width), int(height),
                   _ptr(points), self._stream())
        return points

    # ------------------------------------------------------- per-env RNGs
    def seed(self, seeds, mask=None) -> None:
        """seeding.np_random(seed) per env (core.py:244): seeds [B] uint64 (int64 bits)."""
        seeds = torch.as_tensor(seeds, device=self.device).to(torch.int64).reshape(self.num_envs).contiguous()
        m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._call("ps_rng_seed", self._ctx, _ptr(self.state), _ptr(m), _ptr(seeds), self._stream())

    def random_rotation(self, mask=None) -> torch.Tensor:
        """Rotation.random().as_quat() of every env's Flip goal stream -> [B, 4] float64."""
        out = torch.empty(self.num_envs, 4, dtype=torch.float64, device=self.device)
        m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._call("ps_rng_rotation", self._ctx, _ptr(self.state), _ptr(m), _ptr(out), self._stream())
        return out

    def uniform(self, low, high, mask=None) -> torch.Tensor:
        """Generator.uniform(low, high) of every env's own PCG64 stream -> [B, n] float64."""
        lo = [float(x) for x in (low if hasattr(low, "__len__") else [low])]
        hi = [float(x) for x in (high if hasattr(high, "__len__") else [high])]
        n = len(lo)
        if n != len(hi) or not 1 <= n <= L.PS_MAX_UNIFORM:
            raise ValueError("uniform: low/high must have the same length, 1..8")
        out = torch.empty(self.num_envs, n, dtype=torch.float64, device=self.device)
        m = None if mask is None else torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._call("ps_rng_uniform", self._ctx, _ptr(self.state), _ptr(m), n, (C.c_double * n)(*lo),
                   (C.c_double * n)(*hi), _ptr(out), self._stream())
        return out

    # ------------------------------------------------------------ stepping
    def step(self) -> None:
        """pybullet.py:52-55: n_substeps stepSimulation() calls."""
        self._call("ps_sim_step", self._ctx, _ptr(self.state), self.n_substeps, self._stream())

    def save_state(self) -> int:
        """pybullet.py:61-68: in-memory snapshot; returns a state id."""
        sid = next(self._ids)
        self._saved[sid] = self.state.clone()
        return sid

    def restore_state(self, state_id: int) -> None:
        """pybullet.py:266-272.  Unknown/removed ids raise (pybullet.error in the reference)."""
        if state_id not in self._saved:
            raise L.PandasimError(f"restoreState: unknown state id {state_id}")
        self.state.copy_(self._saved[state_id])
        self._call("ps_mark_motor_rows_dirty", self._ctx)  # the snapshot's motor rows

    def remove_state(self, state_id: int) -> None:
        """pybullet.py:274-280."""
        if self._saved.pop(state_id, None) is None:
            raise L.PandasimError(f"removeState: unknown state id {state_id}")

    # -------------------------------------------------------------- getters
    def link_state(self, link: int):
        B = self.num_envs
        pos = torch.empty(B, 3, device=self.device)
        quat = torch.empty(B, 4, device=self.device)
        lv = torch.empty(B, 3, device=self.device)
        av = torch.empty(B, 3, device=self.device)
        self._call("ps_link_state", self._ctx, _ptr(self.state), int(link), _ptr(pos), _ptr(quat), _ptr(lv), _ptr(av),
                   self._stream())
        return pos, quat, lv, av

    def get_link_position(self, body: str, link: int) -> torch.Tensor:
        return self.link_state(link)[0]

    def get_link_orientation(self, body: str, link: int) -> torch.Tensor:
        return self.link_state(link)[1]

    def get_link_velocity(self, body: str, link: int) -> torch.Tensor:
        return self.link_state(link)[2]

    def get_link_angular_velocity(self, body: str, link: int) -> torch.Tensor:
        return self.link_state(link)[3]

    def get_joint_angle(self, body: str, joint: int) -> torch.Tensor:
        return self.f[L.F_Q + JOINT_TO_DOF[joint], :self.num_envs].clone()

    def get_joint_velocity(self, body: str, joint: int) -> torch.Tensor:
        return self.f[L.F_QD + JOINT_TO_DOF[joint], :self.num_envs].clone()

    def _object_rows(self, body: str) -> int:
        return L.OBJECT_ROWS[self._objects[body]]

    def _base_state(self, body: str):
        B = self.num_envs
        pos, euler, vel, avel = (torch.empty(B, 3, device=self.device) for _ in range(4))
        quat = torch.empty(B, 4, device=self.device)
        self._call("ps_base_state", self._ctx, _ptr(self.state), self._objects[body], _ptr(pos), _ptr(quat),
                   _ptr(euler), _ptr(vel), _ptr(avel), self._stream())
        return pos, quat, euler, vel, avel

    def get_base_position(self, body: str) -> torch.Tensor:
        """getBasePositionAndOrientation[0] (pybullet.py:284-294)."""
        kind = self._kind(body)
        if kind == "ghost":
            return self._ghost_pos[body].clone()
        if kind == "robot":
            return torch.tensor([float(x) for x in self.cfg.base], device=self.device).expand(self.num_envs, 3)
        return self.rows(self._object_rows(body), 3).clone()

    def get_base_orientation(self, body: str) -> torch.Tensor:
        """getBasePositionAndOrientation[1] (pybullet.py:296-306), (x, y, z, w)."""
        kind = self._kind(body)
        if kind == "ghost":
            return self._ghost_orn[body].clone()
        if kind == "robot":
            return torch.tensor([0.0, 0.0, 0.0, 1.0], device=self.device).expand(self.num_envs, 4)
        return self.rows(self._object_rows(body) + 3, 4).clone()

    def get_base_rotation(self, body: str, type: str = "euler") -> torch.Tensor:
        """pybullet.py:308-325: getEulerFromQuaternion of the base orientation."""
        if type == "quaternion":
            return self.get_base_orientation(body)
        if type != "euler":
            raise ValueError("""type must be "euler" or "quaternion".""")
        if self._kind(body) == "object":
            return self._base_state(body)[2]
        return euler_from_quaternion(self.get_base_orientation(body))

    def get_base_velocity(self, body: str) -> torch.Tensor:
        """getBaseVelocity[0] (pybullet.py:327-337)."""
        if self._kind(body) != "object":
            return torch.zeros(self.num_envs, 3, device=self.device)
        return self.rows(self._object_rows(body) + 7, 3).clone()

    def get_base_angular_velocity(self, body: str) -> torch.Tensor:
        """getBaseVelocity[1] (pybullet.py:339-349)."""
        if self._kind(body) != "object":
            return torch.zeros(self.num_envs, 3, device=self.device)
        return self.rows(self._object_rows(body) + 10, 3).clone()

    # -------------------------------------------------------------- setters
    def set_joint_angles(self, body: str, joints: Sequence[int], angles) -> None:
        """resetJointState (pybullet.py:441-460): position set, velocity zeroed;
        the robot's cached contacts break (the links are teleported)."""
        angles = torch.as_tensor(angles, dtype=torch.float32, device=self.device)
        for k, j in enumerate(joints):
            d = JOINT_TO_DOF[int(j)]
            self.f[L.F_Q + d, :self.num_envs] = angles[..., k]
            self.f[L.F_QD + d, :self.num_envs] = 0.0
        self.f[L.F_WR:L.F_WRID + 1, :self.num_envs] = 0.0

    def set_joint_angle(self, body: str, joint: int, angle) -> None:
        self.set_joint_angles(body, [joint], torch.as_tensor(angle, dtype=torch.float32).reshape(-1, 1)
                              if torch.as_tensor(angle).dim() else [angle])

    def set_base_pose(self, body: str, position, orientation) -> None:
        """resetBasePositionAndOrientation (pybullet.py:427-439).  PyBullet's
        init-pose command zeroes the base linear and angular velocity with the
        pose; the object's cached contacts break (it is teleported).  A 3-vector
        orientation is Euler angles (getQuaternionFromEuler)."""
        orientation = torch.as_tensor(orientation, dtype=torch.float64, device=self.device)
        if orientation.shape[-1] == 3:
            orientation = quaternion_from_euler(orientation)
        kind = self._kind(body)
        if kind == "robot":
            raise NotImplementedError("the Panda base is fixed (loadURDF useFixedBase=True)")
        if kind == "ghost":
            pos = torch.as_tensor(position, dtype=torch.float64, device=self.device)
            self._ghost_pos[body][:] = pos.expand(self.num_envs, 3)
            self._ghost_orn[body][:] = orientation.expand(self.num_envs, 4)
            return
        row = self._object_rows(body)
        self.set_rows(row, torch.as_tensor(position, device=self.device).to(torch.float32))
        self.set_rows(row + 3, orientation.to(torch.float32))
        self.f[row + 7:row + 13, :self.num_envs] = 0.0
        g = L.F_WG0 if self._objects[body] == 0 else L.F_WG1
        self.f[g:g + 5, :self.num_envs] = 0.0
        self.f[L.F_WR:L.NUM_FLOAT_ROWS, :self.num_envs] = 0.0  # gripper and object-object contacts

    def control_joints(self, body: str, joints: Sequence[int], target_angles, forces) -> None:
        """setJointMotorControlArray(POSITION_CONTROL) (pybullet.py:462-477)."""
        t = torch.as_tensor(target_angles, dtype=torch.float32, device=self.device)
        for k, j in enumerate(joints):
            d = JOINT_TO_DOF[int(j)]
            self.f[L.F_MTARGET + d, :self.num_envs] = t[..., k]
            self.f[L.F_MKP + d, :self.num_envs] = 0.1
            self.f[L.F_MKD + d, :self.num_envs] = 1.0
            self.f[L.F_MVEL + d, :self.num_envs] = 0.0
            self.f[L.F_MIMP + d, :self.num_envs] = float(forces[k]) * DT_SUBSTEP
        self._call("ps_mark_motor_rows_dirty", self._ctx)  # a fused step rewrites the gains

    def inverse_kinematics(self, body: str, link: int, position, orientation) -> torch.Tensor:
        """calculateInverseKinematics from the current joints (pybullet.py:479-497) -> [B, 9]."""
        B = self.num_envs
        pos = torch.as_tensor(position, dtype=torch.float32, device=self.device).expand(B, 3).contiguous()
        orn = torch.as_tensor(orientation, dtype=torch.float32, device=self.device).expand(B, 4).contiguous()
        out = torch.empty(B, 9, device=self.device)
        self._call("ps_inverse_kinematics", self._ctx, _ptr(self.state), int(link), _ptr(pos), _ptr(orn), _ptr(out),
                   self._stream())
        return out

    def euler_xyz_to_quat(self, euler_xyz) -> torch.Tensor:
        """scipy's R.from_euler('xyz', e, degrees=True).as_quat() (panda_ori.py:91)
        for (..., 3) degrees -> (..., 4) float32 (x, y, z, w), on the GPU."""
        e = torch.as_tensor(euler_xyz, dtype=torch.float32, device=self.device)
        if e.dim() == 0 or e.shape[-1] != 3:
            raise ValueError(f"euler_xyz_to_quat: expected (..., 3) angles, got {tuple(e.shape)}")
        flat = e.reshape(-1, 3).contiguous()
        out = torch.empty(flat.shape[0], 4, device=self.device)
        self._call("ps_euler_xyz_to_quat", self._ctx, _ptr(flat), _ptr(out), flat.shape[0], self._stream())
        return out.reshape(*e.shape[:-1], 4)

    def quat_to_euler_xyz(self, quat) -> torch.Tensor:
        """R.from_quat(q).as_euler('xyz', degrees=True) (panda_cartesian.py:222-225)
        for (..., 4) quaternions (x, y, z, w) -> (..., 3) float32 degrees, on
        the GPU; unspecified within 1e-3 degrees of pitch +-90."""
        q = torch.as_tensor(quat, dtype=torch.float32, device=self.device)
        if q.dim() == 0 or q.shape[-1] != 4:
            raise ValueError(f"quat_to_euler_xyz: expected (..., 4) quaternions, got {tuple(q.shape)}")
        flat = q.reshape(-1, 4).contiguous()
        out = torch.empty(flat.shape[0], 3, device=self.device)
        self._call("ps_quat_to_euler_xyz", self._ctx, _ptr(flat), _ptr(out), flat.shape[0], self._stream())
        return out.reshape(*q.shape[:-1], 3)

    # ---------------------------------------------------- motion primitives
    # panda_cartesian.py:74-145 (move / grasp / release), fused: a plan call
    # fills a MotionPlan from the state, motion_run executes its control steps
    def motion_plan(self) -> "MotionPlan":
        """A zeroed plan buffer of this batch (nothing to do, gripper free)."""
        return MotionPlan(self)

    def _mask(self, mask) -> Optional[torch.Tensor]:
        if mask is None:
            return None
        m = torch.as_tensor(mask, device=self.device)
        if m.shape != (self.num_envs,):
            raise ValueError(f"mask: expected ({self.num_envs},), got {tuple(m.shape)}")
        return (m != 0).to(torch.uint8).contiguous()

    def plan_move(self, plan: "MotionPlan", goal_pos, goal_quat, mask=None) -> None:
        """ps_plan_move: goal_pos [B, 3] or [3] world, goal_quat [B, 4] or [4] (x, y, z, w)."""
        B = self.num_envs
        pos = torch.as_tensor(goal_pos, dtype=torch.float32, device=self.device)
        orn = torch.as_tensor(goal_quat, dtype=torch.float32, device=self.device)
        if pos.shape not in ((3,), (B, 3)):
            raise ValueError(f"goal_pos: expected (3,) or ({B}, 3), got {tuple(pos.shape)}")
        if orn.shape not in ((4,), (B, 4)):
            raise ValueError(f"goal_quat: expected (4,) or ({B}, 4), got {tuple(orn.shape)}")
        pos, orn, m = pos.expand(B, 3).contiguous(), orn.expand(B, 4).contiguous(), self._mask(mask)
        self._call("ps_plan_move", self._ctx, _ptr(self.state), _ptr(plan.buf), _ptr(pos), _ptr(orn), _ptr(m),
                   self._stream())

    def plan_grasp(self, plan: "MotionPlan", mask=None) -> None:
        m = self._mask(mask)
        self._call("ps_plan_grasp", self._ctx, _ptr(self.state), _ptr(plan.buf), _ptr(m), self._stream())

    def plan_release(self, plan: "MotionPlan", width=None, mask=None) -> None:
        """ps_plan_release: width a number or [B] (None = 1)."""
        w = None
        if width is not None:
            w = torch.as_tensor(width, dtype=torch.float32, device=self.device).expand(self.num_envs).contiguous()
        m = self._mask(mask)
        self._call("ps_plan_release", self._ctx, _ptr(self.state), _ptr(plan.buf), _ptr(w), _ptr(m), self._stream())

    def motion_run(self, plan: "MotionPlan", max_steps: int) -> None:
        """ps_motion_run: every env runs min(max_steps, num_steps - done) control steps."""
        self._call("ps_motion_run", self._ctx, _ptr(self.state), _ptr(plan.buf), int(max_steps), self._stream())

    def motion_program(self, plan: "MotionPlan", program, blocked: bool):
        """ps_motion_program: the segments of `program` (a
        panda_cartesian.MotionProgram of this batch) in one launch, each env
        planning its next segment from the state it has reached; `blocked` is
        the gripper's flag before the first segment.  The goals' Euler angles
        become quaternions in one euler_xyz_to_quat call.  Returns (completed
        [B] i32, steps [B] i32, the flag after the last segment); no tensor is
        read on the host."""
        if program.num_envs != self.num_envs or program.device != self.device:
            raise ValueError(f"program: built for {program.num_envs} envs on {program.device}, the sim has "
                             f"{self.num_envs} on {self.device}")
        low = program.lower(blocked)
        S, B = len(low.kinds), self.num_envs
        quat = None if low.goal_euler is None else self.euler_xyz_to_quat(low.goal_euler)
        completed = torch.empty(B, dtype=torch.int32, device=self.device)
        steps = torch.empty(B, dtype=torch.int32, device=self.device)
        self._call("ps_motion_program", self._ctx, _ptr(self.state), _ptr(plan.buf), S, (C.c_int32 * S)(*low.kinds),
                   (C.c_int32 * S)(*low.wait_steps), int(bool(blocked)), _ptr(low.goal_pos), _ptr(quat), _ptr(low.width),
                   _ptr(low.mask), _ptr(completed), _ptr(steps), self._stream())
        return completed, steps, low.blocked_after


class MotionPlan:
    """The plan buffer of the motion primitives (include/pandasim.h PS_PLAN_*):
    ``d`` [PLAN_NUM_F64_ROWS, stride] float64 and ``n`` [PLAN_NUM_I32_ROWS,
    stride] int32 are views of ``buf``; num_steps / done / blocked are the
    [B] views of their rows."""

    def __init__(self, sim: PandaSim):
        nbytes = sim._lib.ps_motion_plan_bytes(sim.num_envs)
        if nbytes <= 0:
            raise L.PandasimError("ps_motion_plan_bytes failed")
        stride, B = sim.layout.stride, sim.num_envs
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=sim.device)
        split = L.PLAN_NUM_F64_ROWS * stride * 8
        self.d = self.buf[:split].view(torch.float64).view(L.PLAN_NUM_F64_ROWS, stride)
        self.n = self.buf[split:].view(torch.int32).view(L.PLAN_NUM_I32_ROWS, stride)
        self.num_steps = self.n[L.PLAN_NUM_STEPS, :B]
        self.done = self.n[L.PLAN_DONE, :B]
        self.blocked = self.n[L.PLAN_BLOCKED, :B]


# ---------------------------------------------------------------- helpers
PLANE_Z = -0.4                      # tasks/*.py: create_plane(z_offset=-0.4)


def euler_from_quaternion(q: torch.Tensor) -> torch.Tensor:
    """getEulerFromQuaternion (Bullet btQuaternion::getEulerZYX convention, as
    ps_task_rng.h::euler_from_quat) for (..., 4) (x, y, z, w) tensors."""
    x, y, z, w = q.unbind(-1)
    sarg = -2.0 * (x * z - w * y)
    roll = torch.atan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z)
    pitch = torch.asin(sarg.clamp(-1.0, 1.0))
    yaw = torch.atan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
    lo, hi = sarg <= -0.99999, sarg >= 0.99999
    roll = torch.where(lo | hi, torch.zeros_like(roll), roll)
    pitch = torch.where(lo, torch.full_like(pitch, -0.5 * math.pi), torch.where(hi, torch.full_like(pitch, 0.5 * math.pi),
                                                                              pitch))
    yaw = torch.where(lo, 2.0 * torch.atan2(x, -y), torch.where(hi, 2.0 * torch.atan2(-x, y), yaw))
    return torch.stack([roll, pitch, yaw], -1)


def quaternion_from_euler(e: torch.Tensor) -> torch.Tensor:
    """getQuaternionFromEuler (roll about x, pitch about y, yaw about z) -> (x, y, z, w)."""
    r, p, y = (e * 0.5).unbind(-1)
    cr, sr, cp, sp, cy, sy = torch.cos(r), torch.sin(r), torch.cos(p), torch.sin(p), torch.cos(y), torch.sin(y)
    return torch.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                        cr * cp * cy + sr * sp * sy], -1)


# ---------------------------------------------- keypoint conditioning (host)
def patch_size(radius: int) -> int:
    """P of keypoint_features: the integer offsets within `radius` of a pixel
    (1, 29 and 197 for radius 0, 3 and 8)."""
    r = int(radius)
    return sum(2 * math.isqrt(r * r - dx * dx) + 1 for dx in range(-r, r + 1))


def keypoint_features_args(num_envs: int, points, keypoints, colors, count, radius, threshold, values):
    """keypoint_features' argument checks (ValueError), on tensors of any
    device: -> K, n_kp, radius, threshold and the values as floats."""
    from .cloudnet import _want

    B, fn = int(num_envs), "keypoint_features"
    _want(fn, "points", points, (B, "K", 3))
    K = int(points.shape[1])
    if not 1 <= K <= L.CLOUD_MAX_DENSE_POINTS:
        raise ValueError(f"{fn}: points holds K = {K} points (1 to {L.CLOUD_MAX_DENSE_POINTS})")
    whole = torch.is_tensor(keypoints) and not keypoints.is_floating_point() and not keypoints.is_complex() \
        and keypoints.dtype != torch.bool
    if not whole or keypoints.dim() not in (2, 3) or keypoints.shape[-1] != 2 or \
            (keypoints.dim() == 3 and keypoints.shape[0] != B):
        raise ValueError(f"{fn}: keypoints must be [{B}, n_kp, 2] or [n_kp, 2] integers (column, row), got "
                         f"{tuple(keypoints.shape) if torch.is_tensor(keypoints) else type(keypoints).__name__} "
                         f"{getattr(keypoints, 'dtype', '')}")
    n_kp = int(keypoints.shape[-2])
    if not 1 <= n_kp <= L.CLOUD_KEYPOINT_MAX:
        raise ValueError(f"{fn}: keypoints holds n_kp = {n_kp} keypoints (1 to {L.CLOUD_KEYPOINT_MAX})")
    if colors is not None:
        _want(fn, "colors", colors, (B, K, 3), torch.uint8)
    if count is not None:
        _want(fn, "count", count, (B,), torch.int32)
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or \
            not 0 <= radius <= L.CLOUD_KEYPOINT_MAX_RADIUS:
        raise ValueError(f"{fn}: radius = {radius!r} (a whole number of pixels from 0 to {L.CLOUD_KEYPOINT_MAX_RADIUS})")
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        thr = math.nan
    if not 0.0 < thr < math.inf:
        raise ValueError(f"{fn}: threshold = {threshold!r} must be positive and finite")
    if values is None:
        values = (1.0, 2.0, 3.0, 4.0)[:n_kp]
    try:
        values = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: values must be {n_kp} numbers") from None
    if len(values) != n_kp:
        raise ValueError(f"{fn}: values holds {len(values)} numbers for n_kp = {n_kp} keypoints")
    return K, n_kp, int(radius), thr, values


def project_to_pixels(points, view_matrix, proj_matrix, width: int, height: int) -> torch.Tensor:
    """render()'s waypoints_proj arithmetic (pybullet.py:251-258) for a tensor
    of world points [..., 3] on any device -> [..., 2] i32 (column, row):
    (x, y, z, w) = P V (p, 1) in f64, x = (x / w + 1) / 2 * width, the same for
    y with height, and [int(x), int(height - y)], int() truncating towards 0.
    P V is numpy's product of the order='F' matrices, as there; its product
    with the point is written out term by term (k ascending)."""
    PV = np.matmul(np.asarray(proj_matrix).reshape([4, 4], order="F"), np.asarray(view_matrix).reshape([4, 4], order="F"))
    p = torch.as_tensor(points).to(torch.float64)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    x, y, _, w = (px * float(PV[r, 0]) + py * float(PV[r, 1]) + pz * float(PV[r, 2]) + float(PV[r, 3]) for r in range(4))
    x, y = (x / w + 1) / 2 * width, (y / w + 1) / 2 * height
    out = torch.stack([x, height - y], -1).trunc()
    # a point on the camera plane has no pixel: as far off the image as i32 goes
    return torch.nan_to_num(out, nan=-2.0 ** 31, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31).clamp(
        -2.0 ** 31, 2.0 ** 31 - 1).to(torch.int32)
