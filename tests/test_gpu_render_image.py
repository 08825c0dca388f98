"""GPU tests of the camera image itself (ps_render: k_render_prep + k_render,
csrc/ps_render.h) against the oracle's fp64 image after DESIGN.md §11
(render_oracle.raycast_image): role, depth and colour on every stable pixel,
the ghost targets, the arm culling's independence of the tiling, the output
plumbing and the degenerate rays.

Scenes (helpers.render_scene) are written straight into the state rows and
ps_render is called through the C ABI with an explicit ps_visual and targets
tensor.  A pixel is compared where the oracle marks it stable (role,
primitive, face and ghost flags equal on all its neighbours); the coverage
conditions asserted before each comparison (tests/test_render_cpu.py checks
the same ones without a GPU) keep those sets from being empty.

Bounds.  Depth: relative error of the linear depth < 1e-4 on every stable
pixel (the bound test_gpu_render.py applies to 99 % of pixels).  Colour: the
unquantised fp32 colour is a product and sum of a handful of terms of size
<= 1, its error is some 1e-6, far below half a level (2e-3), so floor(255 c +
0.5) can differ from the oracle's by at most one level.  Hit or miss: exact.
Every test prints its figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import render_oracle as RO
from helpers import (GHOST_ALPHAS, GHOST_CAMERAS, GHOST_CASES, GHOST_VARIANTS, MIN_CASE_PIXELS, MIN_TILING_ROBOT_PIXELS,
                     RENDER_B, RENDER_H, RENDER_TASKS, RENDER_W, TILING_CAMERAS, TILING_SHAPES, RenderVisual,
                     check_render_coverage, oracle_config_for, render_camera, render_scene, snapshot)
from pandasim import _lib as L

pytestmark = pytest.mark.gpu

DEPTH_REL = 1e-4
PS_ERR_ARG = -1


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib_visual(v):
    out = L.Visual()
    for r in range(8):
        for k in range(4):
            out.rgba[r][k] = float(v.rgba[r][k])
    for g in range(2):
        out.target_shape[g] = int(v.target_shape[g])
        for k in range(3):
            out.target_half[g][k] = float(v.target_half[g][k])
    return out


def _targets(t):
    return None if t is None else torch.from_numpy(np.asarray(t, np.float32)).cuda().contiguous()


def ps_render_rc(sim, view, proj, w, h, vis, targets, depth, rgb):
    """The C ABI's return code (outputs are torch tensors or None)."""
    fv, fp = (C.c_float * 16)(*view), (C.c_float * 16)(*proj)
    with torch.cuda.device(sim.device):
        return sim._lib.ps_render(sim._ctx, _ptr(sim.state), fv, fp, int(w), int(h),
                                  None if vis is None else C.byref(vis), _ptr(targets), _ptr(depth), _ptr(rgb),
                                  sim._stream())


def render(sim, view, proj, w, h, visual, targets, want_depth=True, want_rgb=True):
    """ps_render -> (depth [B, h, w] f32, rgb [B, h, w, 3] u8) as numpy; a buffer not wanted is passed as NULL."""
    B = sim.num_envs
    depth = torch.full((B, h, w), float("nan"), dtype=torch.float32, device=sim.device) if want_depth else None
    rgb = torch.full((B, h, w, 3), 77, dtype=torch.uint8, device=sim.device) if want_rgb else None
    vis = _lib_visual(visual)
    tg = _targets(targets)
    fv, fp = (C.c_float * 16)(*view), (C.c_float * 16)(*proj)
    sim._call("ps_render", sim._ctx, _ptr(sim.state), fv, fp, int(w), int(h), C.byref(vis), _ptr(tg), _ptr(depth),
              _ptr(rgb), sim._stream())
    torch.cuda.synchronize()
    return (None if depth is None else depth.cpu().numpy()), (None if rgb is None else rgb.cpu().numpy())


def scene_sim(scene, envs=None):
    """A PandaSim of the scene's task whose state rows hold the scene (all envs, or the listed ones)."""
    from pandasim.sim import PandaSim

    envs = list(range(RENDER_B)) if envs is None else envs
    sim = PandaSim(scene.task, num_envs=len(envs))
    sim.set_rows(L.F_Q, torch.from_numpy(scene.q[envs].astype(np.float32)))
    for ob, (rp, rq) in enumerate(((L.F_CPOS, L.F_CQUAT), (L.F_C2POS, L.F_C2QUAT))[:scene.n_objects]):
        sim.set_rows(rp, torch.from_numpy(scene.obj_pos[envs, ob].astype(np.float32)))
        sim.set_rows(rq, torch.from_numpy(scene.obj_quat[envs, ob].astype(np.float32)))
    torch.cuda.synchronize()
    # the state the kernel reads is the state the oracle is given
    f = snapshot(sim)["f"]
    assert np.array_equal(f[L.F_Q:L.F_Q + 9].T, scene.q[envs])
    for ob, rp in enumerate((L.F_CPOS, L.F_C2POS)[:scene.n_objects]):
        assert np.array_equal(f[rp:rp + 3].T, scene.obj_pos[envs, ob])
        assert np.array_equal(f[rp + 3:rp + 7].T, scene.obj_quat[envs, ob])
    want, have = scene.oracle_cfg(), oracle_config_for(sim.cfg)
    assert scene.n_objects == sim.cfg.n_objects
    for name in ("has_table", "has_plane", "n_objects", "object_shape", "table_cx", "table_hx", "table_hy"):
        assert getattr(want, name) == getattr(have, name), name
    assert list(want.base) == list(have.base) and list(want.object_half) == list(have.object_half)
    return sim


_sims = {}


def sim_of(task):
    if task not in _sims:
        _sims[task] = scene_sim(render_scene(task))
    return _sims[task]


def _linear(depth, proj):
    P = np.asarray(proj, np.float64).reshape(4, 4, order="F")
    with np.errstate(divide="ignore"):
        return P[2, 3] / (2.0 * depth.astype(np.float64) - 1.0 + P[2, 2])


class Tally:
    """Figures of a comparison, gathered over images and printed before the assertions."""

    def __init__(self):
        self.pixels = self.stable = self.channels = self.equal = 0
        self.depth_rel, self.level, self.bad = 0.0, 0, []

    def add(self, tag, depth, rgb, im, proj, colour=True):
        st = im["stable"]
        self.pixels += st.size
        self.stable += int(st.sum())
        if depth is not None:
            hit_g, hit_r = depth < 1.0, im["depth"] < 1.0
            n = int((hit_g != hit_r)[st].sum())
            if n:
                self.bad.append((tag, "hit or miss differs on stable pixels", n))
            both = st & hit_g & hit_r
            if both.any():
                rel = np.abs(_linear(depth[both], proj) - im["t"][both]) / im["t"][both]
                self.depth_rel = max(self.depth_rel, float(rel.max()))
                if rel.max() >= DEPTH_REL:
                    self.bad.append((tag, "depth", float(rel.max()), int((rel >= DEPTH_REL).sum())))
        if rgb is not None and colour:
            diff = np.abs(rgb.astype(np.int64) - im["rgb"].astype(np.int64))[st]
            self.channels += diff.size
            self.equal += int((diff == 0).sum())
            if diff.size:
                self.level = max(self.level, int(diff.max()))
                if diff.max() > 1:
                    where = np.argwhere(st & (np.abs(rgb.astype(np.int64) - im["rgb"].astype(np.int64)).max(-1) > 1))[0]
                    r, c = int(where[0]), int(where[1])
                    self.bad.append((tag, "colour", int(diff.max()), int((diff.max(-1) > 1).sum()), (r, c),
                                     rgb[r, c].tolist(), im["rgb"][r, c].tolist(), int(im["role"][r, c]),
                                     int(im["face"][r, c]), im["ghost"][r, c].tolist()))

    def report(self, what):
        share = self.equal / max(self.channels, 1)
        print(f"{what}: stable {self.stable}/{self.pixels} pixels, max relative depth error {self.depth_rel:.3e}, "
              f"max colour difference {self.level} level(s), exactly equal channels {self.equal}/{self.channels} "
              f"= {share:.5f}")
        assert not self.bad, self.bad[:6]
        assert self.stable > 0


# ------------------------------------------------ a. colour and depth
@pytest.mark.parametrize("task", RENDER_TASKS)
def test_image_matches_oracle_on_stable_pixels(task):
    sc, sim = render_scene(task), sim_of(task)
    oracle = {cam["name"]: sc.oracle_images(cam) for cam in sc.cameras}
    shares, counts = check_render_coverage(sc, oracle)
    assert len(sc.cameras) >= 4 and sorted(c["roll"] for c in sc.cameras)[-2:] == [30, 90]
    assert any(c["pitch"] == -90 for c in sc.cameras)
    assert max(sc.straddles_near(sc.cameras[sc.closeup], i) for i in range(RENDER_B)) >= 1
    tally = Tally()
    for cam in sc.cameras:
        view, proj = render_camera(cam)
        depth, rgb = render(sim, view, proj, RENDER_W, RENDER_H, sc.visual, sc.targets)
        assert np.isfinite(depth).all() and depth.min() >= 0.0 and depth.max() <= 1.0
        for i in range(RENDER_B):
            tally.add((task, cam["name"], i), depth[i], rgb[i], oracle[cam["name"]][i], proj)
    print(task, "min stable share %.3f" % min(shares.values()), "case pixels", counts)
    tally.report(f"image {task}")


def test_ps_camera_matrices_render_the_same_stable_pixels():
    """The comparisons above use the oracle's own camera matrices; the same
    image through ps_camera's (which agree to fp32 rounding) holds too."""
    sc, sim = render_scene("push"), sim_of("push")
    tally = Tally()
    for cam in sc.cameras[:3]:
        view, proj, _ = sim.get_cam2world_transforms(RENDER_W, RENDER_H, np.array(cam["target"]), cam["distance"],
                                                     cam["yaw"], cam["pitch"], cam["roll"])
        cfg = sc.oracle_cfg()
        depth, rgb = render(sim, view, proj, RENDER_W, RENDER_H, sc.visual, sc.targets)
        for i in range(RENDER_B):
            im = RO.raycast_image(cfg, sc.oracle_env(cfg, i), view, proj, RENDER_W, RENDER_H, sc.visual, sc.targets[i])
            tally.add((cam["name"], i), depth[i], rgb[i], im, proj)
    tally.report("ps_camera matrices")


# ------------------------------------------------ b. ghost targets
@pytest.mark.parametrize("variant", list(GHOST_VARIANTS))
def test_ghost_targets(variant):
    sc, sim = render_scene("push"), sim_of("push")
    shapes, halves = GHOST_VARIANTS[variant]
    cams = [c for c in sc.cameras if c["name"] in GHOST_CAMERAS]
    assert len(cams) == len(GHOST_CAMERAS)
    none = RenderVisual((-1, -1), halves)
    tally = Tally()
    covered = dict.fromkeys(GHOST_CASES, 0)
    pure = [0, 0]
    for cam in cams:
        view, proj = render_camera(cam)
        d_none, c_none = render(sim, view, proj, RENDER_W, RENDER_H, none, sc.targets)
        # targets == NULL: the ghosts are nowhere, whatever their shapes
        d_null, c_null = render(sim, view, proj, RENDER_W, RENDER_H, RenderVisual(shapes, halves), None)
        assert np.array_equal(d_null.view(np.int32), d_none.view(np.int32)) and np.array_equal(c_null, c_none), cam
        for alphas in GHOST_ALPHAS:
            vis = RenderVisual(shapes, halves, alphas=alphas)
            depth, rgb = render(sim, view, proj, RENDER_W, RENDER_H, vis, sc.targets)
            # ghosts write no depth
            assert np.array_equal(depth.view(np.int32), d_none.view(np.int32)), (cam["name"], alphas)
            if alphas == (0.0, 0.0):
                assert np.array_equal(rgb, c_none), (cam["name"], "alpha 0 is not the image without ghosts")
            ims = sc.oracle_images(cam, visual=vis)
            for i, im in enumerate(ims):
                tally.add((variant, cam["name"], alphas, i), depth[i], rgb[i], im, proj)
                st, gh = im["stable"], im["ghost"]
                if alphas == GHOST_ALPHAS[0]:
                    for case in GHOST_CASES:
                        covered[case] += int((sc.cases[case](im) & st).sum())
                    # the background stays at depth 1 under a ghost
                    assert np.all(depth[i][st & gh[..., 0] & (im["role"] == RO.ROLE_BACKGROUND)] == 1.0)
                # the ghost blended last with alpha 1 shows its pure colour
                for g in range(2):
                    if alphas[g] == 1.0:
                        on = st & gh[..., g] & (~gh[..., 1] if g == 0 else True)
                        pure[g] += int(on.sum())
                        assert np.all(rgb[i][on] == RO.quantise(vis.rgba[RO.ROLE_TARGET1 + g, :3])), (cam["name"], g)
                if alphas == (1.0, 1.0):
                    # no stable pixel shows a ghost that the oracle has behind an opaque body
                    behind = st & ~gh.any(-1)
                    assert np.abs(rgb[i][behind].astype(int) - c_none[i][behind].astype(int)).max(initial=0) <= 0
    print(variant, "stable pixels per case", covered, "pure-colour pixels", pure)
    tally.report(f"ghosts {variant}")
    assert min(covered.values()) >= MIN_CASE_PIXELS, covered
    assert min(pure) >= MIN_CASE_PIXELS, pure


# ------------------------------------------------ c. tiling independence of the arm culling
@pytest.mark.parametrize("shape", TILING_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_arm_culling_does_not_depend_on_the_tiling(shape):
    sc, sim = render_scene("push"), sim_of("push")
    w, h = shape
    cams = [c if isinstance(c, dict) else next(k for k in sc.cameras if k["name"] == c) for c in TILING_CAMERAS]
    assert any(c["roll"] == 90 for c in cams)
    tally = Tally()
    robot = prims = 0
    for cam in cams:
        view, proj = render_camera(cam, w, h)
        depth, rgb = render(sim, view, proj, w, h, sc.visual, sc.targets)
        for i, im in enumerate(sc.oracle_images(cam, w, h)):
            tally.add((shape, cam["name"], i), depth[i], rgb[i], im, proj)
            on = im["stable"] & (im["role"] == RO.ROLE_ROBOT)
            robot += int(on.sum())
            prims = max(prims, len(np.unique(im["prim"][im["role"] == RO.ROLE_ROBOT])))
    print(shape, "stable robot pixels", robot, "most arm primitives in one image", prims)
    tally.report(f"tiling {w}x{h}")
    assert robot >= MIN_TILING_ROBOT_PIXELS.get(shape, MIN_CASE_PIXELS)


# ------------------------------------------------ d. output plumbing
def test_null_outputs_and_single_env():
    sc, sim = render_scene("stack"), sim_of("stack")
    cam = sc.cameras[0]
    view, proj = render_camera(cam, 50, 37)
    depth, rgb = render(sim, view, proj, 50, 37, sc.visual, sc.targets)
    d_only, none = render(sim, view, proj, 50, 37, sc.visual, sc.targets, want_rgb=False)
    none2, c_only = render(sim, view, proj, 50, 37, sc.visual, sc.targets, want_depth=False)
    assert none is None and none2 is None
    assert np.array_equal(d_only.view(np.int32), depth.view(np.int32)) and np.array_equal(c_only, rgb)
    assert (depth < 1.0).any() and len(np.unique(rgb.reshape(-1, 3), axis=0)) > 10
    for i in range(RENDER_B):
        one = scene_sim(sc, [i])
        d1, c1 = render(one, view, proj, 50, 37, sc.visual, sc.targets[i:i + 1])
        assert np.array_equal(d1[0].view(np.int32), depth[i].view(np.int32)), i
        assert np.array_equal(c1[0], rgb[i]), i
    assert not np.array_equal(rgb[0], rgb[1])


def test_argument_errors():
    sc, sim = render_scene("reach"), sim_of("reach")
    view, proj = render_camera(sc.cameras[0])
    vis = _lib_visual(sc.visual)
    depth = torch.zeros(RENDER_B, RENDER_H, RENDER_W, dtype=torch.float32, device=sim.device)
    assert ps_render_rc(sim, view, proj, RENDER_W, RENDER_H, vis, None, depth, None) == 0
    for w, h in ((0, RENDER_H), (RENDER_W, 0), (-1, RENDER_H), (RENDER_W, -5)):
        assert ps_render_rc(sim, view, proj, w, h, vis, None, depth, None) == PS_ERR_ARG, (w, h)
    assert ps_render_rc(sim, view, proj, RENDER_W, RENDER_H, None, None, depth, None) == PS_ERR_ARG
    # 4096 x 4097 pixels = 65 552 tiles of 256; with NULL outputs nothing is allocated or written
    assert ps_render_rc(sim, view, proj, 4096, 4097, vis, None, None, None) == PS_ERR_ARG
    torch.cuda.synchronize()
    assert ps_render_rc(sim, view, proj, RENDER_W, RENDER_H, vis, None, depth, None) == 0
    torch.cuda.synchronize()


def test_render_rgb_is_the_camera_image_with_channels_swapped():
    """render()'s docstring: rgb has the channels swapped (the reference's
    cv2.cvtColor(BGR2RGB) of pybullet's pixels); colors keeps the camera's order."""
    sim = sim_of("stack")
    cam = dict(target_position=np.array([0.0, 0.1, 0.1]), distance=0.8, yaw=30, pitch=-35, roll=20)
    out = sim.render(RENDER_W, RENDER_H, **cam)
    view, proj, _ = sim.get_cam2world_transforms(RENDER_W, RENDER_H, cam["target_position"], cam["distance"],
                                                 cam["yaw"], cam["pitch"], cam["roll"])
    depth, img = sim.get_camera_image(RENDER_W, RENDER_H, view, proj)
    assert torch.equal(out["rgb"], img[..., [2, 1, 0]]) and torch.equal(out["depth"], depth)
    assert torch.equal(out["colors"], img.reshape(RENDER_B, -1, 3))
    assert not torch.equal(img[..., 0], img[..., 2])  # or the order would not show


# ------------------------------------------------ e. degenerate rays
def _snapped(view):
    """The view matrix with its cos(90 degrees) entries (6e-17) at exactly 0: exactly axis-parallel camera axes."""
    return tuple(0.0 if abs(v) < 1e-9 else v for v in view)


AXIS_CAMERAS = [dict(name="along +y over the table", target=(0.0, 0.0, 0.1), distance=0.5, yaw=0, pitch=0, roll=0),
                dict(name="along +y at the arm", target=(-0.6, 0.0, 0.2), distance=0.6, yaw=0, pitch=0, roll=0),
                dict(name="down on the table", target=(0.2, -0.2, 0.0), distance=0.5, yaw=0, pitch=-90, roll=0),
                dict(name="down on the base column", target=(-0.6, 0.0, 0.3), distance=0.6, yaw=0, pitch=-90, roll=0)]


@pytest.mark.parametrize("snap", [False, True], ids=["as computed", "exact zeros"])
def test_axis_parallel_centre_rays(snap):
    """Odd image sizes: the centre pixel's ray is the camera's forward axis, so
    ray_box divides by zero on two axes and the capsule test may see a == 0."""
    sc, sim = render_scene("push"), sim_of("push")
    w, h = 33, 25
    cfg = sc.oracle_cfg()
    tally = Tally()
    centre = 0
    for cam in AXIS_CAMERAS:
        view, proj = render_camera(cam, w, h)
        if snap:
            view = _snapped(view)
            assert sorted(abs(v) for v in view[:11] if v != 0.0) == [1.0, 1.0, 1.0]
        depth, rgb = render(sim, view, proj, w, h, sc.visual, sc.targets)
        assert np.isfinite(depth).all() and depth.min() >= 0.0 and depth.max() <= 1.0, cam["name"]
        for i in range(RENDER_B):
            im = RO.raycast_image(cfg, sc.oracle_env(cfg, i), view, proj, w, h, sc.visual, sc.targets[i])
            tally.add((cam["name"], i), depth[i], rgb[i], im, proj)
            centre += int(im["stable"][h // 2, w // 2])
    print("stable centre pixels", centre, "of", len(AXIS_CAMERAS) * RENDER_B)
    tally.report("axis-parallel rays")
    assert centre >= len(AXIS_CAMERAS)  # derivable: most centre pixels lie inside one face


def test_ray_parallel_to_a_capsule_from_its_first_end():
    """The robot alone, seen from straight below its base column (capsule 0,
    from the base origin up to link 0's frame): the centre ray runs along the
    capsule's axis from the pa side, and must meet the pa cap."""
    from pandasim.sim import PandaSim

    cfg = L.default_config(0, 0, 0)
    cfg.has_table = cfg.has_plane = 0
    sim = PandaSim(config=cfg, num_envs=1)
    q = render_scene("reach").q[:1]
    sim.set_rows(L.F_Q, torch.from_numpy(q.astype(np.float32)))
    ocfg = oracle_config_for(sim.cfg)
    from helpers import oracle_env_with

    env = oracle_env_with(ocfg, q[0])
    base = [float(ocfg.base[k]) for k in range(3)]
    vis = RenderVisual((-1, -1), ((0, 0, 0), (0, 0, 0)))
    w, h = 33, 25
    tally = Tally()
    for snap in (False, True):
        cam = dict(target=(base[0], base[1], base[2] + 0.15), distance=0.5, yaw=0, pitch=90, roll=0)
        view, proj = render_camera(cam, w, h)
        view = _snapped(view) if snap else view
        depth, rgb = render(sim, view, proj, w, h, vis, None)
        im = RO.raycast_image(ocfg, env, view, proj, w, h, vis, None)
        c, r = h // 2, w // 2
        assert im["stable"][c, r] and im["prim"][c, r] == RO.PRIM_ARM and abs(im["t"][c, r] - (0.35 - 0.07)) < 1e-6
        print("snap", snap, "centre: GPU linear depth", float(_linear(depth[0][c, r], proj)), "oracle", im["t"][c, r],
              "rgb", rgb[0][c, r].tolist(), im["rgb"][c, r].tolist())
        assert np.isfinite(depth).all()
        tally.add(("below the column", snap), depth[0], rgb[0], im, proj)
    tally.report("parallel capsule")
