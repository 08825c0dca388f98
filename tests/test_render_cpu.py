"""CPU checks of the camera-image row (§8(f) rank 4, pybullet.py:69-264): the
oracle's restatement of render()/deproject() against the goldens the
reference's own code produced (tests/golden/make_render_golden.py), and the
host-only camera arithmetic of libpandasim (ps_camera) against them."""
import ctypes as C

import numpy as np
import pytest
import render_oracle as RO


def _cams(g):
    for k in range(int(g["n_cameras"])):
        yield k, {n[len(f"c{k}_"):]: v for n, v in g.items() if n.startswith(f"c{k}_")}


def test_oracle_render_postprocessing_matches_reference_goldens(render_golden):
    for k, c in _cams(render_golden):
        pts, cols, pix2d, flat = RO.deproject_image(c["depth_in"], c["tran"], c["px_in"])
        # same numpy operations in the same order: bit for bit
        assert np.array_equal(pts, c["points"]), k
        assert np.array_equal(cols, c["colors"]), k
        assert np.array_equal(pix2d, c["pixels_2d"]), k
        assert np.array_equal(c["depth"], c["depth_in"].astype(np.float64)), k
        # rgb: the reference returns the channel-swapped (cv2 BGR2RGB) pixels
        assert np.array_equal(c["rgb"], c["px_in"][:, :, 2::-1]), k


def test_oracle_deproject_matches_reference_goldens(render_golden):
    for k, c in _cams(render_golden):
        w, h = int(c["camera"][0]), int(c["camera"][1])
        assert np.array_equal(RO.deproject(c["depth"], c["pixels"], c["tran"], w, h), c["deproject"]), k


def test_camera_tran_is_inverse_of_projection_times_view(render_golden):
    for k, c in _cams(render_golden):
        P = np.asarray(c["proj"], np.float64).reshape(4, 4, order="F")
        V = np.asarray(c["view"], np.float64).reshape(4, 4, order="F")
        assert np.allclose(c["tran"] @ (P @ V), np.eye(4), atol=1e-9), k


def test_ps_camera_host_arithmetic(render_golden):
    """libpandasim's ps_camera (host code, no GPU) against the matrices and
    inv(P V) of the goldens (the matrices themselves are the oracle's restated
    formula: unpinned against PyBullet, which is absent)."""
    from pandasim import _lib as L

    lib = L.lib()
    for k, c in _cams(render_golden):
        w, h, tx, ty, tz, dist, yaw, pitch, roll = c["camera"]
        view, proj, tran = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_double * 16)()
        rc = lib.ps_camera((C.c_float * 3)(tx, ty, tz), dist, yaw, pitch, roll, int(w), int(h), view, proj, tran)
        assert rc == 0
        assert np.allclose(np.array(view[:]), c["view"], atol=2e-7), k
        assert np.array_equal(np.array(proj[:], np.float32), c["proj"]), k
        t = np.array(tran[:]).reshape(4, 4)
        assert np.allclose(t, c["tran"], rtol=1e-5, atol=1e-6 * np.abs(c["tran"]).max()), k


# ------------------------------------------------ raycast_image
def _bare(task="reach", **over):
    import oracle as O

    cfg = O.config(task, **over)
    env = O.new_env(cfg)
    for d, v in enumerate([-0.9, 0.41, 0.0, -1.85, 0.0, 2.26, 0.79, 0.0, 0.0]):  # the arm turned towards -y
        env.q[d] = v
    return cfg, env


def _visual(shapes=(-1, -1), halves=((0, 0, 0), (0, 0, 0)), alphas=None):
    from helpers import RenderVisual

    return RenderVisual(shapes, halves, alphas=alphas)


def test_image_of_the_bare_table_from_straight_above():
    """pitch = -90: f = (0, 0, -1), u horizontal, so l = (0.6 u + (0, 0, 1)) / sqrt(1.36)
    and every table pixel has n = (0, 0, 1), |n.l| = 1 / sqrt(1.36)."""
    cfg, env = _bare()
    w, h = 33, 25
    view, proj, _ = RO.camera((0.0, 0.15, 0.0), 0.2, 30.0, -90.0, 0.0, w, h)
    vis = _visual()
    im = RO.raycast_image(cfg, env, view, proj, w, h, vis, None)
    assert np.all(im["role"] == RO.ROLE_TABLE) and np.all(im["prim"] == RO.PRIM_TABLE) and np.all(im["face"] == 4)
    assert np.all(im["stable"]) and not im["ghost"].any()
    assert np.array_equal(im["normal"], np.broadcast_to([0.0, 0.0, 1.0], (h, w, 3)))
    assert np.allclose(im["t"], 0.2, rtol=0, atol=1e-7)  # the view matrix is fp32
    assert np.all(im["t2"] > im["t"])  # the plane below the table
    shade = 0.35 + 0.65 / np.sqrt(1.36)
    want = vis.rgba[RO.ROLE_TABLE, :3] * shade
    assert np.allclose(im["color"], want, rtol=0, atol=1e-7)
    # (0.95, 0.9, 0.85) x 0.90737 x 255 = 219.8, 208.2, 196.7
    assert np.array_equal(im["rgb"], np.broadcast_to(np.array([220, 208, 197], np.uint8), (h, w, 3)))
    assert np.array_equal(im["rgb"][0, 0], np.floor(255 * want + 0.5).astype(np.uint8))


def test_ghost_sphere_over_the_background_blends_exactly():
    cfg, env = _bare(has_table=0, has_plane=0)
    w, h = 21, 15
    view, proj, _ = RO.camera((2.0, 2.0, 1.0), 0.5, 45.0, 20.0, 0.0, w, h)  # looks up and away from the robot
    vis = _visual((RO.VISUAL_SPHERE, -1), ((0.1, 0, 0), (0, 0, 0)))
    tg = np.array([[2.0, 2.0, 1.0, 0, 0, 0, 1], [0, 0, -100.0, 0, 0, 0, 1]])
    im = RO.raycast_image(cfg, env, view, proj, w, h, vis, tg)
    assert np.all(im["role"] == RO.ROLE_BACKGROUND) and np.all(im["depth"] == 1.0) and np.all(np.isinf(im["t"]))
    c, r = h // 2, w // 2
    assert im["ghost"][c, r, 0] and not im["ghost"][..., 1].any() and not im["ghost"][0, 0, 0]
    assert abs(im["ghost_t"][c, r, 0] - 0.4) < 1e-6  # distance 0.5, radius 0.1
    a, ct, bg = vis.rgba[4, 3], vis.rgba[4, :3], vis.rgba[7, :3]
    assert np.array_equal(im["color"][c, r], a * ct + (1 - a) * bg)
    assert np.array_equal(im["color"][0, 0], bg)  # the background is unshaded
    # with no targets, or shape -1, there is no ghost
    for v, t in ((vis, None), (_visual(), tg)):
        im0 = RO.raycast_image(cfg, env, view, proj, w, h, v, t)
        assert not im0["ghost"].any() and np.array_equal(im0["color"][c, r], bg)


def test_ghost_behind_the_table_top_is_not_blended():
    cfg, env = _bare()
    w, h = 21, 15
    view, proj, _ = RO.camera((0.0, 0.15, 0.0), 0.2, 0.0, -90.0, 0.0, w, h)
    vis = _visual((RO.VISUAL_SPHERE, RO.VISUAL_SPHERE), ((0.05, 0, 0), (0.03, 0, 0)))
    tg = np.array([[0.0, 0.15, -0.1, 0, 0, 0, 1], [0.0, 0.15, 0.05, 0, 0, 0, 1]])  # below and above the top
    im = RO.raycast_image(cfg, env, view, proj, w, h, vis, tg)
    c, r = h // 2, w // 2
    assert np.all(im["role"] == RO.ROLE_TABLE)
    assert not im["ghost"][..., 0].any() and abs(im["ghost_t"][c, r, 0] - 0.25) < 1e-6
    assert im["ghost"][c, r, 1] and abs(im["ghost_t"][c, r, 1] - 0.12) < 1e-6
    table = vis.rgba[1, :3] * (0.35 + 0.65 / np.sqrt(1.36))
    a = vis.rgba[5, 3]
    assert np.allclose(im["color"][c, r], a * vis.rgba[5, :3] + (1 - a) * table, rtol=0, atol=1e-7)
    assert np.allclose(im["color"][0, 0], table, rtol=0, atol=1e-7) and not im["ghost"][0, 0].any()
    assert np.abs(im["depth"] - im["depth"][0, 0]).max() < 1e-12  # ghosts write no depth


def test_image_centre_ray_hits_the_rotated_box_on_the_face_geometry_says():
    """A 4 x 6 x 10 cm box turned 90 degrees about x: its +y axis points up,
    its +z axis towards world -y."""
    cfg, env = _bare("push", object_half=(0.02, 0.03, 0.05))
    s = np.sqrt(0.5)
    for k, v in enumerate((0.1, 0.3, 0.2)):
        env.obj[0].pos[k] = v
    for k, v in enumerate((s, 0.0, 0.0, s)):
        env.obj[0].quat[k] = v
    w, h = 41, 31
    c, r = h // 2, w // 2
    cases = [((0.0, -90.0), 2, (0, 0, 1), 0.2 - 0.03),  # from above: local +y, 3 cm above the centre
             ((0.0, 0.0), 4, (0, -1, 0), 0.2 - 0.05),  # looking along world +y: local +z, 5 cm in front
             ((90.0, 0.0), 0, (1, 0, 0), 0.2 - 0.02),  # looking along world -x: local +x
             ((-90.0, 0.0), 1, (-1, 0, 0), 0.2 - 0.02),
             ((180.0, 0.0), 5, (0, 1, 0), 0.2 - 0.05),
             ((0.0, 90.0), 3, (0, 0, -1), 0.2 - 0.03)]
    cfg.has_table = cfg.has_plane = 0  # the last camera looks up from below
    for (yaw, pitch), face, n, t in cases:
        view, proj, _ = RO.camera((0.1, 0.3, 0.2), 0.2, yaw, pitch, 0.0, w, h)
        im = RO.raycast_image(cfg, env, view, proj, w, h, _visual(), None)
        assert im["role"][c, r] == RO.ROLE_OBJECT1 and im["prim"][c, r] == RO.PRIM_OBJECT, (yaw, pitch)
        assert im["face"][c, r] == face, (yaw, pitch, im["face"][c, r])
        assert np.allclose(im["normal"][c, r], n, rtol=0, atol=1e-12), (yaw, pitch, im["normal"][c, r])
        assert abs(im["t"][c, r] - t) < 1e-6, (yaw, pitch, im["t"][c, r])
        assert im["stable"][c, r]


def test_stable_mask_marks_a_pixel_and_its_neighbours():
    key = np.zeros((5, 6), int)
    key[0, 0] = 1  # a corner: it and its three neighbours
    key[3, 4] = 2  # an inner pixel: it and its eight neighbours
    st = RO.stable_mask(key, np.zeros((5, 6, 2), bool))
    want = np.ones((5, 6), bool)
    want[:2, :2] = False
    want[2:5, 3:6] = False
    assert np.array_equal(st, want)
    flag = np.zeros((5, 6, 2), bool)
    flag[4, 0, 1] = True
    want[3:, :2] = False
    assert np.array_equal(RO.stable_mask(key, flag), want)


def test_raycast_image_depth_equals_raycast_depth():
    import oracle as O
    from helpers import RENDER_B, RENDER_H, RENDER_W, render_camera, render_scene

    cfg = O.config("stack")
    env = O.new_env(cfg)
    O.reset(cfg, env, seed=3)  # unit quaternions: the very same arithmetic, bit for bit
    view, proj, _ = RO.camera((0, 0, 0.1), 0.8, 30.0, -35.0, 20.0, 40, 30)
    im = RO.raycast_image(cfg, env, view, proj, 40, 30, _visual(), None)
    assert np.array_equal(im["depth"], RO.raycast_depth(cfg, env, view, proj, 40, 30))
    assert len(np.unique(im["role"])) >= 4
    # the fixtures' quaternions are fp32 roundings of unit ones, which raycast_image normalises
    sc = render_scene("stack")
    cfg = sc.oracle_cfg()
    for cam in sc.cameras:
        view, proj = render_camera(cam)
        for i, im in enumerate(sc.oracle_images(cam)):
            ref = RO.raycast_depth(cfg, sc.oracle_env(cfg, i), view, proj, RENDER_W, RENDER_H)
            st = im["stable"]
            assert np.array_equal(im["depth"][st] < 1.0, ref[st] < 1.0), (cam["name"], i)
            assert np.allclose(im["depth"][st], ref[st], rtol=0, atol=1e-6), (cam["name"], i)
    assert i == RENDER_B - 1


@pytest.mark.parametrize("task", ["reach", "push", "slide", "stack"])
def test_render_fixtures_meet_their_coverage_conditions(task):
    """What tests/test_gpu_render_image.py relies on, by the oracle alone: at
    least 70 % stable pixels in every image, at least 20 stable pixels of every
    role, face and ghost case of the scene, two cameras with roll, one at
    pitch -90 and a close-up in which arm primitives straddle the near plane."""
    from helpers import RENDER_B, check_render_coverage, render_scene

    sc = render_scene(task)
    ims = {cam["name"]: sc.oracle_images(cam) for cam in sc.cameras}
    shares, counts = check_render_coverage(sc, ims)
    print(task, "min stable share %.3f" % min(shares.values()), counts)
    assert sorted(c["roll"] for c in sc.cameras)[-2:] == [30, 90] and any(c["pitch"] == -90 for c in sc.cameras)
    close = sc.cameras[sc.closeup]
    assert abs(close["distance"] - 0.35) < 1e-9
    assert max(sc.straddles_near(close, i) for i in range(RENDER_B)) >= 1
    # the random orientations are far from the identity
    assert np.all(np.abs(sc.obj_quat[..., 3]) < 0.95)
    want = {"plane", "table", "robot", "background", "ghost 0 over background", "ghost 0 over ghost 1",
            "ghost 1 behind the table"}
    if sc.n_objects:
        want |= {"object 1", "ghost 0 over object", "ghost 0 behind object"}
        want |= {f"object 1 face {f}" for f in (("side", "cap -z", "cap +z") if task == "slide"
                                                else ("+x", "-x", "+y", "-y", "+z", "-z"))}
    if sc.n_objects == 2:
        want.add("object 2")
    assert want <= set(sc.cases)


def test_ps_camera_matches_the_oracle_camera_with_roll():
    """The goldens' cameras all have roll = 0; the image fixtures' do not."""
    from helpers import RENDER_H, RENDER_W, render_scene
    from pandasim import _lib as L

    lib = L.lib()
    for cam in render_scene("push").cameras:
        view, proj, tran = (C.c_float * 16)(), (C.c_float * 16)(), (C.c_double * 16)()
        rc = lib.ps_camera((C.c_float * 3)(*cam["target"]), cam["distance"], cam["yaw"], cam["pitch"], cam["roll"],
                           RENDER_W, RENDER_H, view, proj, tran)
        assert rc == 0
        v, p, _ = RO.camera(cam["target"], cam["distance"], cam["yaw"], cam["pitch"], cam["roll"], RENDER_W, RENDER_H)
        assert np.allclose(np.array(view[:]), v, rtol=0, atol=2e-7), cam["name"]
        assert np.array_equal(np.array(proj[:], np.float32), np.array(p, np.float32)), cam["name"]


def test_mgrid_sizes_the_reference_cannot_render():
    from pandasim.sim import PandaSim

    PandaSim._check_image_size(480, 480)
    PandaSim._check_image_size(64, 48)
    with pytest.raises(ValueError):
        PandaSim._check_image_size(49, 64)  # np.mgrid[-1:1:2/49] has 50 entries
