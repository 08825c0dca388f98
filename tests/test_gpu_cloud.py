"""GPU tests of the fused multi-view point-cloud observation (ps_point_cloud,
PandaSim.point_cloud).

The yardstick is the composition the call fuses, run with the same library:
per view ps_render and ps_deproject_image, then in torch `valid & crop`, the
views concatenated in order, and the ranks of tests/test_cloud_cpu.py's
pure-Python sampler.  points (against .float() of the f64 points), colors,
source and count must be equal bit for bit: no tolerance anywhere.

The crop compares the f64 world point with the box's f32 corners (ps_cloud_crop
holds floats), so the yardstick rounds the corners to f32 first.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cloud_cpu import GOLDEN, MASK64, ranks

pytestmark = pytest.mark.gpu

B, K, SEED = 4, 257, 2024
TASKS = ("push", "stack", "reach")  # one object, two objects, none
SIZES = ((40, 40), (48, 32))  # 1 600 pixels = 6 tiles + a 64-pixel partial one; non-square
MIN_CLOUD = 64  # every env's merged cloud in the non-empty cases
CROPS = {"none": None,
         "table": ((-10.0, -10.0, 0.002), (10.0, 10.0, 10.0)),  # lo z = 0.002: the table-dropping filter
         "box": ((-0.15, -0.15, 0.002), (0.15, 0.15, 0.5)),  # cuts the cloud on every side
         "empty": ((10.0, 10.0, 10.0), (11.0, 11.0, 11.0))}


def views3():
    import pandasim

    return list(pandasim.GRASP_VIEWS[:3])


def stepped_env(task, num_envs=B, seed=777):
    """`num_envs` envs of `task`, made to differ: a seeded reset and 3 random steps."""
    from pandasim.envs import PandaVecEnv

    env = PandaVecEnv(task, "sparse", "ee", num_envs, "cuda:0", autoreset=False)
    env.reset(seed=seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    for _ in range(3):
        env.step(torch.rand(num_envs, env.action_dim, device="cuda", generator=g) * 2 - 1)
    return env


@pytest.fixture(scope="module")
def envs():
    return {task: stepped_env(task) for task in TASKS}


def unfused(sim, views, w, h):
    """Per view ps_render + ps_deproject_image: valid [B, V * n] bool, points
    [B, V * n, 3] f64 and rgb [B, V * n, 3] u8 in merged (view, pixel) order."""
    from pandasim.sim import _ptr

    nb, n = sim.num_envs, w * h
    valid, points, rgb = [], [], []
    for kw in views:
        view, proj, tran = sim.get_cam2world_transforms(w, h, **kw)
        depth, img = sim.get_camera_image(w, h, view, proj)
        pts = torch.empty(nb, n, 3, dtype=torch.float64, device="cuda")
        ok = torch.empty(nb, n, dtype=torch.uint8, device="cuda")
        T = (C.c_double * 16)(*tran.reshape(-1).tolist())
        sim._call("ps_deproject_image", sim._ctx, _ptr(depth), T, w, h, _ptr(pts), _ptr(ok), None, sim._stream())
        valid.append(ok.bool())
        points.append(pts)
        rgb.append(img.reshape(nb, n, 3))
    return torch.cat(valid, 1), torch.cat(points, 1), torch.cat(rgb, 1)


_unfused_cache = {}


def unfused_of(envs, task, size):
    key = (task, size)
    if key not in _unfused_cache:
        _unfused_cache[key] = unfused(envs[task].sim, views3(), *size)
    return _unfused_cache[key]


def expected(valid, points, rgb, crop, n_points, seed, env_offset=0):
    """The merged, cropped and sampled cloud from the unfused arrays."""
    keep = valid.clone()
    if crop is not None:
        lo = torch.tensor(np.asarray(crop[0], np.float32).astype(np.float64), device=points.device)
        hi = torch.tensor(np.asarray(crop[1], np.float32).astype(np.float64), device=points.device)
        keep &= ((points > lo) & (points < hi)).all(-1)
    nb = keep.shape[0]
    out = {"points": torch.zeros(nb, n_points, 3, dtype=torch.float32), "count": torch.zeros(nb, dtype=torch.int32),
           "colors": torch.zeros(nb, n_points, 3, dtype=torch.uint8),
           "source": torch.full((nb, n_points), -1, dtype=torch.int32)}
    for b in range(nb):
        merged = torch.nonzero(keep[b]).reshape(-1).cpu()  # ascending: view 0 first, pixel order inside a view
        m = int(merged.numel())
        out["count"][b] = m
        if m == 0:
            continue
        src = merged[torch.tensor(ranks(seed, b + env_offset, n_points, m))]
        out["source"][b] = src.int()
        out["points"][b] = points[b].cpu()[src].float()
        out["colors"][b] = rgb[b].cpu()[src]
    return out


def assert_same(got, want, what):
    for k in ("count", "source", "colors", "points"):
        g, w = got[k].cpu().numpy(), want[k].cpu().numpy()
        if k == "points":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, int((g != w).sum()))


@pytest.mark.parametrize("crop", list(CROPS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("task", TASKS)
def test_point_cloud_equals_the_unfused_composition(envs, task, size, crop):
    w, h = size
    valid, points, rgb = unfused_of(envs, task, size)
    want = expected(valid, points, rgb, CROPS[crop], K, SEED)
    print(task, size, crop, "M_b =", want["count"].tolist())
    if crop == "empty":
        assert int(want["count"].max()) == 0  # the unfused path finds nothing in the box
    else:
        assert int(want["count"].min()) >= MIN_CLOUD
    if crop == "box":  # the crop is felt: it drops points of every env
        assert bool((want["count"] < expected(valid, points, rgb, None, K, SEED)["count"]).all())
    got = envs[task].sim.point_cloud(views3(), n_points=K, width=w, height=h, seed=SEED, crop=CROPS[crop])
    assert got["points"].shape == (B, K, 3) and got["points"].dtype == torch.float32
    assert got["colors"].shape == (B, K, 3) and got["colors"].dtype == torch.uint8
    assert got["source"].shape == (B, K) and got["source"].dtype == torch.int32
    assert got["count"].shape == (B,) and got["count"].dtype == torch.int32
    assert_same(got, want, (task, size, crop))
    if crop == "empty":
        assert not got["points"].any() and not got["colors"].any() and bool((got["source"] == -1).all())


def test_workload_size_one_env_four_views():
    """The workload's own shape: 480x480, the four grasp views, K = 5 000."""
    import pandasim

    env = stepped_env("push", num_envs=1, seed=5)
    views = list(pandasim.GRASP_VIEWS)
    valid, points, rgb = unfused(env.sim, views, 480, 480)
    want = expected(valid, points, rgb, None, 5000, 1)
    assert int(want["count"][0]) > 10000
    got = env.point_cloud(views, n_points=5000, width=480, height=480, seed=1)  # the env's thin forwarder
    assert_same(got, want, "480x480")
    assert len(torch.unique(got["source"] // (480 * 480))) == 4  # samples from every view
    assert_same(env.point_cloud(seed=1), want, "defaults")  # GRASP_VIEWS, 5 000 points, 480x480


def test_sample_does_not_depend_on_the_batch(envs):
    """Sample j of env b is the same whether the batch holds 4 envs or env b's
    state alone in a 1-env sim: there the env is number 0, so the counter
    c = b * K + j is reached by the seed SEED + golden * b * K (mod 2^64)."""
    from pandasim.envs import PandaVecEnv

    big = envs["stack"].sim
    full = big.point_cloud(views3(), n_points=K, width=40, height=40, seed=SEED)
    one = PandaVecEnv("stack", "sparse", "ee", 1, "cuda:0", autoreset=False)
    one.reset(seed=1)
    for b in range(B):
        one.sim.f[:, 0] = big.f[:, b]
        one.sim.goal[:, 0] = big.goal[:, b]
        alone = one.sim.point_cloud(views3(), n_points=K, width=40, height=40, seed=(SEED + GOLDEN * b * K) & MASK64)
        assert int(alone["count"][0]) == int(full["count"][b]) >= MIN_CLOUD
        for k in ("source", "colors", "points"):
            assert torch.equal(alone[k][0], full[k][b]), (b, k)


def test_same_seed_repeats_and_another_seed_differs(envs):
    sim = envs["push"].sim
    a = sim.point_cloud(views3(), n_points=K, width=40, height=40, seed=9)
    b = sim.point_cloud(views3(), n_points=K, width=40, height=40, seed=9)
    c = sim.point_cloud(views3(), n_points=K, width=40, height=40, seed=10)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["count"], c["count"])
    assert not torch.equal(a["source"], c["source"])


def _raw_call(sim, views, w, h, n_points, seed, points, colors, source, count, ws, crop=None, n_views=None,
              ctx="ctx", state="state", vis="vis"):
    """ps_point_cloud through ctypes, returning its code (no exception)."""
    from pandasim import _lib as L
    from pandasim.sim import _ptr

    cv = (L.CloudView * max(len(views), 1))()
    for v, kw in zip(cv, views):
        view, proj, tran = sim.get_cam2world_transforms(w or 40, h or 40, **kw)
        v.view[:], v.proj[:], v.tran_pix_world[:] = view, proj, tran.reshape(-1).tolist()
    visual = sim._visual()
    targets = sim._target_poses().contiguous()
    with torch.cuda.device(sim.device):
        return L.lib().ps_point_cloud(sim._ctx if ctx else None, _ptr(sim.state) if state else None,
                                      cv if views else None, len(views) if n_views is None else n_views, w, h,
                                      C.byref(visual) if vis else None, _ptr(targets), crop, n_points, seed,
                                      _ptr(points), _ptr(colors), _ptr(source), _ptr(count), _ptr(ws), sim._stream())


def test_optional_outputs_and_argument_errors(envs):
    from pandasim import _lib as L

    sim = envs["push"].sim
    w = h = 40
    views = views3()
    full = sim.point_cloud(views, n_points=K, width=w, height=h, seed=SEED)
    ws = torch.empty(L.lib().ps_cloud_workspace_bytes(B, 3, w, h), dtype=torch.uint8, device="cuda")

    def bufs():
        return (torch.empty(B, K, 3, dtype=torch.float32, device="cuda"),
                torch.empty(B, K, 3, dtype=torch.uint8, device="cuda"),
                torch.empty(B, K, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"))

    # colors / source / count may each be NULL; what is written stays the same
    for drop in range(1, 4):
        out = list(bufs())
        out[drop] = None
        assert _raw_call(sim, views, w, h, K, SEED, *out, ws) == 0
        torch.cuda.synchronize()
        for k, t in zip(("points", "colors", "source", "count"), out):
            assert t is None or torch.equal(t, full[k]), (drop, k)
    p, c, s, n = bufs()
    bad = L.ERRORS
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, ws, ctx=None)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, ws, state=None)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, [], w, h, K, SEED, p, c, s, n, ws, n_views=3)] == "PS_ERR_ARG"  # views NULL
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, ws, vis=None)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, K, SEED, None, c, s, n, ws)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, None)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, ws, n_views=0)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, K, SEED, p, c, s, n, ws, n_views=9)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, 0, SEED, p, c, s, n, ws)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, w, h, -5, SEED, p, c, s, n, ws)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, 0, h, K, SEED, p, c, s, n, ws)] == "PS_ERR_ARG"
    assert bad[_raw_call(sim, views, 4096, 4097, K, SEED, p, c, s, n, ws)] == "PS_ERR_ARG"  # 65 552 pixel tiles
    with pytest.raises(ValueError):
        sim.point_cloud([], n_points=K, width=w, height=h)
    with pytest.raises(ValueError):
        sim.point_cloud(views, n_points=K, width=49, height=64)  # _check_image_size, as render()
    # nothing faulted: the next call still computes the same cloud
    torch.cuda.synchronize()
    again = sim.point_cloud(views, n_points=K, width=w, height=h, seed=SEED)
    for k in full:
        assert torch.equal(again[k], full[k]), k


def test_plugin_path_sim_with_ghost_targets():
    """pandasim.core's sim (create_* bodies, ghost targets placed by
    set_base_pose) equals its own unfused composition."""
    import pandasim

    plug = pandasim.make("PandaPush-v3", num_envs=3, fused=False)
    plug.reset(seed=4)
    sim = plug.env.sim
    assert sim._ghost_shape  # the target is a ghost body of the plugin path
    valid, points, rgb = unfused(sim, views3(), 40, 40)
    want = expected(valid, points, rgb, None, K, 7)
    assert int(want["count"].min()) >= MIN_CLOUD
    assert_same(sim.point_cloud(views3(), n_points=K, width=40, height=40, seed=7), want, "plugin")
