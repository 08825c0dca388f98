"""GPU tests of the stream contract of include/pandasim.h: "Calls are
asynchronous on the given HIP stream" and, for the cloud calls, "every call is
ordered on `stream`".  Every other module runs on the default stream, where
everything is serialised whatever stream a kernel was launched on; this one
leaves it.  The comparisons are all "the same bits as the default stream":
what a kernel computes is the other modules' business, here only when it runs.

The protocol, one table row per entry point.  On the default stream two valid
inputs A and B give ref_A and ref_B, which must differ in bits (asserted per
row: without it the row could not fail).  The buffer the call reads holds A.
On a side stream s, without host synchronisation: a delay, buf.copy_(B), the
call into fresh outputs, a clone of each output.  After s.synchronize() every
clone must be ref_B bit for bit.  A kernel that is not ordered behind s runs
while the delay holds s back, reads A and gives ref_A (or a mixture, when one
stage of a multi-kernel call strayed).  A and B are real simulator states
(reset(seed=1); reset(seed=2) and three random steps), finite clouds and
in-range indices, so a stray kernel computes a wrong but harmless result.
ps_init_state's result does not depend on what the buffer held, so there the
misordered result is the other one: the call runs early and copy_(B) then
overwrites it, and "ref_A" is B itself.

A row has power only if the call is enqueued while the delay still holds s
back, so every row also measures the host time of its enqueue and asserts
that it is less than half the delay.  A wrapper that blocks the host on the
current stream cannot pass that, and its row goes to the entry point through
PandaSim._call with PandaSim._stream(), the same plumbing the wrappers use:
  ps_reset                 PandaVecEnv.reset uploads the seeds (a blocking copy);
  ps_deproject_pixels      PandaSim.deproject reads the pixels back to refuse one outside the image;
  ps_cloud_set_abstraction PandaSim.group_cloud uploads the start indices (a blocking copy).
The composites segment_cloud and predict_waypoints call group_cloud twice, so
the host waits for the delay at the first one: their rows (marked `blocks`)
check only that the result on a side stream is the default stream's.
Entry points without a Python wrapper (ps_init_state, ps_cloud_normalize,
ps_cloud_fps, ps_cloud_ball_query, ps_cloud_group, ps_cloud_three_nn,
ps_cloud_interpolate, ps_deproject_image alone) are called the same way.

The control, one test per family, produces the misordering from outside with
a correct library: the call is issued under a second side stream t while the
delay and copy_(B) stay on s, and the result must not be ref_B.

The delay is torch.cuda._sleep(cycles) where torch has it, else a chain of
torch.mm calls; it is calibrated once per module with events on the side
stream, doubling (at most MAX_DOUBLINGS times) until it is DELAY_FACTOR = 10
times the slowest row's default-stream call time -- a margin over launch
latency and clock ramp, not a measured quantity.  Both times are printed.
Measured on an MI355X: the delay is torch.cuda._sleep(2^27) = 55.9 ms after
seven doublings; the slowest row is ps_step[stack-1], 4.46 ms; ratio 12.5.  The
module's budget is one delay per row, control and first-use test (48 + 5 + 2)
and one for the calibration: 56 delays, 3.1 s; it runs in about 7 s with its
set-up.

Not covered, deliberately: graph capture (two entry points allocate on first
use, which capture forbids), more than one device, more than two side streams,
one context used from two streams at once (documented as unsupported).
Every ps_* function of include/pandasim.h that takes a stream has a row or is
part of a named composite; ps_camera, ps_*_bytes, ps_create and the getters
and setters without a stream argument are host-only and have none.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from cloud_helpers import DEV, dev, make_sims, net, random_groups, raw_group, same_bits, upload

pytestmark = pytest.mark.gpu

DELAY_FACTOR = 10  # the delay is at least this many times the slowest row's call
MAX_DOUBLINGS = 16
FIRST_CYCLES = 1 << 20  # where the doubling of torch.cuda._sleep's argument starts
B_ENV = 70  # one full wave plus six lanes
CAM_B, CAM_W, CAM_H, CAM_K = 4, 40, 40, 257  # tests/test_gpu_cloud.py's batch, image and sample count
CROP_BOX = ((-0.15, -0.15, 0.002), (0.15, 0.15, 0.5))  # its "box" crop
NET_N = 600  # tests/test_gpu_net.py's cloud
EE_LINK = 11


# ------------------------------------------------------------------ plumbing
def _bitwise(t):
    """A tensor as integers of its own width (same_bits views only f32)."""
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype == torch.bool:
        return t.to(torch.uint8)
    return t


def all_same(got, want):
    return len(got) == len(want) and all(same_bits(_bitwise(g), _bitwise(w)) for g, w in zip(got, want))


def clones(outs):
    return [o.clone() for o in outs]


class Row:
    """One entry point: `bufs` are the device buffers the call reads, A and B
    what they hold (lists as long as bufs), call() enqueues the library call on
    the current stream and returns its outputs.  `blocks` names why the call
    blocks the host (no power check); `misordered` replaces ref_A where the
    result does not depend on the buffer."""

    def __init__(self, name, family, bufs, A, B, call, blocks=None, misordered=None):
        self.name, self.family, self.bufs, self.A, self.B, self.call = name, family, bufs, A, B, call
        self.blocks, self.misordered = blocks, misordered
        self.ref_A = self.ref_B = self.ms = None

    def load(self, X):
        for buf, x in zip(self.bufs, X):
            buf.copy_(x)

    def prepare(self):
        """ref_A, ref_B and the default-stream time of the call (events around f(B))."""
        self.load(self.A)
        self.ref_A = clones(self.call())
        self.load(self.B)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.ref_B = clones(self.call())
        e1.record()
        torch.cuda.synchronize()
        self.ms = e0.elapsed_time(e1)
        if self.misordered is not None:
            self.ref_A = clones(self.misordered)
        return self


def behind_delay(row, delay, s, t=None):
    """Step 3 of the protocol: on s a delay, copy_(B), the call (under t if
    given: the control) and the clones -> (clones, host ms of the enqueue)."""
    row.load(row.A)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
        t0 = time.perf_counter()
        row.load(row.B)
        with torch.cuda.stream(s if t is None else t):
            got = clones(row.call())
        host_ms = (time.perf_counter() - t0) * 1e3
    s.synchronize()
    if t is not None:
        t.synchronize()
    torch.cuda.synchronize()
    return got, host_ms


def _ptr(t):
    from pandasim.sim import _ptr as p

    return p(t)


def two_states(env, steps=3):
    """Two real states of `env` (fused or plugin path) and one more batch of
    actions: after reset(seed=1), and after reset(seed=2) and `steps` random steps."""
    sim = env.sim
    n_act = env.action_dim if hasattr(env, "action_dim") else env.robot.action_space.shape[0]
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    env.reset(seed=1)
    a = sim.state.clone()
    env.reset(seed=2)
    for _ in range(steps):
        env.step(torch.rand(sim.num_envs, n_act, device=DEV, generator=g) * 2 - 1)
    b = sim.state.clone()
    acts = torch.rand(sim.num_envs, n_act, device=DEV, generator=g) * 2 - 1
    torch.cuda.synchronize()
    return a, b, acts


def fused_env(task, num_envs=B_ENV, lanes=0):
    from pandasim.envs import PandaVecEnv

    return PandaVecEnv(task, "sparse", "ee", num_envs, DEV, autoreset=False, lanes_per_env=lanes)


# --------------------------------------------------------------------- rows
def env_rows():
    """Env and engine: the input is the state buffer; the outputs are obs, ag,
    dg, reward, flags and the state afterwards."""
    from pandasim.envs import make

    rows = []

    def step_row(name, task, lanes, oriented=False):
        env = fused_env(task, lanes=lanes)
        assert env.lanes_per_env == lanes
        sim = env.sim
        a, b, acts = two_states(env)
        kw = {}
        if oriented:
            g = torch.Generator(device="cuda")
            g.manual_seed(5)
            kw["euler_xyz"] = torch.tensor([180.0, 0.0, 0.0], device=DEV) + \
                (torch.rand(B_ENV, 3, device=DEV, generator=g) * 40 - 20)

        def call():
            sim._call("ps_mark_motor_rows_dirty", sim._ctx)  # the buffer was copied into: see include/pandasim.h
            obs, r, te, tr, _ = env.step(acts, **kw)
            return [obs["observation"], obs["achieved_goal"], obs["desired_goal"], r, te, tr, sim.state]

        rows.append(Row(name, "env", [sim.state], [a], [b], call))
        return env, a, b

    env, a, b = step_row("ps_step[push-1]", "push", 1)
    sim = env.sim

    def init_state():
        sim._call("ps_init_state", sim._ctx, _ptr(sim.state), sim._stream())
        return [sim.state]

    rows.append(Row("ps_init_state", "env", [sim.state], [a], [b], init_state, misordered=[b]))

    seeds = torch.arange(100, 100 + B_ENV, dtype=torch.int64, device=DEV)
    mask = (torch.arange(B_ENV, device=DEV) % 3 != 0).to(torch.uint8)

    def reset():
        # zeros: the rows of the envs outside the mask are left
        obs = torch.zeros(B_ENV, env.obs_dim, device=DEV)
        ag, dg = torch.zeros(B_ENV, env.goal_dim, device=DEV), torch.zeros(B_ENV, env.goal_dim, device=DEV)
        sim._call("ps_reset", sim._ctx, _ptr(sim.state), _ptr(mask), _ptr(seeds), _ptr(obs), _ptr(ag), _ptr(dg),
                  sim._stream())
        return [obs, ag, dg, sim.state]

    rows.append(Row("ps_reset", "env", [sim.state], [a], [b], reset))
    step_row("ps_step[push-16]", "push", 16)
    step_row("ps_step[pick_and_place-8]", "pick_and_place", 8)
    step_row("ps_step[stack-1]", "stack", 1)
    step_row("ps_step_oriented[push-1]", "push", 1, oriented=True)
    for env_id in ("PandaPush-v3", "PandaStack-v3"):
        penv = make(env_id, num_envs=B_ENV, device=DEV, fused=False)
        psim = penv.sim
        pa, pb, _ = two_states(penv)
        rows.append(Row(f"ps_sim_step[{env_id}]", "env", [psim.state], [pa], [pb],
                        (lambda psim: lambda: (psim.step(), [psim.state])[1])(psim)))
    return rows


def query_rows():
    from pandasim.utils import goal_reward_and_success

    env = fused_env("push", lanes=1)
    sim = env.sim
    a, b, _ = two_states(env)
    state = ([sim.state], [a], [b])
    rows = [Row("ps_link_state", "queries", *state, lambda: list(sim.link_state(EE_LINK)))]
    sim.state.copy_(a)
    pos = (sim.link_state(EE_LINK)[0] + torch.tensor([0.03, -0.02, 0.04], device=DEV)).contiguous()
    orn = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).expand(B_ENV, 4).contiguous()
    rows.append(Row("ps_inverse_kinematics", "queries", *state,
                    lambda: [sim.inverse_kinematics("panda", EE_LINK, pos, orn)]))
    rows.append(Row("ps_base_state", "queries", *state, lambda: list(sim._base_state("object"))))

    seeds = torch.arange(7, 7 + B_ENV, dtype=torch.int64, device=DEV)
    mask = (torch.arange(B_ENV, device=DEV) % 2 == 0).to(torch.uint8)  # the other envs draw from the state's rows

    def rng():
        sim.seed(seeds, mask)
        return [sim.uniform([0.0, -1.0, 2.0], [1.0, 1.0, 5.0]), sim.random_rotation(), sim.state]

    rows.append(Row("ps_rng_seed+uniform+rotation", "queries", *state, rng))

    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    r = lambda *shape: torch.rand(*shape, device=DEV, generator=g)
    ag, ag_a, ag_b, dg = torch.empty(B_ENV, 3, device=DEV), r(B_ENV, 3) * 0.1, r(B_ENV, 3) * 0.1, r(B_ENV, 3) * 0.1
    rows.append(Row("ps_compute_reward", "queries", [ag], [ag_a], [ag_b],
                    lambda: list(goal_reward_and_success(ag, dg, "dense", task="push"))))
    eu, eu_a, eu_b = torch.empty(B_ENV, 3, device=DEV), r(B_ENV, 3) * 160 - 80, r(B_ENV, 3) * 160 - 80
    rows.append(Row("ps_euler_xyz_to_quat", "queries", [eu], [eu_a], [eu_b], lambda: [sim.euler_xyz_to_quat(eu)]))
    qa, qb = (torch.nn.functional.normalize(r(B_ENV, 4) * 2 - 1, dim=1) for _ in range(2))
    q = torch.empty(B_ENV, 4, device=DEV)
    rows.append(Row("ps_quat_to_euler_xyz", "queries", [q], [qa], [qb], lambda: [sim.quat_to_euler_xyz(q)]))
    torch.cuda.synchronize()
    return rows


def motion_rows_of(task):
    """The plan calls (the output is the plan buffer) and ps_motion_run (the
    inputs are the state and the plan) in one scene."""
    env = fused_env(task)
    sim = env.sim
    a, b, _ = two_states(env)
    sim.state.copy_(a)
    g = torch.Generator(device="cuda")
    g.manual_seed(13)
    goal = sim.link_state(EE_LINK)[0] + (torch.rand(B_ENV, 3, device=DEV, generator=g) * 0.12 - 0.06)
    goal[:, 2] = goal[:, 2].clamp(min=0.05)
    goal = goal.contiguous()
    quat = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).expand(B_ENV, 4).contiguous()
    mask = (torch.arange(B_ENV, device=DEV) % 7 != 0).to(torch.uint8)
    width = torch.rand(B_ENV, device=DEV, generator=g) * 0.08
    state = ([sim.state], [a], [b])

    def planned(fill):
        plan = sim.motion_plan()
        fill(plan)
        return plan

    fills = {"ps_plan_move": lambda plan: sim.plan_move(plan, goal, quat, mask),
             "ps_plan_grasp": lambda plan: sim.plan_grasp(plan, mask),
             "ps_plan_release": lambda plan: sim.plan_release(plan, width, mask)}
    rows = [Row(f"{name}[{task}]", "motion", *state, (lambda fill: lambda: [planned(fill).buf])(fill))
            for name, fill in fills.items()]
    plans = []
    for st in (a, b):
        sim.state.copy_(st)
        plans.append(planned(fills["ps_plan_move"]).buf)
    plan = sim.motion_plan()

    def run():
        sim.motion_run(plan, 3)
        return [sim.state, plan.buf]

    rows.append(Row(f"ps_motion_run[{task}]", "motion", [sim.state, plan.buf], [a, plans[0]], [b, plans[1]], run))
    torch.cuda.synchronize()
    return rows


def motion_rows():
    return motion_rows_of("reach") + motion_rows_of("pick_and_place")


def camera_rows():
    import pandasim

    views = list(pandasim.GRASP_VIEWS[:3])
    env = fused_env("push", CAM_B)
    sim = env.sim
    a, b, _ = two_states(env)
    state = ([sim.state], [a], [b])
    view, proj, tran = sim.get_cam2world_transforms(CAM_W, CAM_H, **views[0])
    T = (C.c_double * 16)(*tran.reshape(-1).tolist())
    n = CAM_W * CAM_H
    rows = [Row("ps_render", "camera", *state, lambda: list(sim.get_camera_image(CAM_W, CAM_H, view, proj)))]

    def render():
        out = sim.render(CAM_W, CAM_H, **views[0])
        return [out[k] for k in ("depth", "colors", "points", "valid", "pixels_2d")]

    rows.append(Row("render (ps_render + ps_deproject_image)", "camera", *state, render))
    depths = []
    for st in (a, b):
        sim.state.copy_(st)
        depths.append(sim.get_camera_image(CAM_W, CAM_H, view, proj)[0].clone())
    depth = torch.empty_like(depths[0])

    def deproject_image():
        pts = torch.empty(CAM_B, n, 3, dtype=torch.float64, device=DEV)
        ok = torch.empty(CAM_B, n, dtype=torch.uint8, device=DEV)
        pix = torch.empty(CAM_B, n, 2, dtype=torch.float64, device=DEV)
        sim._call("ps_deproject_image", sim._ctx, _ptr(depth), T, CAM_W, CAM_H, _ptr(pts), _ptr(ok), _ptr(pix),
                  sim._stream())
        return [pts, ok, pix]

    rows.append(Row("ps_deproject_image", "camera", [depth], [depths[0]], [depths[1]], deproject_image))
    rng = np.random.default_rng(4)
    n_pix = 77
    pixels = dev(np.stack([rng.integers(0, CAM_W, (CAM_B, n_pix)), rng.integers(0, CAM_H, (CAM_B, n_pix))], -1)
                 .astype(np.int32))

    def deproject_pixels():
        pts = torch.empty(CAM_B, n_pix, 3, dtype=torch.float64, device=DEV)
        sim._call("ps_deproject_pixels", sim._ctx, _ptr(depth), _ptr(pixels), n_pix, T, CAM_W, CAM_H, _ptr(pts),
                  sim._stream())
        return [pts]

    rows.append(Row("ps_deproject_pixels", "camera", [depth], [depths[0]], [depths[1]], deproject_pixels))
    for name, crop in (("uncropped", None), ("cropped", CROP_BOX)):
        rows.append(Row(f"ps_point_cloud[{name}]", "camera", *state,
                        (lambda crop: lambda: list(sim.point_cloud(views, CAM_K, CAM_W, CAM_H, 2024, crop).values()))(crop)))

    # the push case of tests/test_gpu_keypoint.py: B = 3, 64 x 48, K = 300, the object's pixel in view 0
    kB, kw, kh, kK = 3, 64, 48, 300
    kenv = fused_env("push", kB)
    ksim = kenv.sim
    ka, kb, _ = two_states(kenv)
    ksim.state.copy_(ka)
    cloud = ksim.point_cloud(views, kK, kw, kh, 11)
    px = ksim.project_to_pixels(ksim.get_base_position("object").reshape(kB, 1, 3), kw, kh, **views[0])
    rows.append(Row("ps_cloud_keypoint_features", "camera", [ksim.state], [ka], [kb],
                    lambda: list(ksim.keypoint_features(cloud["points"], px, views[0], cloud["colors"], cloud["count"],
                                                        width=kw, height=kh, return_targets=True))))
    torch.cuda.synchronize()
    return rows


def two_clouds(seed, n=NET_N):
    """Two batches of two clouds [2, n, 3] f32: a slab (the table) and a small
    box on it, as tests/test_gpu_net.py's second cloud, shifted and scaled."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        xyz = rng.uniform(-1, 1, (2, n, 3)) * [0.35, 0.35, 0.05]
        box = rng.random((2, n)) < 0.4
        xyz[box] = rng.uniform(-1, 1, (int(box.sum()), 3)) * 0.07 + [0.05, -0.1, 0.1]
        out.append(dev(xyz.astype(np.float32) * np.float32(0.4) + np.array([0.1, -0.2, 0.5], np.float32)))
    return out


def cloud_rows():
    from net_helpers import NUM_CLASSES, STATE_SEED, seeded_state
    from pandasim import CloudSegNet
    from pandasim import _lib as L

    sim = make_sims((2,))[2]
    rng = np.random.default_rng(21)
    N, S, K = NET_N, 128, 16
    rows = []

    def add(name, bufs, A, B, call, **kw):
        rows.append(Row(name, "cloud", bufs, A, B, call, **kw))

    def raw(name, *args):
        sim._call(name, sim._ctx, *args, sim._stream())

    pa, pb = two_clouds(31)
    pts = torch.empty_like(pa)
    E = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=DEV)

    def normalize():
        out = [E(2, N, 3), E(2, 3), E(2)]
        raw("ps_cloud_normalize", _ptr(pts), N, *(_ptr(t) for t in out))
        return out

    add("ps_cloud_normalize", [pts], [pa], [pb], normalize)
    start = dev(rng.integers(0, N, 2).astype(np.int32))

    def fps():
        idx = E(2, S, dtype=torch.int32)
        raw("ps_cloud_fps", _ptr(pts), N, _ptr(start), S, _ptr(idx))
        return [idx]

    add("ps_cloud_fps", [pts], [pa], [pb], fps)
    centre = dev(np.stack([rng.permutation(N)[:S] for _ in range(2)]).astype(np.int32))

    def ball_query(radius=0.05):
        gidx = E(2, S, K, dtype=torch.int32)
        raw("ps_cloud_ball_query", _ptr(pts), N, _ptr(centre), S, float(radius), K, _ptr(gidx))
        return [gidx]

    add("ps_cloud_ball_query", [pts], [pa], [pb], ball_query)
    pts.copy_(pa)
    gidx = ball_query()[0]
    feats = dev(rng.normal(size=(2, N, 3)).astype(np.float32))
    add("ps_cloud_group", [pts], [pa], [pb], lambda: list(raw_group(sim, pts, feats, centre, gidx, new_xyz=True)))

    radii, nsamples = (0.03, 0.08), (8, 16)

    def set_abstraction():
        out = [E(2, N, 3), E(2, 3), E(2), E(2, S, dtype=torch.int32), E(2, S, 3)]
        gi = [E(2, S, k, dtype=torch.int32) for k in nsamples]
        gr = [E(2, S, k, 6) for k in nsamples]
        scales = (L.CloudScale * len(radii))()
        for sc, r, k, i, g in zip(scales, radii, nsamples, gi, gr):
            sc.radius, sc.nsample, sc.group_idx, sc.grouped = r, k, i.data_ptr(), g.data_ptr()
        sim._call("ps_cloud_set_abstraction", sim._ctx, _ptr(pts), _ptr(feats), N, 3, _ptr(start), S, scales, len(radii),
                  1, *(_ptr(t) for t in out), sim._stream())
        return out + gi + gr

    add("ps_cloud_set_abstraction", [pts], [pa], [pb], set_abstraction)

    coarse = pa[:, :S].contiguous()

    def three_nn():
        idx, w = E(2, N, 3, dtype=torch.int32), E(2, N, 3)
        raw("ps_cloud_three_nn", _ptr(pts), N, _ptr(coarse), S, _ptr(idx), _ptr(w))
        return [idx, w]

    add("ps_cloud_three_nn", [pts], [pa], [pb], three_nn)
    pts.copy_(pa)
    nn_idx, nn_w = three_nn()
    D1, D2 = 5, 19
    p1 = dev(rng.normal(size=(2, N, D1)).astype(np.float32))
    p2a, p2b = (dev(rng.normal(size=(2, S, D2)).astype(np.float32)) for _ in range(2))
    p2 = torch.empty_like(p2a)

    def interpolate():
        out = E(2, N, D1 + D2)
        raw("ps_cloud_interpolate", _ptr(p1), D1, _ptr(p2), D2, N, S, _ptr(nn_idx), _ptr(nn_w), _ptr(out))
        return [out]

    add("ps_cloud_interpolate", [p2], [p2a], [p2b], interpolate)
    add("ps_cloud_feature_propagation", [pts], [pa], [pb],
        lambda: list(sim.propagate_features(pts, coarse, p2a, p1, return_nn=True)))

    # "k515-hidden96" of SHAPES in tests/test_gpu_mlp.py and tests/test_gpu_bfloat.py: G = 31, 515 input channels
    R, C0, widths = 31, 515, [96, 33]
    layers = net(11 + R + C0, C0, widths)
    xa, xb = (dev(rng.normal(size=(2, R, C0)).astype(np.float32)) for _ in range(2))
    x = torch.empty_like(xa)
    # the gathered twin: D + 3 = 515 channels, groups of 5
    gxyz, gfa, gcentre, ggidx = (dev(t) for t in random_groups(41, 2, 100, 33, 5, C0 - 3))
    gfb = dev(rng.normal(size=tuple(gfa.shape)).astype(np.float32))
    gf = torch.empty_like(gfa)
    for precision, tag in (("float32", ""), ("bfloat16", "_bfloat")):
        mlp = upload(layers, precision)
        add(f"ps_cloud_mlp{tag}", [x], [xa], [xb], (lambda mlp: lambda: [sim.shared_mlp(x, mlp, pool=R)])(mlp))
        add(f"ps_cloud_group_mlp{tag}", [gf], [gfa], [gfb],
            (lambda mlp: lambda: [sim.abstract_features(gxyz, gf, gcentre, [ggidx], mlps=[mlp], fused=True)])(mlp))

    ld = NUM_CLASSES + 14
    ha, hb = (dev(rng.normal(size=(2, N, ld)).astype(np.float32)) for _ in range(2))
    head = torch.empty_like(ha)
    nxyz = dev(rng.uniform(-1, 1, (2, N, 3)).astype(np.float32))
    cen, sca = dev(rng.normal(size=(2, 3)).astype(np.float32)), dev(rng.uniform(0.5, 2, 2).astype(np.float32))

    def decode():
        d = sim.decode_waypoints(head, nxyz, NUM_CLASSES, cen, sca, return_labels=True)
        return [d.waypoints, d.quats, d.euler_deg, d.counts, d.first_idx, d.labels]

    add("ps_cloud_decode_waypoints", [head], [ha], [hb], decode)

    ca, cb = (dev(rng.random((2, N, 3)).astype(np.float32)) for _ in range(2))
    cols = torch.empty_like(ca)
    why = "group_cloud uploads the start indices: a blocking copy on the current stream"
    for precision in ("float32", "bfloat16"):
        segnet = CloudSegNet(seeded_state(STATE_SEED), DEV, precision=precision)

        def segment(segnet=segnet):
            h, g1 = sim.segment_cloud(segnet, pts, cols, 3)
            return [h, g1.xyz, g1.centroid, g1.scale, g1.fps_idx, g1.new_xyz]

        def predict(segnet=segnet):
            d = sim.predict_waypoints(segnet, pts, cols, 3)
            return [d.waypoints, d.quats, d.euler_deg, d.counts, d.first_idx]

        add(f"segment_cloud[{precision}]", [pts, cols], [pa, ca], [pb, cb], segment, blocks=why)
        add(f"predict_waypoints[{precision}]", [pts, cols], [pa, ca], [pb, cb], predict, blocks=why)
    torch.cuda.synchronize()
    return rows


FAMILIES = {"env": env_rows, "queries": query_rows, "motion": motion_rows, "camera": camera_rows, "cloud": cloud_rows}
ROW_NAMES = (
    "ps_step[push-1]", "ps_init_state", "ps_reset", "ps_step[push-16]", "ps_step[pick_and_place-8]", "ps_step[stack-1]",
    "ps_step_oriented[push-1]", "ps_sim_step[PandaPush-v3]", "ps_sim_step[PandaStack-v3]",
    "ps_link_state", "ps_inverse_kinematics", "ps_base_state", "ps_rng_seed+uniform+rotation", "ps_compute_reward",
    "ps_euler_xyz_to_quat", "ps_quat_to_euler_xyz",
    "ps_plan_move[reach]", "ps_plan_grasp[reach]", "ps_plan_release[reach]", "ps_motion_run[reach]",
    "ps_plan_move[pick_and_place]", "ps_plan_grasp[pick_and_place]", "ps_plan_release[pick_and_place]",
    "ps_motion_run[pick_and_place]",
    "ps_render", "render (ps_render + ps_deproject_image)", "ps_deproject_image", "ps_deproject_pixels",
    "ps_point_cloud[uncropped]", "ps_point_cloud[cropped]", "ps_cloud_keypoint_features",
    "ps_cloud_normalize", "ps_cloud_fps", "ps_cloud_ball_query", "ps_cloud_group", "ps_cloud_set_abstraction",
    "ps_cloud_three_nn", "ps_cloud_interpolate", "ps_cloud_feature_propagation",
    "ps_cloud_mlp", "ps_cloud_group_mlp", "ps_cloud_mlp_bfloat", "ps_cloud_group_mlp_bfloat",
    "ps_cloud_decode_waypoints", "segment_cloud[float32]", "predict_waypoints[float32]", "segment_cloud[bfloat16]",
    "predict_waypoints[bfloat16]",
)
# the row each family's control runs: one whose call does not block the host
CONTROLS = {"env": "ps_step[push-1]", "queries": "ps_link_state", "motion": "ps_motion_run[pick_and_place]",
            "camera": "ps_point_cloud[cropped]", "cloud": "ps_cloud_set_abstraction"}


# ----------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def table():
    """Every row, with ref_A, ref_B and its default-stream time: computed once."""
    rows = {}
    for family, build in FAMILIES.items():
        for row in build():
            assert row.family == family and row.name not in rows, row.name
            rows[row.name] = row.prepare()
    assert tuple(rows) == ROW_NAMES, sorted(set(rows) ^ set(ROW_NAMES))
    return rows


@pytest.fixture(scope="module")
def streams():
    """The module's two side streams: no more than these are ever live."""
    return torch.cuda.Stream(), torch.cuda.Stream()


def _mm_chain(n):
    a = torch.ones(2048, 2048, device=DEV)
    out = torch.empty_like(a)

    def delay():
        for _ in range(n):
            torch.mm(a, a, out=out)

    return delay


def make_delay(amount):
    """(the delay as a callable enqueuing it on the current stream, its facility)."""
    if hasattr(torch.cuda, "_sleep"):
        return (lambda: torch.cuda._sleep(amount)), "torch.cuda._sleep"
    return _mm_chain(max(1, amount >> 16)), "torch.mm chain"


def time_on(s, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        fn()
        e1.record()
    s.synchronize()
    return e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def delay(table, streams):
    """The calibrated delay: at least DELAY_FACTOR times the slowest row's
    default-stream call, measured with events on the side stream."""
    from types import SimpleNamespace

    s = streams[0]
    slowest = max(table.values(), key=lambda r: r.ms)
    amount = FIRST_CYCLES
    for doubling in range(MAX_DOUBLINGS + 1):
        fn, facility = make_delay(amount)
        time_on(s, fn)  # once unmeasured: the first launch, the clock ramp
        ms = time_on(s, fn)
        if ms >= DELAY_FACTOR * slowest.ms:
            break
        amount *= 2
    print(f"\n[streams] delay {ms:.2f} ms ({facility}, argument {amount}, {doubling} doublings); slowest row "
          f"{slowest.name} {slowest.ms:.3f} ms; ratio {ms / slowest.ms:.1f}; {len(table)} rows, "
          f"budget {len(table) + len(CONTROLS) + 3} delays = {(len(table) + len(CONTROLS) + 3) * ms / 1e3:.1f} s")
    assert ms >= DELAY_FACTOR * slowest.ms, (
        f"the delay reached {ms:.2f} ms after {MAX_DOUBLINGS} doublings; {DELAY_FACTOR} x the slowest row "
        f"({slowest.name}, {slowest.ms:.3f} ms) is {DELAY_FACTOR * slowest.ms:.2f} ms")
    return SimpleNamespace(fn=fn, ms=ms, slowest=slowest, facility=facility)


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ROW_NAMES)
def test_a_call_on_a_side_stream_is_ordered_behind_it(table, streams, delay, name):
    row = table[name]
    assert not all_same(row.ref_A, row.ref_B), f"{name}: ref_A and ref_B are the same bits, the row cannot fail"
    got, host_ms = behind_delay(row, delay.fn, streams[0])
    print(f"\n[streams] {name}: call {row.ms:.3f} ms, enqueued in {host_ms:.2f} ms of host time"
          f"{' (blocks: ' + row.blocks + ')' if row.blocks else ''}")
    bad = [k for k, (g, w) in enumerate(zip(got, row.ref_B)) if not same_bits(_bitwise(g), _bitwise(w))]
    was_a = [k for k in bad if same_bits(_bitwise(got[k]), _bitwise(row.ref_A[k]))]
    assert not bad, f"{name}: outputs {bad} differ from the default stream's; {was_a} of them are ref_A's bits"
    if row.blocks is None:
        assert host_ms < 0.5 * delay.ms, (f"{name}: the enqueue took {host_ms:.1f} ms of host time against a delay of "
                                          f"{delay.ms:.1f} ms: the call waited for the stream, the row has no power")


@pytest.mark.parametrize("family", tuple(FAMILIES))
def test_control_a_call_under_another_stream_is_caught(table, streams, delay, family):
    """The misordering the rows exist to catch, made from outside: the call goes
    to t while the delay and copy_(B) stay on s."""
    row = table[CONTROLS[family]]
    assert row.family == family and row.blocks is None
    assert not all_same(row.ref_A, row.ref_B)
    got, _ = behind_delay(row, delay.fn, *streams)
    assert not all_same(got, row.ref_B), f"{row.name}: a call on another stream gave ref_B: the protocol has no power"


def test_first_render_of_a_context_on_a_side_stream(streams, delay):
    """render_prims is allocated by the first ray-casting call and filled on
    that call's stream: the first render() of a context that only ever saw s
    equals an identically seeded context's on the default stream."""
    import pandasim

    view = pandasim.GRASP_VIEWS[0]
    keys = ("depth", "colors", "points", "valid", "pixels_2d")
    twin = fused_env("push", CAM_B)
    twin.reset(seed=5)
    want = [twin.sim.render(CAM_W, CAM_H, **view)[k] for k in keys] + [twin.sim.state]
    torch.cuda.synchronize()
    s = streams[0]
    with torch.cuda.stream(s):
        env = fused_env("push", CAM_B)
        env.reset(seed=5)
    s.synchronize()
    with torch.cuda.stream(s):
        delay.fn()
        out = env.sim.render(CAM_W, CAM_H, **view)
        got = clones([out[k] for k in keys] + [env.sim.state])
    s.synchronize()
    assert all_same(got, want)


def test_first_steps_of_a_stack_context_on_a_side_stream(streams, delay):
    """Stack's stash is allocated and cleared by the first step, on that step's
    stream (its unused pair and gripper slots read the zero block behind it):
    the first five steps of a context that only ever saw s equal an
    identically seeded context's on the default stream, obs and state."""
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    acts = [torch.rand(B_ENV, 4, device=DEV, generator=g) * 2 - 1 for _ in range(5)]
    twin = fused_env("stack")
    assert twin.action_dim == 4
    twin.reset(seed=6)
    want = []
    for a in acts:
        obs = twin.step(a)[0]
        want += [obs["observation"], obs["achieved_goal"], twin.sim.state.clone()]
    torch.cuda.synchronize()
    s = streams[0]
    with torch.cuda.stream(s):
        env = fused_env("stack")
        env.reset(seed=6)
    s.synchronize()
    got = []
    with torch.cuda.stream(s):
        delay.fn()
        for a in acts:
            obs = env.step(a)[0]
            got += [obs["observation"], obs["achieved_goal"], env.sim.state.clone()]
    s.synchronize()
    assert all_same(got, want)


def test_two_contexts_on_two_streams_share_nothing(streams):
    """A push context on s1 and a stack context on s2, five steps each
    interleaved from the host without synchronisation, then point_cloud of the
    first and render of the second: each equals the same sequence run alone on
    the default stream.  Contexts share no device scratch."""
    import pandasim

    views = list(pandasim.GRASP_VIEWS[:3])
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    acts = {task: [torch.rand(B_ENV, n_act, device=DEV, generator=g) * 2 - 1 for _ in range(5)]
            for task, n_act in (("push", 3), ("stack", 4))}  # Push's gripper is blocked: no finger action

    def finish(task, env, obs):
        out = [obs["observation"], obs["achieved_goal"], env.sim.state.clone()]
        if task == "push":
            return out + list(env.sim.point_cloud(views, CAM_K, CAM_W, CAM_H, 2024, CROP_BOX).values())
        image = env.sim.render(CAM_W, CAM_H, **views[0])
        return out + [image[k] for k in ("depth", "colors", "points", "valid")]

    want = {}
    for task in acts:
        env = fused_env(task)
        env.reset(seed=8)
        for a in acts[task]:
            obs = env.step(a)[0]
        want[task] = clones(finish(task, env, obs))
    torch.cuda.synchronize()

    on = dict(zip(acts, streams))
    envs = {}
    for task, s in on.items():
        with torch.cuda.stream(s):
            envs[task] = fused_env(task)
            envs[task].reset(seed=8)
    for s in streams:
        s.synchronize()
    obs = {}
    for k in range(5):
        for task, s in on.items():
            with torch.cuda.stream(s):
                obs[task] = envs[task].step(acts[task][k])[0]
    got = {}
    for task, s in on.items():
        with torch.cuda.stream(s):
            got[task] = clones(finish(task, envs[task], obs[task]))
    for s in streams:
        s.synchronize()
    for task in acts:
        assert all_same(got[task], want[task]), task
