"""CPU tests of the Cartesian motion primitives (panda_cartesian.py:53-145:
Cartesian set_action, move, grasp, release): the fp64 yardstick the GPU tests
of tests/test_gpu_motion.py hold ps_plan_* / ps_motion_run to, the new ABI
symbols, and the host logic of pandasim.panda_cartesian.Panda.

The oracle has no primitives; `oracle_plan_move`, `oracle_control_step` and
`oracle_run` compose them from its engine-level entry points (link_state,
inverse_kinematics, control_joints, sim_step) with scipy's Rotation / Slerp and
numpy fp64, following panda_cartesian.py line by line, the way
tests/test_ori_cpu.py::oracle_oriented_step composes the oriented step.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as R
from scipy.spatial.transform import Slerp

import oracle as O
from parity_judge import TOL, _obs_err, _within, groups_for
from test_ori_cpu import EE_LINK, FORCES, JOINTS, STANDARD_ORN, copy_env, oracle_oriented_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["reach", "pick_and_place", "slide", "stack"]  # the four compile units of k_motion
HOLD_STEPS = 30  # panda_cartesian.py:127, 142
# parity_judge.NOT_TOL_CAP by the plan's gripper, not the task's: 0.005 blocked, 0.08 free
CAP = {True: 0.005, False: 0.08}

# The teacher-forced schedule (shared with tests/test_gpu_motion.py): B envs
# reset with seed SEED + i; goals at MOVE_DISTANCES[i % 8] from the start in a
# random direction, goal angles (-180, 0, 0) + U(-15, 15) degrees per axis;
# then the first HOLD_TF_STEPS control steps of release and of grasp.
SCHED_B, SCHED_SEED, SCHED_RNG = 100, 4321, 9
MOVE_DISTANCES = (0.02, 0.0305, 0.0325, 0.045, 0.05, 0.065, 0.08, 0.10)  # 20, 2, 3, 3, 4, 5, 6, 7 control steps
MOVE_STEPS = (20, 2, 3, 3, 4, 5, 6, 7)
HOLD_TF_STEPS = 5
# release(width=1) presses both fingers into their upper limit within its first
# control step (width 0.08), the finger-limit bifurcation of parity_judge: from
# its third step on the oracle alone leaves TOL under one ulp of state noise (11
# to 20 of 40 envs at the third step, 37 to 39 from the fourth, in every scene:
# scripts/motion_release_probe.py, profiles/motion_release_probe.txt), far over
# the cap.  The schedule's release is narrowed to a width
# that keeps the fingers inside their range over the steps it covers (+ 8.8 mm
# per control step: 0.044 of 0.08 m after five); the cap stays.
RELEASE_TF_WIDTH = 0.01
DELTA_DEG = 15.0


# ------------------------------------------------------------ the yardstick
def oracle_set_action(cfg, env, action, orn, blocked):
    """Cartesian Panda.set_action(action[4], orientation) (panda_cartesian.py:53-72,
    147-176) on `env`: every component clipped to [-1, 1]; target = ee position
    + action[:3] (factor 1), z >= 0; IK on link 11 with quaternion `orn`;
    fingers 0 when blocked, else width + action[3] (factor 1), half each."""
    a = np.clip(np.asarray(action, np.float64), -1.0, 1.0)
    p = O.link_state(cfg, env, EE_LINK)[0]
    tp = p + a[:3]
    tp[2] = np.max((0, tp[2]))
    target = list(O.inverse_kinematics(cfg, np.array(env.q), EE_LINK, tp, orn)[:7])
    width = 0.0 if blocked else (env.q[7] + env.q[8]) + a[3]
    target += [width / 2, width / 2]
    O.control_joints(env, JOINTS, target, FORCES)


def num_steps_of(d):
    """move's step count for a distance d (panda_cartesian.py:74-85, 105-114)."""
    if d < 0.03:
        return 20
    n = d // 0.015
    if d % 0.015 > 1e-3:
        n += 1
    return int(n)


def ee_euler(cfg, env):
    """get_ee_orientation (panda_cartesian.py:222-225)."""
    return R.from_quat(O.link_state(cfg, env, EE_LINK)[1]).as_euler("xyz", degrees=True)


def oracle_plan_move(cfg, env, goal_pos, goal_euler):
    """Panda.move up to its loop (panda_cartesian.py:98-114)."""
    goal_pos = np.asarray(goal_pos, np.float64)
    start = O.link_state(cfg, env, EE_LINK)[0]
    start_euler = ee_euler(cfg, env)
    n = num_steps_of(np.linalg.norm(goal_pos - start))
    rots = R.from_euler("xyz", [start_euler.copy(), np.asarray(goal_euler, np.float64).copy()], degrees=True)
    return dict(kind="move", num=n, start=start, delta=(goal_pos - start) / n, width=env.q[7] + env.q[8],
                slerp=Slerp([1, n], rots), start_quat=rots[0].as_quat())


def oracle_plan_hold(width=1.0):
    """grasp (width 1, gripper blocked) / release(width) (panda_cartesian.py:124-145)."""
    return dict(kind="hold", num=HOLD_STEPS, width=float(width))


def oracle_control_step(cfg, env, plan, i, blocked):
    """Control step i (1-based) of a plan on `env`: the loop bodies of
    panda_cartesian.py:116-122 / 127-130 / 142-145."""
    if plan["kind"] == "move":
        next_pos = plan["start"] + plan["delta"] * min(i, plan["num"])
        next_euler = plan["slerp"](i).as_euler("xyz", degrees=True)
        action = (next_pos - O.link_state(cfg, env, EE_LINK)[0]).tolist() + [plan["width"]]
    else:
        next_euler = ee_euler(cfg, env)
        action = [0, 0, 0, plan["width"]]
    orn = R.from_euler("xyz", next_euler, degrees=True).as_quat()
    oracle_set_action(cfg, env, action, orn, blocked)
    O.sim_step(cfg, env)


def oracle_run(cfg, env, plan, blocked, first=1, last=None):
    for i in range(first, (plan["num"] if last is None else last) + 1):
        oracle_control_step(cfg, env, plan, i, blocked)


def obs_config(cfg):
    """`cfg` with a free gripper: O.get_obs then includes the finger width."""
    c = O.Config.from_buffer_copy(cfg)
    c.block_gripper = 0
    return c


def motion_obs(cfg, env):
    """The state as parity_judge's groups read it: ee position and velocity,
    width, then the objects' pose and velocity (groups_for(task, 7))."""
    return O.get_obs(obs_config(cfg), env)[0]


def move_goals(starts, seed=SCHED_RNG):
    """(goal_pos [B, 3], goal_euler [B, 3]) of the schedule, both rounded to
    fp32 (what the C ABI takes): env i's goal lies MOVE_DISTANCES[i % 8] from
    starts[i], and the rounding moves that distance by < 1e-7 m, so it stays
    >= 1e-4 m from the branch points 0.03 and 0.015 k + 0.001."""
    rng = np.random.default_rng(seed)
    B = len(starts)
    u = rng.normal(size=(B, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = np.array([MOVE_DISTANCES[i % len(MOVE_DISTANCES)] for i in range(B)])
    goal = (np.asarray(starts, np.float64) + u * d[:, None]).astype(np.float32).astype(np.float64)
    euler = (np.array([-180.0, 0.0, 0.0]) + rng.uniform(-DELTA_DEG, DELTA_DEG, size=(B, 3))).astype(np.float32)
    return goal, euler.astype(np.float64)


def scene_blocked(cfg):
    return bool(cfg.block_gripper)


# ------------------------------------------------------------------- the ABI
def test_new_symbols_resolve_and_version_matches_the_header():
    """The motion entry points are exported and bound.  PS_ABI_VERSION: the
    library reports the header's value (6: the entry points are added within
    it, as the oriented step's were; tests/test_abi_cpu.py pins 6)."""
    from pandasim import _lib as L

    lib = L.lib()
    for s in ("ps_motion_plan_bytes", "ps_plan_move", "ps_plan_grasp", "ps_plan_release", "ps_motion_run"):
        assert hasattr(lib, s) and s in L.exported_symbols(), s
    src = open(os.path.join(ROOT, "include", "pandasim.h")).read()
    assert lib.ps_abi_version() == int(re.search(r"#define PS_ABI_VERSION (\d+)", src).group(1))
    for name in ("PLAN_START", "PLAN_DELTA", "PLAN_WIDTH", "PLAN_Q0", "PLAN_ROTVEC", "PLAN_NUM_F64_ROWS",
                 "PLAN_NUM_STEPS", "PLAN_DONE", "PLAN_BLOCKED", "PLAN_KIND", "PLAN_NUM_I32_ROWS", "PLAN_KIND_MOVE",
                 "PLAN_KIND_HOLD"):
        assert int(re.search(rf"\bPS_{name} = (\d+)", src).group(1)) == getattr(L, name), name
    assert int(re.search(r"#define PS_PLAN_HOLD_STEPS (\d+)", src).group(1)) == L.PLAN_HOLD_STEPS == HOLD_STEPS


def test_plan_bytes_and_argument_errors():
    from pandasim import _lib as L

    lib = L.lib()
    for n in (1, 64, 100, 1000):
        stride = L.layout(n).stride
        assert lib.ps_motion_plan_bytes(n) == stride * (14 * 8 + 4 * 4)
    assert lib.ps_motion_plan_bytes(0) < 0 and lib.ps_motion_plan_bytes((1 << 28) + 1) < 0
    cfg = L.default_config(2, 1, 0)  # joints control: the primitives take any context
    ctx = C.c_void_p()
    assert lib.ps_create(C.byref(cfg), 8, 0, C.byref(ctx)) == 0
    x = C.c_void_p(64)  # never dereferenced: every call below fails its argument check first
    assert lib.ps_motion_run(ctx, None, x, 1, None) == -1
    assert lib.ps_motion_run(ctx, x, None, 1, None) == -1
    assert lib.ps_motion_run(ctx, x, x, 0, None) == -1
    assert lib.ps_motion_run(ctx, x, x, -3, None) == -1
    assert lib.ps_motion_run(None, x, x, 1, None) == -1
    assert lib.ps_plan_move(ctx, x, x, None, x, None, None) == -1
    assert lib.ps_plan_move(ctx, x, x, x, None, None, None) == -1
    assert lib.ps_plan_move(ctx, None, x, x, x, None, None) == -1
    assert lib.ps_plan_grasp(ctx, x, None, None, None) == -1
    assert lib.ps_plan_release(ctx, None, x, None, None, None) == -1
    lib.ps_destroy(ctx)


# ---------------------------------------------------------------- host logic
class _Plan:
    def __init__(self, steps):
        self.num_steps = torch.tensor(steps, dtype=torch.int32)
        self.blocked = torch.zeros(len(steps), dtype=torch.int32)


class _Sim:
    """Stand-in for PandaSim: records the calls, plans `steps` control steps."""

    device = torch.device("cpu")

    def __init__(self, steps):
        self.calls, self.steps = [], steps

    def motion_plan(self):
        self.calls.append(("motion_plan",))
        return _Plan(self.steps)

    def euler_xyz_to_quat(self, e):
        e = torch.as_tensor(e, dtype=torch.float32)
        self.calls.append(("euler_xyz_to_quat", tuple(e.shape)))
        return torch.zeros(*e.shape[:-1], 4)

    def plan_move(self, plan, pos, quat, mask):
        self.calls.append(("plan_move", tuple(torch.as_tensor(pos).shape), tuple(quat.shape), mask,
                           plan.blocked.tolist()))

    def plan_grasp(self, plan, mask):
        self.calls.append(("plan_grasp", mask))

    def plan_release(self, plan, width, mask):
        self.calls.append(("plan_release", width, mask))

    def motion_run(self, plan, n):
        self.calls.append(("motion_run", n))


def _host_robot(steps=(3, 7, 2), block_gripper=False):
    from pandasim.panda_cartesian import Panda

    robot = object.__new__(Panda)
    robot.sim, robot.block_gripper, robot._plan = _Sim(list(steps)), block_gripper, None
    return robot


def test_primitives_issue_plan_then_run():
    robot = _host_robot()
    assert robot.move([0.1, 0.0, 0.2], [-180.0, 0.0, 30.0]) == 7
    assert robot.sim.calls == [("motion_plan",), ("euler_xyz_to_quat", (3,)),
                               ("plan_move", (3,), (4,), None, [0, 0, 0]), ("motion_run", 7)]
    robot.sim.calls.clear()
    mask = [1, 0, 1]
    robot.move(np.zeros((3, 3)), np.zeros((3, 3)), mask=mask, chunk=3)  # [B, 3] goals, 3 + 3 + 1 control steps
    assert robot.sim.calls == [("euler_xyz_to_quat", (3, 3)), ("plan_move", (3, 3), (3, 4), mask, [0, 0, 0]),
                               ("motion_run", 3), ("motion_run", 3), ("motion_run", 1)]
    with pytest.raises(ValueError, match="chunk"):
        robot.move([0.0, 0.0, 0.1], [-180.0, 0.0, 0.0], chunk=0)


def test_grasp_and_release_toggle_block_gripper():
    robot = _host_robot(steps=(30, 30, 30))
    assert robot.block_gripper is False
    assert robot.grasp() == 30
    assert robot.block_gripper is True
    assert robot.sim.calls == [("motion_plan",), ("plan_grasp", None), ("motion_run", 30)]
    robot.sim.calls.clear()
    robot.move([0.0, 0.0, 0.1], [-180.0, 0.0, 0.0])  # a blocked gripper reaches the plan
    assert robot.sim.calls[1] == ("plan_move", (3,), (4,), None, [1, 1, 1])
    robot.sim.calls.clear()
    assert robot.release(width=0.5, mask=[0, 1, 1], chunk=20) == 30
    assert robot.block_gripper is False
    assert robot.sim.calls == [("plan_release", 0.5, [0, 1, 1]), ("motion_run", 20), ("motion_run", 10)]
    robot.sim.calls.clear()
    robot.release()
    assert robot.sim.calls[0] == ("plan_release", 1, None)


def test_cartesian_set_action_is_unscaled():
    """panda_cartesian.Panda.set_action: the displacement and the finger
    command reach IK and the motors as they are (panda_cartesian.py:67, 157)."""
    from pandasim.panda_cartesian import Panda

    seen = {}

    class S:
        device = torch.device("cpu")

        def euler_xyz_to_quat(self, e):
            seen["euler"] = e
            return torch.full((2, 4), 0.5)

        def get_link_position(self, body, link):
            return torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.0, 0.05]])

        def get_joint_angle(self, body, joint):
            return torch.full((2,), 0.01)

        def inverse_kinematics(self, body, link, position, orientation):
            seen["pos"], seen["orn"] = position, orientation
            return torch.zeros(2, 9)

        def control_joints(self, **kw):
            seen["targets"] = kw["target_angles"]

    robot = object.__new__(Panda)
    robot.sim, robot.body_name, robot.control_type, robot.block_gripper, robot.ee_link = S(), "panda", "ee", False, 11
    robot.joint_indices, robot.joint_forces, robot.fingers_indices = np.array(JOINTS), np.array(FORCES), np.array([9, 10])
    robot.set_action(torch.tensor([[0.5, -0.25, 2.0, 0.03], [0.0, 0.0, -0.5, -2.0]]))
    assert torch.allclose(seen["pos"], torch.tensor([[0.6, -0.05, 1.3], [0.0, 0.0, 0.0]]))  # clipped to 1; z >= 0
    assert list(seen["orn"]) == list(STANDARD_ORN) and "euler" not in seen
    assert torch.allclose(seen["targets"][:, 7:], torch.tensor([[0.025, 0.025], [-0.49, -0.49]]))
    robot.block_gripper = True
    robot.set_action(torch.zeros(2, 4), [-180.0, 0.0, 45.0])
    assert seen["euler"] == [-180.0, 0.0, 45.0] and torch.equal(seen["orn"], torch.full((2, 4), 0.5))
    assert torch.equal(seen["targets"][:, 7:], torch.zeros(2, 2))


def test_module_is_exported():
    import pandasim

    assert pandasim.panda_cartesian.Panda.__mro__[1] is pandasim.robots.Panda


# ------------------------------------------------ the composed oracle is sane
def test_num_steps_at_the_branch_points():
    assert [num_steps_of(d) for d in (0.02, 0.0305, 0.0315, 0.045)] == [20, 2, 3, 3]
    assert tuple(num_steps_of(d) for d in MOVE_DISTANCES) == MOVE_STEPS
    cfg = O.config("reach")
    env = O.new_env(cfg)
    O.reset(cfg, env, seed=1)
    start = O.link_state(cfg, env, EE_LINK)[0]
    for d, n in zip((0.02, 0.0305, 0.0315, 0.045), (20, 2, 3, 3)):
        plan = oracle_plan_move(cfg, env, start + np.array([0.0, d, 0.0]), [-180.0, 0.0, 0.0])
        assert plan["num"] == n and np.allclose(plan["delta"] * n, [0.0, d, 0.0], atol=1e-15)


def test_move_approaches_the_goal():
    cfg = O.config("reach")
    env = O.new_env(cfg)
    O.reset(cfg, env, seed=3)
    start = O.link_state(cfg, env, EE_LINK)[0]
    goal, goal_euler = start + np.array([0.03, -0.04, 0.02]), [-180.0, 0.0, 30.0]
    q_goal = R.from_euler("xyz", goal_euler, degrees=True)

    def angle():
        return (q_goal * R.from_quat(O.link_state(cfg, env, EE_LINK)[1]).inv()).magnitude()

    first = angle()
    plan = oracle_plan_move(cfg, env, goal, goal_euler)
    assert plan["num"] == 4
    oracle_run(cfg, env, plan, scene_blocked(cfg))
    end = O.link_state(cfg, env, EE_LINK)[0]
    assert np.linalg.norm(end - goal) < 0.5 * np.linalg.norm(start - goal)
    assert first > 0.5 and angle() < first


@pytest.mark.parametrize("task", ["push", "pick_and_place"])
def test_cartesian_step_reproduces_the_oriented_step(task):
    """A Cartesian step with action * 0.05, width * 0.2 and the standard
    orientation is oracle_oriented_step's robot state, bit for bit."""
    cfg = O.config(task, control="ee")
    rng = np.random.default_rng(5)
    a_env, b_env = O.new_env(cfg), O.new_env(cfg)
    O.reset(cfg, a_env, seed=77)
    O.reset(cfg, b_env, seed=77)
    for s in range(4):
        act = rng.uniform(-1, 1, size=O.action_dim(cfg)).astype(np.float32)
        oracle_oriented_step(cfg, a_env, act, STANDARD_ORN)
        a4 = list((act[:3] * np.float32(0.05)).astype(np.float64))
        a4.append(0.0 if cfg.block_gripper else float(act[3] * np.float32(0.2)))
        oracle_set_action(cfg, b_env, a4, STANDARD_ORN, scene_blocked(cfg))
        O.sim_step(cfg, b_env)
        for f in ("q", "qd", "m_target", "m_maximp"):
            x, y = np.array(getattr(a_env, f)), np.array(getattr(b_env, f))
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (s, f)


# ------------------------------------------------- the schedule, judged alone
def _outside(cfg, task, env, plan, i, blocked, seed):
    """One control step of `env` (in place), and whether its repeat under one
    ulp of state noise leaves parity_judge.TOL."""
    groups = groups_for(task, 7)
    before = {}
    for b in range(cfg.n_objects):
        p = "obj_" if b == 0 else "obj2_"
        before[p + "vel"] = float(np.abs(np.array(env.obj[b].vel)).max())
        before[p + "avel"] = float(np.abs(np.array(env.obj[b].omg)).max())
    noisy = copy_env(env)
    O.set_state_noise(1.0, seed)
    try:
        oracle_control_step(cfg, noisy, plan, i, blocked)
    finally:
        O.set_state_noise(0.0)
    oracle_control_step(cfg, env, plan, i, blocked)
    o_n, o = motion_obs(cfg, noisy), motion_obs(cfg, env)
    return any(not _within(_obs_err(o_n, o, k, idx, task), o, groups, k, TOL[task], before)
               for k, idx in groups.items())


@pytest.mark.parametrize("task", SCENES)
def test_schedule_is_resolved_by_the_oracle_at_fp32_resolution(task):
    """The teacher-forced GPU test's inputs, judged with the reference alone
    (as tests/test_ori_cpu.py does for the oriented step): along the move
    schedule, then the first HOLD_TF_STEPS control steps of release and of
    grasp -- the states are the oracle's own run from the same resets -- every
    control step is repeated with one fp32 ulp of state noise per substep.
    The share of samples leaving parity_judge.TOL must stay within the cap of
    the plan's gripper (0.005 blocked, 0.08 free).  Narrowed input: release's
    width (RELEASE_TF_WIDTH, see there); the move schedule and grasp are not."""
    cfg = O.config(task, control="ee")
    envs = []
    for i in range(SCHED_B):
        e = O.new_env(cfg)
        O.reset(cfg, e, seed=SCHED_SEED + i)
        envs.append(e)
    goal, euler = move_goals([O.link_state(cfg, e, EE_LINK)[0] for e in envs])
    counts = {}
    for phase, blocked in (("move", scene_blocked(cfg)), ("release", False), ("grasp", True)):
        outside = total = 0
        for i, e in enumerate(envs):
            if phase == "move":
                plan = oracle_plan_move(cfg, e, goal[i], euler[i])
                assert plan["num"] == MOVE_STEPS[i % len(MOVE_STEPS)]
                last = plan["num"]
            else:
                plan, last = oracle_plan_hold(RELEASE_TF_WIDTH if phase == "release" else 1.0), HOLD_TF_STEPS
            for s in range(1, last + 1):
                outside += _outside(cfg, task, e, plan, s, blocked, 1 + i)
                total += 1
        counts[phase] = (outside, total)
        print(task, phase, f"outside TOL under 1 ulp of state noise: {outside} of {total}")
    for phase, blocked in (("move", scene_blocked(cfg)), ("release", False), ("grasp", True)):
        outside, total = counts[phase]
        assert outside <= CAP[blocked] * total, (phase, outside, total)
