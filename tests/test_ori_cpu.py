"""CPU tests of the oriented env step (Panda.set_action(action, euler_xyz),
panda_ori.py:52-99): the fp64 yardstick the GPU tests of
tests/test_gpu_oriented.py hold ps_step_oriented to, and the host logic of
PandaVecEnv.step's euler_xyz / orientation arguments.

The oracle has no oriented step of its own; `oracle_oriented_step` composes
one from its engine-level entry points (link_state, inverse_kinematics with any
target orientation, control_joints, sim_step, get_obs, is_success,
compute_reward) in the order po_step runs them.  With the standard orientation
it must reproduce oracle.step bit for bit, which is what makes it a yardstick.
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as R

import oracle as O
from parity_judge import FREE_GRIPPER, TOL, _obs_err, _within, groups_for, not_tight_cap

TASK_NAMES = ["reach", "push", "pick_and_place", "slide", "stack", "flip"]
JOINTS = [0, 1, 2, 3, 4, 5, 6, 9, 10]
FORCES = [87.0, 87.0, 87.0, 87.0, 12.0, 120.0, 120.0, 170.0, 170.0]  # panda.py:41
EE_LINK = 11
STANDARD_ORN = (1.0, 0.0, 0.0, 0.0)  # panda.py:89

# The orientation schedule of the teacher-forced GPU test: target Euler angles
# (-180, 0, 0) -- the standard orientation -- plus U(-DELTA, DELTA) degrees per
# axis, redrawn per env and step.
DELTA_DEG = 15.0
SCHEDULE_B, SCHEDULE_STEPS, SCHEDULE_SEED, SCHEDULE_RNG = 64, 10, 12345, 7


def oracle_oriented_step(cfg, env, action, orn):
    """One RobotTaskEnv.step(action, euler_xyz) + TimeLimit of the fp64 oracle
    on `env` (in place), the IK target's orientation being the quaternion
    `orn` (x, y, z, w): po_step (oracle/panda_oracle.c) restated with
    Panda.set_action of panda_ori.py:52-99.  Returns oracle.step's tuple."""
    na = O.action_dim(cfg)
    a = np.asarray(action, np.float32)[:na]
    a = np.where(a < np.float32(-1.0), np.float32(-1.0), np.where(a > np.float32(1.0), np.float32(1.0), a))
    if cfg.control == 0:
        p = O.link_state(cfg, env, EE_LINK)[0]
        tp = p + (a[:3] * np.float32(0.05)).astype(np.float64)  # the product in fp32, as the reference's float32 action
        if tp[2] < 0.0:
            tp[2] = 0.0
        target = list(O.inverse_kinematics(cfg, np.array(env.q), EE_LINK, tp, orn)[:7])
    else:  # joints control ignores the orientation (panda_ori.py:58-60)
        target = [env.q[d] + float(a[d] * np.float32(0.05)) for d in range(7)]
    width = 0.0
    if not cfg.block_gripper:
        width = (env.q[7] + env.q[8]) + float(a[na - 1] * np.float32(0.2))
    target += [width / 2.0, width / 2.0]
    O.control_joints(env, JOINTS, target, FORCES)
    O.sim_step(cfg, env)
    obs, ag, dg = O.get_obs(cfg, env)
    task = TASK_NAMES[cfg.task]
    goal = np.array(env.goal)
    te = O.is_success(ag, goal, task)
    r = O.compute_reward("sparse" if cfg.reward == 0 else "dense", ag, goal, task)
    env.elapsed += 1
    tr = env.elapsed >= O.max_episode_steps(cfg)
    return obs, ag, dg, float(r), bool(te), bool(tr)


def copy_env(env):
    return O.Env.from_buffer_copy(env)


def schedule(action_dim, delta=DELTA_DEG, B=SCHEDULE_B, steps=SCHEDULE_STEPS, seed=SCHEDULE_RNG):
    """[(actions [B, A] f32, euler_xyz [B, 3] f32 degrees)] per step: actions
    U(-1, 1), angles (-180, 0, 0) + U(-delta, delta) per axis."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        a = rng.uniform(-1, 1, size=(B, action_dim)).astype(np.float32)
        e = (np.array([-180.0, 0.0, 0.0]) + rng.uniform(-delta, delta, size=(B, 3))).astype(np.float32)
        out.append((a, e))
    return out


def quat_of(euler_deg):
    """The reference's quaternion of target angles (panda_ori.py:91), fp64."""
    return R.from_euler("xyz", np.asarray(euler_deg, np.float64), degrees=True).as_quat()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("task", TASK_NAMES)
def test_composed_step_reproduces_oracle_step(task):
    """Standard orientation: the composed step is oracle.step bit for bit --
    observation, goals, reward, flags and the env's joints and objects -- over
    8 envs x 5 seeded steps of every task at ee control."""
    cfg = O.config(task, control="ee")
    rng = np.random.default_rng(11)
    for i in range(8):
        a_env, b_env = O.new_env(cfg), O.new_env(cfg)
        O.reset(cfg, a_env, seed=500 + i)
        O.reset(cfg, b_env, seed=500 + i)
        for s in range(5):
            act = rng.uniform(-1.2, 1.2, size=O.action_dim(cfg)).astype(np.float32)  # some beyond the clip
            ref = O.step(cfg, a_env, act)
            got = oracle_oriented_step(cfg, b_env, act, STANDARD_ORN)
            for x, y in zip(ref[:3], got[:3]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (i, s)
            assert np.float32(ref[3]).view(np.uint32) == np.float32(got[3]).view(np.uint32)
            assert ref[4:] == got[4:]
            assert _same_bits(a_env.q, b_env.q) and _same_bits(a_env.qd, b_env.qd), (i, s)
            assert _same_bits(a_env.m_target, b_env.m_target) and _same_bits(a_env.m_maximp, b_env.m_maximp)
            assert a_env.elapsed == b_env.elapsed
            for k in range(cfg.n_objects):
                for f in ("pos", "quat", "vel", "omg"):
                    assert _same_bits(getattr(a_env.obj[k], f), getattr(b_env.obj[k], f)), (i, s, k, f)


def test_composed_step_follows_the_orientation():
    """A yawed target turns the oracle's end effector towards it."""
    cfg = O.config("reach", control="ee")
    env = O.new_env(cfg)
    O.reset(cfg, env, seed=3)
    q_t = quat_of([-180.0, 0.0, 45.0])

    def angle():
        q = O.link_state(cfg, env, EE_LINK)[1]
        return (R.from_quat(q_t) * R.from_quat(q).inv()).magnitude()

    first = angle()
    for _ in range(25):
        oracle_oriented_step(cfg, env, np.zeros(3, np.float32), q_t)
    assert first > 0.7 and angle() < 0.5 * first


@pytest.mark.parametrize("task", TASK_NAMES)
def test_schedule_is_resolved_by_the_oracle_at_fp32_resolution(task):
    """The teacher-forced GPU test's inputs, judged with the reference alone:
    along the schedule (DELTA_DEG = 15 degrees, B = 64, 10 steps, the GPU
    test's seeds; the states are the oracle's own free run from the same
    resets) each composed step is repeated with one fp32 ulp of noise on the
    state per substep (oracle.set_state_noise), the fp32 resolution of the
    state.  The share of samples whose observation then leaves
    parity_judge.TOL must stay within not_tight_cap(task): the orientation
    range does not put the step where fp32 cannot resolve it.  Range used:
    +-15 degrees per axis about (-180, 0, 0), not narrowed."""
    cfg = O.config(task, control="ee")
    groups = groups_for(task, 7 if task in FREE_GRIPPER else 6)
    envs = []
    for i in range(SCHEDULE_B):
        e = O.new_env(cfg)
        O.reset(cfg, e, seed=SCHEDULE_SEED + i)
        envs.append(e)
    outside = total = 0
    try:
        for a, eul in schedule(O.action_dim(cfg)):
            q = quat_of(eul)
            for i, e in enumerate(envs):
                before = {}
                for b in range(cfg.n_objects):
                    p = "obj_" if b == 0 else "obj2_"
                    before[p + "vel"] = float(np.abs(np.array(e.obj[b].vel)).max())
                    before[p + "avel"] = float(np.abs(np.array(e.obj[b].omg)).max())
                noisy = copy_env(e)
                O.set_state_noise(1.0, 1 + i)
                o_n = oracle_oriented_step(cfg, noisy, a[i], q[i])[0]
                O.set_state_noise(0.0)
                o = oracle_oriented_step(cfg, e, a[i], q[i])[0]
                bad = [k for k, idx in groups.items()
                       if not _within(_obs_err(o_n, o, k, idx, task), o, groups, k, TOL[task], before)]
                outside += bool(bad)
                total += 1
    finally:
        O.set_state_noise(0.0)
    print(task, f"outside TOL under 1 ulp of state noise: {outside} of {total}")
    assert total == SCHEDULE_B * SCHEDULE_STEPS
    assert outside <= not_tight_cap(task) * total


# ------------------------------------------------------------- host logic
class _Sim:
    """Stand-in for PandaSim: records the C-ABI calls, converts no angles."""

    def __init__(self):
        self.calls, self.state, self._ctx = [], None, None

    def _call(self, name, *args):
        self.calls.append(name)

    def _stream(self):
        return None

    def euler_xyz_to_quat(self, e):
        self.calls.append("euler_xyz_to_quat")
        return torch.zeros(e.shape[0], 4)


def _host_env(control="ee", B=4):
    from pandasim.envs import PandaVecEnv

    env = object.__new__(PandaVecEnv)
    env.sim, env.num_envs, env.device, env.control_type = _Sim(), B, torch.device("cpu"), control
    env.action_dim, env.autoreset, env._has_reset, env._nonfinite = 3, False, True, None
    for name, shape in (("_obs", (B, 6)), ("_ag", (B, 3)), ("_dg", (B, 3)), ("_final_obs", (B, 6)),
                        ("_final_ag", (B, 3)), ("_reward", (B,))):
        setattr(env, name, torch.zeros(shape))
    env._term = torch.zeros(B, dtype=torch.uint8)
    env._trunc = torch.zeros(B, dtype=torch.uint8)
    return env


def test_step_rejects_both_orientation_arguments():
    env = _host_env()
    with pytest.raises(ValueError, match="not both"):
        env.step(torch.zeros(4, 3), euler_xyz=[-180.0, 0.0, 0.0], orientation=[1.0, 0.0, 0.0, 0.0])
    assert env.sim.calls == []


@pytest.mark.parametrize("kw,value", [("euler_xyz", np.zeros(4)), ("euler_xyz", np.zeros((3, 3))),
                                      ("euler_xyz", np.zeros((4, 4))), ("euler_xyz", np.zeros((1, 3))),
                                      ("orientation", np.zeros(3)), ("orientation", np.zeros((4, 3))),
                                      ("orientation", np.zeros((5, 4))), ("orientation", np.zeros((4, 4, 1)))])
def test_step_rejects_wrong_orientation_shapes(kw, value):
    for control in ("ee", "joints"):  # a wrong shape is an error even where the value is ignored
        env = _host_env(control)
        with pytest.raises(ValueError, match=kw):
            env.step(torch.zeros(4, 3), **{kw: value})
        assert env.sim.calls == []


def test_step_picks_the_entry_point():
    """Neither argument: ps_step, as before.  One of them at ee control:
    ps_step_oriented (angles converted first).  Joints control ignores both
    (panda_ori.py:58-60): ps_step."""
    env = _host_env()
    env.step(torch.zeros(4, 3))
    assert env.sim.calls == ["ps_step"]
    for kw, value, calls in (("euler_xyz", [-180.0, 0.0, 30.0], ["euler_xyz_to_quat", "ps_step_oriented"]),
                             ("euler_xyz", np.zeros((4, 3)), ["euler_xyz_to_quat", "ps_step_oriented"]),
                             ("orientation", [1.0, 0.0, 0.0, 0.0], ["ps_step_oriented"]),
                             ("orientation", np.ones((4, 4)), ["ps_step_oriented"])):
        env = _host_env()
        env.step(torch.zeros(4, 3), **{kw: value})
        assert env.sim.calls == calls, kw
        env = _host_env("joints")
        env.step(torch.zeros(4, 3), **{kw: value})
        assert env.sim.calls == ["ps_step"], kw


def test_plugin_robot_passes_the_orientation_on():
    """robots.Panda.set_action(action, euler_xyz) hands IK the converted
    quaternion, and the standard one without it; RobotTaskEnv.step and
    TimeLimit.step pass euler_xyz through."""
    from pandasim.core import RobotTaskEnv, TimeLimit
    from pandasim.robots import Panda

    seen = {}

    class S:
        device = torch.device("cpu")

        def euler_xyz_to_quat(self, e):
            seen["euler"] = e
            return torch.full((2, 4), 0.5)

        def get_link_position(self, body, link):
            return torch.zeros(2, 3)

        def get_joint_angle(self, body, joint):
            return torch.zeros(2)

        def inverse_kinematics(self, body, link, position, orientation):
            seen["orn"] = orientation
            return torch.zeros(2, 9)

        def control_joints(self, **kw):
            seen["targets"] = kw["target_angles"]

    robot = object.__new__(Panda)
    robot.sim, robot.body_name, robot.control_type, robot.block_gripper, robot.ee_link = S(), "panda", "ee", True, 11
    robot.joint_indices, robot.joint_forces = np.array(JOINTS), np.array(FORCES)
    robot.set_action(torch.zeros(2, 3))
    assert np.array_equal(np.asarray(seen["orn"]), STANDARD_ORN) and "euler" not in seen
    robot.set_action(torch.zeros(2, 3), [-180.0, 0.0, 45.0])
    assert seen["euler"] == [-180.0, 0.0, 45.0] and torch.equal(seen["orn"], torch.full((2, 4), 0.5))

    class Robot:
        def set_action(self, action, euler_xyz="absent"):
            seen["step"] = euler_xyz

    class Sim:
        def step(self):
            pass

    class Task:
        def get_goal(self):
            return torch.zeros(2, 3)

        def is_success(self, ag, dg):
            return torch.zeros(2, dtype=torch.bool)

        def compute_reward(self, ag, dg, info):
            return torch.zeros(2)

    env = object.__new__(RobotTaskEnv)
    env.sim, env.robot, env.task, env.num_envs, env.device = Sim(), Robot(), Task(), 2, torch.device("cpu")
    env._get_obs = lambda: {"achieved_goal": torch.zeros(2, 3)}
    env.step(torch.zeros(2, 3))
    assert seen["step"] == "absent"
    TimeLimit(env, 5).step(torch.zeros(2, 3), euler_xyz=[1.0, 2.0, 3.0])
    assert seen["step"] == [1.0, 2.0, 3.0]
