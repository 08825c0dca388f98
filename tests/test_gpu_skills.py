"""GPU tests of pandasim.skills (run_policy.py:189-193, 287-339 as motion
programs) in PandaPickAndPlace, B = 8: each skill against the written-out list
of Panda calls of the reference's lines, bit for bit; execute with per-env
actions against each env run alone; a DecodedWaypoints with an empty set.
The waits are shortened to 3 control steps through skills.WAIT_STEPS.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 8
WAIT = 3
NEUTRAL = np.array([0.00, 0.41, 0.00, -1.85, 0.00, 2.26, 0.79, 0.00, 0.00])  # panda.py:51


def make_robot(n=B, seed=11):
    from pandasim.envs import PandaVecEnv
    from pandasim.panda_cartesian import Panda

    env = PandaVecEnv("pick_and_place", "sparse", "ee", n, "cuda", autoreset=False)
    env.reset(seed=seed)
    robot = object.__new__(Panda)
    robot.sim, robot.block_gripper, robot._plan = env.sim, False, None
    robot.body_name, robot.joint_indices = "panda", np.array([0, 1, 2, 3, 4, 5, 6, 9, 10])
    robot.neutral_joint_values = NEUTRAL
    return robot


@pytest.fixture(scope="module")
def robot():
    return make_robot()


@pytest.fixture(autouse=True)
def short_waits(monkeypatch):
    from pandasim import skills

    monkeypatch.setattr(skills, "WAIT_STEPS", WAIT)


def waypoints(n=B):
    """(start_pos, end_pos, start_euler, end_euler), [n, 3] each, per env."""
    rng = np.random.default_rng(3)
    start = np.stack([rng.uniform(-0.10, 0.05, n), rng.uniform(-0.15, 0.15, n), rng.uniform(0.03, 0.12, n)], 1)
    end = start + np.stack([rng.uniform(0.03, 0.10, n), rng.uniform(-0.08, 0.08, n), rng.uniform(0.05, 0.15, n)], 1)
    start_e = np.array([180.0, 0.0, 0.0]) + rng.uniform(-10, 10, (n, 3))
    end_e = np.array([180.0, 0.0, 0.0]) + rng.uniform(-25, 25, (n, 3))
    return tuple(torch.from_numpy(a.astype(np.float32)).cuda() for a in (start, end, start_e, end_e))


def wait(robot):
    for _ in range(WAIT):
        robot.sim.step()


def reset_robot_calls(robot):
    robot.reset()                                   # :190
    robot.move(np.array([0, 0, 0.6]), np.array([180, 0, 0]))  # :191-192
    robot.release()                                 # :193


def pour_calls(robot, start_pos, end_pos, start_euler, end_euler):
    up = torch.tensor([0.0, 0.0, 0.10], device=start_pos.device)
    robot.move(start_pos + up, start_euler)  # :327
    robot.move(start_pos, start_euler)       # :328
    robot.grasp()                            # :329
    robot.move(start_pos + up, start_euler)  # :331
    robot.move(end_pos, start_euler)         # :333
    robot.move(end_pos, end_euler)           # :334
    wait(robot)                              # :337-338
    reset_robot_calls(robot)                 # :339


def open_calls(robot, grasp_pos, approach_pos, grasp_euler, approach_euler):
    reset_robot_calls(robot)                 # :292
    robot.move(approach_pos, grasp_euler)    # :293
    wait(robot)
    robot.move(grasp_pos, grasp_euler)       # :296
    wait(robot)
    robot.grasp()                            # :299
    delta = (approach_pos - grasp_pos) / 15  # :301-303
    for i in range(15):
        robot.move(grasp_pos + i * delta, grasp_euler)  # :306
    robot.release()                          # :308
    reset_robot_calls(robot)                 # :309


def close_calls(robot, approach_pos, grasp_pos, approach_euler, grasp_euler):
    delta = (approach_pos - grasp_pos) / 15  # :316-318
    for i in range(15):
        robot.move(approach_pos - i * delta, grasp_euler)  # :321
        if i == 3:
            robot.grasp()                    # :323


CALLS = dict(pour=pour_calls, open=open_calls, close=close_calls)


def restart(robot, state0):
    robot.sim.state.copy_(state0)
    robot._plan, robot.block_gripper = None, False


def final(robot):
    torch.cuda.synchronize()
    return robot.sim.state.clone()


@pytest.mark.parametrize("name", ["pour", "open", "close"])
def test_skill_equals_the_written_out_calls(robot, name):
    from pandasim import skills

    state0 = robot.sim.state.clone()
    w = waypoints()
    try:
        CALLS[name](robot, *w)
        want, flag = final(robot), robot.block_gripper
        restart(robot, state0)
        completed, steps = skills.SKILLS[name](robot, *w)
        got = final(robot)
        print(name, "control steps per env", steps.tolist(), "segments", int(completed[0]))
        assert (completed == {"pour": 7, "open": 23, "close": 16}[name]).all()
        assert robot.block_gripper is flag
        assert not torch.equal(want, state0) and torch.equal(got, want)
    finally:
        restart(robot, state0)


def env_columns(sim, state, j):
    lay, stride = sim.layout, sim.layout.stride
    f = state[lay.float_offset:lay.goal_offset].view(torch.int32).view(-1, stride)[:, j]
    return f.clone()


def test_execute_per_env_actions_equal_each_env_alone(robot):
    """execute(['pour', 'open', 'close', ...]) leaves every env the float rows
    of a batch of one holding that env's state and running its own action."""
    from pandasim import skills

    sim = robot.sim
    state0 = sim.state.clone()
    w = waypoints()
    actions = ["pour", "open", "close", "close", "pour", "open", "pour", "close"]
    try:
        out = skills.execute(robot, w, actions)
        got = final(robot)
        assert list(out) == ["pour", "open", "close"] and robot.block_gripper is True  # close, the last, ends on a grasp
        one = make_robot(1)
        for j, name in enumerate(actions):
            for rows in ("f", "goal", "rng"):
                getattr(one.sim, rows)[:, 0] = state_rows(sim, state0, rows)[:, j]
            one._plan, one.block_gripper = None, False
            skills.execute(one, tuple(a[j:j + 1].clone() for a in w), name)
            alone = final(one)
            assert torch.equal(env_columns(one.sim, alone, 0), env_columns(sim, got, j)), (j, name)
    finally:
        restart(robot, state0)


def state_rows(sim, state, name):
    lay, n = sim.layout, sim.layout.stride
    if name == "f":
        return state[lay.float_offset:lay.goal_offset].view(torch.float32).view(-1, n)
    if name == "goal":
        return state[lay.goal_offset:lay.rng_offset].view(torch.float64).view(-1, n)
    return state[lay.rng_offset:lay.elapsed_offset].view(torch.int64).view(-1, n)


def test_execute_stops_only_the_env_with_an_empty_set(robot):
    """A DecodedWaypoints whose start set is empty in env 2 (NaN waypoint and
    angles, as decode_waypoints reports it): pour's program stops that env at
    its first move (completed 0, no control step) and every other env runs
    all seven segments to the bits of the run without the gap."""
    from pandasim import DecodedWaypoints, skills

    sim = robot.sim
    state0 = sim.state.clone()
    w = waypoints()
    try:
        skills.execute(robot, w, "pour")
        want = final(robot)
        restart(robot, state0)
        d = DecodedWaypoints()
        d.waypoints, d.euler_deg = torch.stack([w[0], w[1]], 1), torch.stack([w[2], w[3]], 1)
        d.waypoints[2, 0], d.euler_deg[2, 0] = float("nan"), float("nan")
        completed, steps = skills.execute(robot, d, "pour")["pour"]
        got = final(robot)
        others = torch.arange(B, device=sim.device) != 2
        assert int(completed[2]) == 0 and int(steps[2]) == 0
        assert (completed[others] == 7).all() and (steps[others] > 0).all()
        f = lambda s: s[:sim.layout.goal_offset].view(torch.int32).view(-1, sim.layout.stride)[:, :B]  # noqa: E731
        assert torch.equal(f(got)[:, others], f(want)[:, others])
        assert not torch.equal(f(got)[:, 2], f(want)[:, 2])
    finally:
        restart(robot, state0)
