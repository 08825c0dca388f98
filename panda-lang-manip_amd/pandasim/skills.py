"""The skills of the language-manipulation policy loop
(panda_gym/envs/task_classes/run_policy.py:189-193, 287-339, 383-390) as motion
programs: reset_robot, pour, open_ and close, and execute, which runs the skill
an action names on the waypoints PandaSim.predict_waypoints decoded.

Every run of primitives between two robot.reset() calls is one MotionProgram,
so one launch (Panda.run); robot.reset() itself stays a Python call, where the
reference calls reset_robot in mid-skill.  Positions and angles are [B, 3] (or
one env's [3]) and may be device tensors: nothing here reads a tensor's value
on the host.  An env whose waypoint is NaN (an empty point set) stops at the
move that would go there and runs nothing after it in that program
(ps_motion_program); the programs after a robot.reset() start afresh.
"""
from __future__ import annotations

import torch

from .panda_cartesian import MotionProgram

WAIT_STEPS = 50                 # `for i in range(50): self.sim.step()` (run_policy.py:294, 297, 337)
HOME_POS = (0.0, 0.0, 0.6)      # reset_robot's goal (:192)
HOME_EULER = (180.0, 0.0, 0.0)  # "standard" (:191)
LIFT = (0.0, 0.0, 0.10)         # pour's approach and lift above the start (:327, :331)
LINE_STEPS = 15                 # open's and close's straight line (:302, :317)
ACTIONS = ("pour", "open", "close")


def _program(robot) -> MotionProgram:
    return MotionProgram(robot.sim.num_envs, robot.sim.device)


def _rows(robot, x) -> torch.Tensor:
    return torch.as_tensor(x, dtype=torch.float32, device=robot.sim.device)


def _reset_joints(robot, mask) -> None:
    """robot.reset() for the envs of `mask` (None: all), on the device: the
    other envs keep every float row as it was."""
    if mask is None:
        robot.reset()
        return
    sim = robot.sim
    rows = sim.f[:, :sim.num_envs]
    before = rows.clone()
    robot.reset()
    keep = torch.as_tensor(mask, device=sim.device) == 0
    rows.copy_(torch.where(keep, before, rows))


def home(program: MotionProgram, mask=None) -> MotionProgram:
    """reset_robot after its robot.reset(): move to the home pose, release (:191-193)."""
    return program.move(HOME_POS, HOME_EULER, mask).release(mask=mask)


def reset_robot(robot, mask=None):
    """run_policy.py:189-193.  Returns Panda.run's (completed, steps)."""
    _reset_joints(robot, mask)
    return robot.run(home(_program(robot), mask))


def pour(robot, start_pos, end_pos, start_euler, end_euler, mask=None):
    """parameterized_pour (:325-339): above the start, down, grasp, lift, over
    to the end, turn to the end angles, wait; then reset_robot.  Returns the
    (completed, steps) of the skill's program (not of the reset after it)."""
    start_pos, end_pos = _rows(robot, start_pos), _rows(robot, end_pos)
    above = start_pos + _rows(robot, LIFT)
    p = _program(robot)
    p.move(above, start_euler, mask).move(start_pos, start_euler, mask).grasp(mask)
    p.move(above, start_euler, mask).move(end_pos, start_euler, mask).move(end_pos, end_euler, mask)
    p.wait(WAIT_STEPS, mask)
    out = robot.run(p)
    reset_robot(robot, mask)
    return out


def open_(robot, grasp_pos, approach_pos, grasp_euler, approach_euler=None, mask=None):
    """parameterized_open (:287-309), which execute calls with (start, end) as
    (grasp, approach): reset_robot; to the approach, wait, to the grasp, wait,
    grasp, back to the approach along 15 goals, release; reset_robot.  Every
    move holds grasp_euler (approach_euler is not read, as there)."""
    grasp_pos, approach_pos = _rows(robot, grasp_pos), _rows(robot, approach_pos)
    _reset_joints(robot, mask)
    p = home(_program(robot), mask)
    p.move(approach_pos, grasp_euler, mask).wait(WAIT_STEPS, mask).move(grasp_pos, grasp_euler, mask)
    p.wait(WAIT_STEPS, mask).grasp(mask)
    delta = (approach_pos - grasp_pos) / LINE_STEPS
    for i in range(LINE_STEPS):
        p.move(grasp_pos + i * delta, grasp_euler, mask)
    p.release(mask=mask)
    out = robot.run(p)
    reset_robot(robot, mask)
    return out


def close(robot, approach_pos, grasp_pos, approach_euler, grasp_euler, mask=None):
    """parameterized_close (:311-323): from the approach towards the grasp
    along 15 goals, all at grasp_euler, with a grasp after the fourth."""
    approach_pos, grasp_pos = _rows(robot, approach_pos), _rows(robot, grasp_pos)
    delta = (approach_pos - grasp_pos) / LINE_STEPS
    p = _program(robot)
    for i in range(LINE_STEPS):
        p.move(approach_pos - i * delta, grasp_euler, mask)
        if i == 3:
            p.grasp(mask)
    return robot.run(p)


SKILLS = {"pour": pour, "open": open_, "close": close}


def execute(robot, decoded, action):
    """TableTop.execute after its predict (:383-390): the skill `action` names
    ("pour", "open" or "close") on `decoded`, a DecodedWaypoints or the tuple
    (start_pos, end_pos, start_euler, end_euler) of [B, 3] tensors, in the
    reference's argument order for every skill.

    `action` may be a list of one name per env.  Each distinct skill then
    runs, in the order of its first env, as its own programs masked to its
    envs: the gripper's blocked flag is one bool for the whole batch, as in
    the reference, so the segments of two skills cannot share a program
    without one skill's grasp reaching the other's moves; every skill starts
    from the flag the robot had at the call, and the robot keeps the last
    skill's.  Each env ends where it would running its own action alone.
    Returns {action: (completed, steps)}."""
    if hasattr(decoded, "waypoints"):
        args = (decoded.waypoints[:, 0], decoded.waypoints[:, 1], decoded.euler_deg[:, 0], decoded.euler_deg[:, 1])
    else:
        args = tuple(decoded)
        if len(args) != 4:
            raise ValueError(f"execute: decoded must be a DecodedWaypoints or (start_pos, end_pos, start_euler, "
                             f"end_euler), got {len(args)} items")
    B = robot.sim.num_envs
    if isinstance(action, str):
        names, per_env = [action], None
    else:
        per_env = list(action)
        if len(per_env) != B:
            raise ValueError(f"execute: action holds {len(per_env)} names for {B} envs")
        names = list(dict.fromkeys(per_env))
    for name in names:
        if name not in SKILLS:
            raise ValueError(f"execute: action {name!r} (one of {', '.join(ACTIONS)})")
    blocked, out = robot.block_gripper, {}
    for name in names:
        mask = None if per_env is None else torch.tensor([a == name for a in per_env], dtype=torch.uint8,
                                                         device=robot.sim.device)
        robot.block_gripper = blocked
        out[name] = SKILLS[name](robot, *args, mask=mask)
    return out
