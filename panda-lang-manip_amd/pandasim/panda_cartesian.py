"""Batched Cartesian Panda of the language-manipulation pipeline
(panda_gym/envs/robots/panda_cartesian.py:11-230): unscaled set_action and the
motion primitives move / grasp / release, which run fused on the GPU
(ps_plan_move / ps_plan_grasp / ps_plan_release + ps_motion_run), and
MotionProgram, a sequence of them that Panda.run executes in one launch
(ps_motion_program)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import robots


class LoweredProgram(NamedTuple):
    """A MotionProgram as ps_motion_program takes it: per segment the kind
    (L.SEG_*), the wait count (0 for another kind) and the gripper's blocked
    flag while it runs, the flag after the last segment, and the tensors
    goal_pos [S, B, 3], goal_euler [S, B, 3] (zero rows for segments that are
    no move; None without a move), width [S, B] (1 but for a release's row;
    None without a release) and mask [S, B] u8 (None when no segment has one)."""
    kinds: list
    wait_steps: list
    blocked: list
    blocked_after: bool
    goal_pos: Optional[torch.Tensor]
    goal_euler: Optional[torch.Tensor]
    width: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]


def program_flags(kinds, wait_steps, blocked: bool):
    """The host half of a program's checks (ValueError; no tensor, no device):
    1 to PROGRAM_MAX_SEGMENTS segments of known kinds, a wait of 1 to
    PROGRAM_MAX_WAIT control steps.  -> (the gripper's blocked flag while each
    segment runs, the flag after the last): it starts from `blocked`, a grasp
    sets it and a release clears it, as Panda.grasp / release do the robot's
    bool whatever their masks are."""
    kinds, wait_steps = list(kinds), list(wait_steps)
    if not 1 <= len(kinds) <= L.PROGRAM_MAX_SEGMENTS:
        raise ValueError(f"program: {len(kinds)} segments (1 to {L.PROGRAM_MAX_SEGMENTS})")
    if len(wait_steps) != len(kinds):
        raise ValueError(f"program: wait_steps holds {len(wait_steps)} counts for {len(kinds)} segments")
    flags, b = [], bool(blocked)
    for s, (k, n) in enumerate(zip(kinds, wait_steps)):
        if k not in (L.SEG_MOVE, L.SEG_GRASP, L.SEG_RELEASE, L.SEG_WAIT):
            raise ValueError(f"program: segment {s} has the unknown kind {k!r}")
        if k == L.SEG_WAIT:
            _wait_count(n)
        b = True if k == L.SEG_GRASP else (False if k == L.SEG_RELEASE else b)
        flags.append(b)
    return flags, b


def _wait_count(n) -> int:
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= L.PROGRAM_MAX_WAIT:
        raise ValueError(f"wait: n = {n!r} (a whole number of control steps from 1 to {L.PROGRAM_MAX_WAIT})")
    return int(n)


class MotionProgram:
    """A sequence of primitives for a batch of num_envs envs, built with
    move / grasp / release / wait (the arguments of Panda's methods; each
    returns the program) and run by Panda.run in one launch.  Goals, widths
    and masks may be tensors on `device`; none of their values is read on the
    host, so a goal can be what predict_waypoints left on the GPU."""

    def __init__(self, num_envs: int, device="cuda") -> None:
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.segments = []  # (kind, wait count, goal_pos, goal_euler, width, mask): [B, ...] views or None

    def __len__(self) -> int:
        return len(self.segments)

    def _rows(self, name: str, value, width: int, dtype=torch.float32) -> torch.Tensor:
        """value as [B, width] (width 0: [B]), broadcast from one env's."""
        B = self.num_envs
        t = torch.as_tensor(value, device=self.device)
        want = ((B, width), (width,)) if width else ((B,), ())
        if tuple(t.shape) not in want:
            raise ValueError(f"{name}: expected {' or '.join(str(w) for w in want)}, got {tuple(t.shape)}")
        return t.to(dtype).expand(want[0])

    def _mask(self, mask):
        if mask is None:
            return None
        m = torch.as_tensor(mask, device=self.device)
        if tuple(m.shape) != (self.num_envs,):
            raise ValueError(f"mask: expected ({self.num_envs},), got {tuple(m.shape)}")
        return (m != 0).to(torch.uint8)

    def _add(self, kind, n=0, pos=None, euler=None, width=None, mask=None) -> "MotionProgram":
        if len(self.segments) >= L.PROGRAM_MAX_SEGMENTS:
            raise ValueError(f"program: more than {L.PROGRAM_MAX_SEGMENTS} segments")
        self.segments.append((kind, n, pos, euler, width, self._mask(mask)))
        return self

    def move(self, goal_pos, goal_euler, mask=None) -> "MotionProgram":
        """Panda.move: goal_pos [3] or [B, 3] world, goal_euler [3] or [B, 3] degrees."""
        return self._add(L.SEG_MOVE, pos=self._rows("goal_pos", goal_pos, 3), euler=self._rows("goal_euler", goal_euler, 3),
                         mask=mask)

    def grasp(self, mask=None) -> "MotionProgram":
        return self._add(L.SEG_GRASP, mask=mask)

    def release(self, width=1, mask=None) -> "MotionProgram":
        """Panda.release: width a number or [B]."""
        return self._add(L.SEG_RELEASE, width=self._rows("width", width, 0), mask=mask)

    def wait(self, n: int, mask=None) -> "MotionProgram":
        """n times sim.step() with the motors as the step before left them."""
        return self._add(L.SEG_WAIT, n=_wait_count(n), mask=mask)

    def lower(self, blocked: bool) -> LoweredProgram:
        """The program as ps_motion_program takes it, from the robot's
        block_gripper before it."""
        kinds, waits = [g[0] for g in self.segments], [g[1] for g in self.segments]
        flags, after = program_flags(kinds, waits, blocked)
        B, dev = self.num_envs, self.device

        def stack(col, width, fill, dtype, present):
            if not present:
                return None
            shape = (B, width) if width else (B,)
            blank = torch.full(shape, fill, dtype=dtype, device=dev)
            return torch.stack([blank if g[col] is None else g[col] for g in self.segments]).contiguous()

        return LoweredProgram(kinds, waits, flags, after,
                              stack(2, 3, 0.0, torch.float32, L.SEG_MOVE in kinds),
                              stack(3, 3, 0.0, torch.float32, L.SEG_MOVE in kinds),
                              stack(4, 0, 1.0, torch.float32, L.SEG_RELEASE in kinds),
                              stack(5, 0, 1, torch.uint8, any(g[5] is not None for g in self.segments)))


class Panda(robots.Panda):
    """robots.Panda with panda_cartesian.py's action scaling (the displacement
    and the finger command are taken as they are: :67, :157) and its
    primitives.  ``block_gripper`` is the robot's bool for the whole batch, as
    in the reference; grasp() sets it, release() clears it."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self._plan = None

    # ------------------------------------------------------------ set_action
    def set_action(self, action: torch.Tensor, euler_xyz=None) -> None:
        """panda_cartesian.py:53-72."""
        action = torch.as_tensor(action, dtype=torch.float32, device=self.sim.device).clone()
        action = action.clamp(-1.0, 1.0)
        if self.control_type == "ee":
            target_arm_angles = self.ee_displacement_to_target_arm_angles(action[:, :3], euler_xyz)
        else:
            target_arm_angles = self.arm_joint_ctrl_to_target_arm_angles(action[:, :7])
        if self.block_gripper:
            target_fingers_width = torch.zeros(action.shape[0], device=action.device)
        else:
            target_fingers_width = self.get_fingers_width() + action[:, -1]  # unscaled (:67)
        half = (target_fingers_width / 2).unsqueeze(-1)
        self.control_joints(target_angles=torch.cat([target_arm_angles, half, half], dim=-1))

    def ee_displacement_to_target_arm_angles(self, ee_displacement: torch.Tensor, euler_xyz=None) -> torch.Tensor:
        """panda_cartesian.py:147-176: the displacement is not scaled (:157)."""
        target_ee_position = self.get_ee_position() + ee_displacement[:, :3]
        target_ee_position[:, 2] = target_ee_position[:, 2].clamp(min=0.0)
        if euler_xyz is not None:
            orientation = self.sim.euler_xyz_to_quat(euler_xyz)
        else:
            orientation = [1.0, 0.0, 0.0, 0.0]
        return self.inverse_kinematics(link=self.ee_link, position=target_ee_position,
                                       orientation=orientation)[:, :7]

    # ------------------------------------------------------------ primitives
    def _motion_plan(self):
        if self._plan is None:
            self._plan = self.sim.motion_plan()
        return self._plan

    def _run(self, plan, chunk) -> int:
        """Runs the plan to its end: the largest num_steps is read back (one
        sync), then one ps_motion_run, or several of `chunk` control steps."""
        n = int(plan.num_steps.max())
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk: expected a positive number of control steps, got {chunk}")
        step = n if chunk is None else int(chunk)
        for start in range(0, n, step):
            self.sim.motion_run(plan, min(step, n - start))
        return n

    def run(self, program: MotionProgram):
        """Runs the program in one launch, every env through its own segments
        to the end (sim.motion_program), and leaves block_gripper as the same
        move / grasp / release calls would.  Returns (completed [B] i32: the
        first segment an env did not run, len(program) when it ran all;
        steps [B] i32: its control steps), on the device; nothing is read back."""
        completed, steps, after = self.sim.motion_program(self._motion_plan(), program, self.block_gripper)
        self.block_gripper = after
        return completed, steps

    def move(self, goal_pos, goal_euler, mask=None, chunk=None) -> int:
        """panda_cartesian.py:98-122 for every env (mask: [B], nonzero = move):
        goal_pos [3] or [B, 3] world, goal_euler [3] or [B, 3] degrees
        (extrinsic 'xyz').  Returns the largest number of control steps."""
        plan = self._motion_plan()
        plan.blocked.fill_(int(bool(self.block_gripper)))
        self.sim.plan_move(plan, goal_pos, self.sim.euler_xyz_to_quat(goal_euler), mask)
        return self._run(plan, chunk)

    def grasp(self, mask=None, chunk=None) -> int:
        """panda_cartesian.py:124-130."""
        self.block_gripper = True
        plan = self._motion_plan()
        self.sim.plan_grasp(plan, mask)
        return self._run(plan, chunk)

    def release(self, width=1, mask=None, chunk=None) -> int:
        """panda_cartesian.py:139-145."""
        self.block_gripper = False
        plan = self._motion_plan()
        self.sim.plan_release(plan, width, mask)
        return self._run(plan, chunk)
