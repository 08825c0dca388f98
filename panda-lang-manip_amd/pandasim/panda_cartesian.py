"""Batched Cartesian Panda of the language-manipulation pipeline
(panda_gym/envs/robots/panda_cartesian.py:11-230): unscaled set_action and the
motion primitives move / grasp / release, which run fused on the GPU
(ps_plan_move / ps_plan_grasp / ps_plan_release + ps_motion_run)."""
from __future__ import annotations

import torch

from . import robots


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
