// ps_physics.h — per-env (one env per lane) fp32 Panda multibody step for
// gfx950.  Same algorithm as the PyBullet 3.2.5 subset used by
// panda_gym/pybullet.py (restated in DESIGN.md §5), derived for a
// register-resident lane:
//   * forward kinematics with exact URDF origin rotations (12 links)
//   * mass matrix by composite rigid bodies in the base frame, bias forces by
//     a recursive Newton-Euler pass with prefix sums (gravity, gyroscopic,
//     btMultiBody damping)
//   * 9x9 Cholesky -> M^-1; joint-space rows (motors, limits) use columns of
//     M^-1 directly; cube-ground rows act only on the cube's 6 DoF;
//     gripper-contact rows carry explicit 9-wide Jacobians
//   * projected Gauss-Seidel in btMultiBodyConstraintSolver order
//   * semi-implicit Euler, exponential-map quaternion update.
//
// This header only gathers the parts:
//   ps_kinematics.h    link frames, DoF axes (fk, dof_axis)
//   ps_dynamics.h      mass_matrix, bias_forces, spd_inverse, inverse_kinematics
//   ps_scene.h         scene, objects, LDS / stash layout, contact row records
//   ps_collide.h       gripper boxes, box_box, robot_candidates
//   ps_solver.h        row helpers, residual and clamps, WarmCache, cone_scale
//   ps_solver_group.h  group_pgs (16 or 8 lanes per env)
//   ps_substep.h       limit_side, split_of, substep() with the one-lane solver
#pragma once

#include "ps_common.h"
#include "ps_kinematics.h"
#include "ps_dynamics.h"
#include "ps_scene.h"
#include "ps_collide.h"
#include "ps_solver.h"
#include "ps_solver_group.h"
#include "ps_substep.h"
