// ps_env.h — the env layer shared by the kernel translation units of
// libpandasim.so, on top of the physics headers ps_physics.h gathers.  This
// header only gathers the layers:
//   ps_task_rng.h  PCG64 + SeedSequence + Generator.uniform, opaque(), euler_from_quat
//   ps_state.h     StateView, KParams, bind_stack, load / store of the state rows
//   ps_ctx.h       ps_ctx, ps_step_io, the task and scene lists and their
//                  launchers, params_of, ensure_stash, fail, check_launch
//   ps_task.h      TaskTraits, write_obs, goal_metric, reward_for, reset_env, set_action
//   ps_step.h      run_substeps, k_step, k_sim_step
// Each step_kernels.hip object instantiates the step kernels of one (task,
// control) pair and sim_kernels.hip / motion_kernels.hip those of one scene,
// so the library builds as parallel hipcc jobs (pandasim/build.py).  The
// units without the substep (state_kernels.hip, render_kernels.hip,
// pandasim.hip) include the layers they use, not this header.
#pragma once

#include "ps_physics.h"
#include "ps_task_rng.h"
#include "ps_state.h"
#include "ps_ctx.h"
#include "ps_task.h"
#include "ps_step.h"
