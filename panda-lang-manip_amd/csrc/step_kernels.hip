// step_kernels.hip — the fused step kernels (k_step, ps_step.h) of one
// (task, control) pair: built once per pair with -DPS_STEP_TASK=t
// -DPS_STEP_CONTROL=c (pandasim/build.py), so the pairs compile as parallel
// jobs.  ps_step (pandasim.hip) calls the pair's launcher.  The one-lane
// kernel and the launcher form one object; the 16- and 8-lane group kernels
// form a second (-DPS_STEP_GROUPS=1), compiled with the same flags (-O3;
// DESIGN.md §12.6).  -DPS_STEP_ORI=1 (ee control only) builds the same two
// objects of ps_step_oriented's kernels, k_step<..., ORI = true>, whose IK
// target takes a per-env orientation.
#include "ps_env.h"

#if !defined(PS_STEP_TASK) || !defined(PS_STEP_CONTROL)
#error "build with -DPS_STEP_TASK=<task> -DPS_STEP_CONTROL=<control>"
#endif

#if defined(PS_STEP_ORI) && PS_STEP_ORI
#if PS_STEP_CONTROL != 0  // PS_CONTROL_EE
#error "-DPS_STEP_ORI=1 needs -DPS_STEP_CONTROL=0 (ee control)"
#endif
#define PS_ORI true
#define PS_THIS_LAUNCHER PS_STEP_ORI_LAUNCHER_NAME(PS_STEP_TASK)
#define PS_THIS_GROUP_LAUNCHER PS_STEP_ORI_GROUP_LAUNCHER_NAME(PS_STEP_TASK)
#else
#define PS_ORI false
#define PS_THIS_LAUNCHER PS_STEP_LAUNCHER_NAME(PS_STEP_TASK, PS_STEP_CONTROL)
#define PS_THIS_GROUP_LAUNCHER PS_STEP_GROUP_LAUNCHER_NAME(PS_STEP_TASK, PS_STEP_CONTROL)
#endif

#define PS_LAUNCH(G)                                                                                         \
    hipLaunchKernelGGL((k_step<PS_STEP_TASK, PS_STEP_CONTROL, G, PS_ORI>), grid_of(P.n * (G), kBlock),       \
                       dim3(kBlock), 0, st, P, io.actions, io.obs, io.ag, io.dg, io.reward, io.terminated,   \
                       io.truncated, io.final_obs, io.final_ag, io.orn)

#if defined(PS_STEP_GROUPS) && PS_STEP_GROUPS
static_assert(task_has_groups(PS_STEP_TASK), "Stack has no group kernels (two objects: 21 DoFs)");

int PS_THIS_GROUP_LAUNCHER(ps_ctx *c, const void *params, const ps_step_io &io, int lanes, hipStream_t st) {
    const KParams P = *static_cast<const KParams *>(params);
    if (lanes == 16) PS_LAUNCH(16);
    else PS_LAUNCH(8);
    return check_launch(c);
}

#else
int PS_THIS_LAUNCHER(ps_ctx *c, void *state, const ps_step_io &io, int lanes, hipStream_t st) {
    KParams P = params_of(c, state);
    P.autoreset = io.autoreset;
    P.nonfinite = c->nonfinite;
    P.reset_nonfinite = c->reset_nonfinite;
    // the gain rows belong to a state buffer: another buffer than the one the
    // last step wrote (a swapped or copied-in state) gets them written too
    P.write_gains = c->gains_dirty || state != c->gains_state;
    // groups of 16 or 8 lanes per env exist for the one-object and robot-only
    // tasks (PS_FOR_EACH_GROUP_TASK, ps_ctx.h)
    if constexpr (task_has_groups(PS_STEP_TASK)) {
        if (lanes == 16 || lanes == 8) return PS_THIS_GROUP_LAUNCHER(c, &P, io, lanes, st);
    }
    PS_LAUNCH(1);
    return check_launch(c);
}
#endif
#undef PS_LAUNCH
