// ps_ctx.h — the host side every unit of libpandasim.so shares: the context
// (ps_ctx, ps_step_io), the lists of tasks and scenes with the launchers
// declared from them, and the host helpers that turn a context and a state
// buffer into a kernel's arguments (view_of, scene_of, params_of) or report a
// failure (fail, check_launch).
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "pandasim.h"
#include "ps_state.h"

struct ps_ctx {
    ps_config cfg;
    int64_t num_envs;
    ps_layout lay;
    int device;
    char err[256];
    float *render_prims;  // [B][RENDER_PRIM_FLOATS] scratch of ps_render, allocated on first use
    float *gstash;        // Stack: GSTASH_FLOATS x stride substep stash and pair rows, allocated on first step
    uint8_t *nonfinite;   // ps_set_nonfinite_guard: per-env flag output of ps_step (caller-owned), or NULL
    int reset_nonfinite;  // ... and reset such envs in-kernel
    int lanes_per_env;    // ps_set_lanes_per_env: 0 auto, 1 or 16
    int gains_dirty;      // the state's motor gain rows may differ from the fused step's (store_motor_gains)
    const void *gains_state;  // the state buffer whose gain rows the last successful ps_step wrote
    float *epstats;       // ps_set_episode_stats: caller-owned [4][num_envs] f32, or NULL
};

// arguments of ps_step that the step launchers pass through
struct ps_step_io {
    const float *actions;
    float *obs, *ag, *dg, *reward;
    uint8_t *terminated, *truncated;
    float *final_obs, *final_ag;
    int autoreset;
    const float *orn;  // ps_step_oriented: [B, 4] target quaternions (x, y, z, w); NULL in ps_step
};

// ps_motion_program's program as its kernel takes it, by value: the checked
// host arrays packed (ps_motion_program, pandasim.hip) and the device arrays
struct ps_program_args {
    int32_t num_segments;
    uint32_t blocked;  // bit s: the gripper's blocked flag while segment s runs
    uint64_t kinds;    // two bits per segment: PS_SEG_*
    uint16_t wait[PS_PROGRAM_MAX_SEGMENTS];  // control steps of a wait segment
    const float *goal_pos, *goal_quat, *width;  // [S, B, 3], [S, B, 4], [S, B] (width: or NULL)
    const uint8_t *mask;                        // [S, B] or NULL
    int32_t *completed, *steps;                 // [B] or NULL
};

// The sets the library is built over, each written once here and once in
// pandasim/build.py (TASKS, GROUP_TASKS, SCENES), as the numerals the
// launcher names and the units' -D defines carry:
//   tasks (PS_TASK_*), those with 16- and 8-lane group kernels first -- Stack
//   (4: two objects, 21 DoFs) has none;
//   scenes of the plugin path, the motion primitives and the motion
//   programs, (objects, shape).
#define PS_FOR_EACH_GROUP_TASK(X) X(0) X(1) X(2) X(3) X(5)
#define PS_FOR_EACH_TASK(X) PS_FOR_EACH_GROUP_TASK(X) X(4)
#define PS_FOR_EACH_SCENE(X) X(0, 0) X(1, 0) X(1, 1) X(2, 0)

// one launcher per (task, control) pair (step_kernels.hip) and per scene
// (sim_kernels.hip); each lives in its own object
#define PS_STEP_LAUNCHER_NAME_(T, C) ps_launch_step_##T##_##C
#define PS_STEP_LAUNCHER_NAME(T, C) PS_STEP_LAUNCHER_NAME_(T, C)
// the 16- and 8-lane group kernels of a pair (not Stack) live in an object of
// their own (step_kernels.hip with -DPS_STEP_GROUPS=1), called by the pair's
// launcher
#define PS_STEP_GROUP_LAUNCHER_NAME_(T, C) ps_launch_step_groups_##T##_##C
#define PS_STEP_GROUP_LAUNCHER_NAME(T, C) PS_STEP_GROUP_LAUNCHER_NAME_(T, C)
// ps_step_oriented's kernels (k_step<..., ORI = true>, ee control only): the
// same split, built from step_kernels.hip with -DPS_STEP_ORI=1
#define PS_STEP_ORI_LAUNCHER_NAME_(T) ps_launch_step_ori_##T
#define PS_STEP_ORI_LAUNCHER_NAME(T) PS_STEP_ORI_LAUNCHER_NAME_(T)
#define PS_STEP_ORI_GROUP_LAUNCHER_NAME_(T) ps_launch_step_ori_groups_##T
#define PS_STEP_ORI_GROUP_LAUNCHER_NAME(T) PS_STEP_ORI_GROUP_LAUNCHER_NAME_(T)
#define PS_SIM_LAUNCHER_NAME_(NOBJ, SHAPE) ps_launch_sim_step_##NOBJ##_##SHAPE
#define PS_SIM_LAUNCHER_NAME(NOBJ, SHAPE) PS_SIM_LAUNCHER_NAME_(NOBJ, SHAPE)
// ps_motion_run's kernel of each scene (motion_kernels.hip)
#define PS_MOTION_LAUNCHER_NAME_(NOBJ, SHAPE) ps_launch_motion_##NOBJ##_##SHAPE
#define PS_MOTION_LAUNCHER_NAME(NOBJ, SHAPE) PS_MOTION_LAUNCHER_NAME_(NOBJ, SHAPE)
// ps_motion_program's kernel of each scene (program_kernels.hip)
#define PS_PROGRAM_LAUNCHER_NAME_(NOBJ, SHAPE) ps_launch_program_##NOBJ##_##SHAPE
#define PS_PROGRAM_LAUNCHER_NAME(NOBJ, SHAPE) PS_PROGRAM_LAUNCHER_NAME_(NOBJ, SHAPE)

typedef int ps_step_launcher(ps_ctx *c, void *state, const ps_step_io &io, int lanes, hipStream_t st);
typedef int ps_step_group_launcher(ps_ctx *c, const void *params, const ps_step_io &io, int lanes, hipStream_t st);
typedef int ps_sim_launcher(ps_ctx *c, void *state, int n_substeps, hipStream_t st);
typedef int ps_motion_launcher(ps_ctx *c, void *state, void *plan, int max_steps, hipStream_t st);
typedef int ps_program_launcher(ps_ctx *c, void *state, void *plan, const ps_program_args &prog, hipStream_t st);
#define PS_DECLARE_STEP_LAUNCHERS(T) \
    ps_step_launcher PS_STEP_LAUNCHER_NAME(T, 0), PS_STEP_LAUNCHER_NAME(T, 1), PS_STEP_ORI_LAUNCHER_NAME(T);
#define PS_DECLARE_STEP_GROUP_LAUNCHERS(T)                                                        \
    ps_step_group_launcher PS_STEP_GROUP_LAUNCHER_NAME(T, 0), PS_STEP_GROUP_LAUNCHER_NAME(T, 1), \
        PS_STEP_ORI_GROUP_LAUNCHER_NAME(T);
#define PS_DECLARE_SCENE_LAUNCHERS(NOBJ, SHAPE)               \
    ps_sim_launcher PS_SIM_LAUNCHER_NAME(NOBJ, SHAPE);       \
    ps_motion_launcher PS_MOTION_LAUNCHER_NAME(NOBJ, SHAPE); \
    ps_program_launcher PS_PROGRAM_LAUNCHER_NAME(NOBJ, SHAPE);
// (the group launchers are declared for every task and defined for the group
// tasks: a pair's launcher names its own behind `if constexpr (task_has_groups)`)
PS_FOR_EACH_TASK(PS_DECLARE_STEP_LAUNCHERS)
PS_FOR_EACH_TASK(PS_DECLARE_STEP_GROUP_LAUNCHERS)
PS_FOR_EACH_SCENE(PS_DECLARE_SCENE_LAUNCHERS)

// the phase-counter buffer of the diagnostic build (pandasim.hip)
#ifdef PS_PROFILE_PHASES
unsigned long long *ps_prof_buffer();
#define PS_ITER_DUMP_ENVS 131072
uint32_t *ps_iter_dump_buffer();
#endif
#ifdef PS_DEBUG_ROW_DUMP
float *ps_row_dump_buffer();
#endif

namespace {

// whether `task` is one of PS_FOR_EACH_GROUP_TASK
constexpr bool task_has_groups(int task) {
#define PS_TASK_IS(T) || task == T
    return false PS_FOR_EACH_GROUP_TASK(PS_TASK_IS);
#undef PS_TASK_IS
}

inline int task_nobj(int task) { return task == PS_TASK_REACH ? 0 : (task == PS_TASK_STACK ? 2 : 1); }
inline int task_goal_dim(int task) { return task == PS_TASK_STACK ? 6 : (task == PS_TASK_FLIP ? 4 : 3); }
inline int task_obs_dim(int task) {
    return task == PS_TASK_REACH ? 0 : (task == PS_TASK_STACK ? 24 : (task == PS_TASK_FLIP ? 13 : 12));
}

inline StateView view_of(const ps_ctx *c, void *state) {
    char *b = (char *)state;
    StateView v;
    v.f = (float *)(b + c->lay.float_offset);
    v.goal = (double *)(b + c->lay.goal_offset);
    v.rng = (uint64_t *)(b + c->lay.rng_offset);
    v.elapsed = (int32_t *)(b + c->lay.elapsed_offset);
    v.stride = c->lay.stride;
    return v;
}

inline Scene scene_of(const ps_config &c) {
    Scene s;
    s.base = mk(c.base[0], c.base[1], c.base[2]);
    s.half = mk(c.object_half[0], c.object_half[1], c.object_half[2]);
    s.mass = c.object_mass;
    s.mass2 = c.object2_mass;
    s.fric = c.object_friction;
    s.table_cx = c.table_cx;
    s.table_hx = c.table_hx;
    s.table_hy = c.table_hy;
    s.has_table = c.has_table;
    s.has_plane = c.has_plane;
    return s;
}

// ----------------------------------------------------------- host helpers
inline int fail(ps_ctx *c, int code, const char *msg) {
    if (c) snprintf(c->err, sizeof c->err, "%s", msg);
    return code;
}

inline int check_launch(ps_ctx *c) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (c) snprintf(c->err, sizeof c->err, "HIP launch failed: %s", hipGetErrorString(e));
        return PS_ERR_HIP;
    }
    return PS_OK;
}

inline KParams params_of(ps_ctx *c, void *state) {
    KParams P;
    P.s = view_of(c, state);
    P.n = c->num_envs;
    P.sc = scene_of(c->cfg);
    P.reward_type = c->cfg.reward;
    P.block_gripper = c->cfg.block_gripper;
    P.obs_dim = ps_obs_dim(c);
    P.action_dim = ps_action_dim(c);
    P.autoreset = 0;
    P.gstash = c->gstash;
    P.nonfinite = nullptr;
    P.reset_nonfinite = 0;
    P.write_gains = 0;
    P.epstats = c->epstats;
    P.epstride = c->num_envs;
#ifdef PS_PROFILE_PHASES
    P.prof = ps_prof_buffer();
    P.itdump = ps_iter_dump_buffer();
#endif
#ifdef PS_DEBUG_ROW_DUMP
    P.dbg = ps_row_dump_buffer();
#endif
    return P;
}

// Stack's global stash (the LDS it would use holds its ground rows): one
// allocation on the first step of a two-object context, never per step
inline int ensure_stash(ps_ctx *c, hipStream_t st) {
    if (c->cfg.n_objects != 2 || c->gstash) return PS_OK;
    const size_t bytes = sizeof(float) * ((int64_t)GSTASH_FLOATS * c->lay.stride + GSTASH_ZERO_FLOATS);
    float *buf = nullptr;
    if (hipMalloc((void **)&buf, bytes) != hipSuccess) return PS_ERR_HIP;
    // all-zero (the solver's zero block after the stash, GSTASH_ZERO_FLOATS),
    // on the stream the steps run on; the context takes the buffer only once
    // the memset is enqueued, so no later step can find it unzeroed
    if (hipMemsetAsync(buf, 0, bytes, st) != hipSuccess) {
        (void)hipFree(buf);
        return PS_ERR_HIP;
    }
    c->gstash = buf;
    return PS_OK;
}

inline dim3 grid_of(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }


// the registered scene of each task (its _create_scene + panda_tasks.py)
inline bool scene_matches_task(const ps_config &c) {
    return c.n_objects == task_nobj(c.task) &&
           (c.n_objects == 0 || c.object_shape == (c.task == PS_TASK_SLIDE ? PS_SHAPE_CYLINDER : PS_SHAPE_BOX));
}

}  // namespace
