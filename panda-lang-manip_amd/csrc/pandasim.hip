// pandasim.hip — the host side of the C ABI (include/pandasim.h) of the
// batched Panda simulator: configuration, layout and context, the dimension
// getters and the setters, and the entry points that dispatch to another
// unit's launcher (ps_step, ps_step_oriented: step_kernels.hip; ps_sim_step:
// sim_kernels.hip; ps_motion_run: motion_kernels.hip; ps_motion_program:
// program_kernels.hip), with the diagnostic
// builds' buffers.  No kernel lives here: every other entry point sits in
// the unit of its kernel (state_kernels.hip, plan_kernels.hip,
// render_kernels.hip).
#include <new>

#include "ps_ctx.h"

#ifdef PS_PROFILE_PHASES
// phase counters of the diagnostic build: one device buffer that every
// step object's kernels add to (KParams::prof)
static unsigned long long *g_prof = nullptr;
unsigned long long *ps_prof_buffer() {
    if (!g_prof && hipMalloc((void **)&g_prof, sizeof(unsigned long long) * PS_NUM_PROF_SLOTS) == hipSuccess)
        (void)hipMemset(g_prof, 0, sizeof(unsigned long long) * PS_NUM_PROF_SLOTS);
    return g_prof;
}
// per-env PGS iterations and contact slots of each one-lane kernel launch's 20
// substeps: PS_ITP_WORDS words x PS_ITER_DUMP_ENVS, 16 bits per substep
// (PhaseTimer::itp)
static uint32_t *g_itdump = nullptr;
uint32_t *ps_iter_dump_buffer() {
    if (!g_itdump && hipMalloc((void **)&g_itdump, sizeof(uint32_t) * PS_ITP_WORDS * PS_ITER_DUMP_ENVS) == hipSuccess)
        (void)hipMemset(g_itdump, 0, sizeof(uint32_t) * PS_ITP_WORDS * PS_ITER_DUMP_ENVS);
    return g_itdump;
}
extern "C" int ps_debug_env_iters(uint32_t *out) {
    uint32_t *b = ps_iter_dump_buffer();
    if (!b || hipDeviceSynchronize() != hipSuccess) return PS_ERR_HIP;
    if (hipMemcpy(out, b, sizeof(uint32_t) * PS_ITP_WORDS * PS_ITER_DUMP_ENVS, hipMemcpyDeviceToHost) != hipSuccess)
        return PS_ERR_HIP;
    return PS_OK;
}
extern "C" int ps_debug_phase_cycles(unsigned long long *out, int reset) {
    unsigned long long *b = ps_prof_buffer();
    if (!b || hipDeviceSynchronize() != hipSuccess) return PS_ERR_HIP;
    if (hipMemcpy(out, b, sizeof(unsigned long long) * PS_NUM_PROF_SLOTS, hipMemcpyDeviceToHost) != hipSuccess)
        return PS_ERR_HIP;
    if (reset && hipMemset(b, 0, sizeof(unsigned long long) * PS_NUM_PROF_SLOTS) != hipSuccess) return PS_ERR_HIP;
    return PS_OK;
}
#endif

#ifdef PS_DEBUG_ROW_DUMP
// row dump of the diagnostic build (KParams::dbg): PS_DUMP_LANES lanes x 2
// substeps x PS_DUMP_ROWS floats, NaN where nothing was recorded
static float *g_dump = nullptr;
static const size_t kDumpFloats = (size_t)PS_DUMP_LANES * 2 * PS_DUMP_ROWS;
float *ps_row_dump_buffer() {
    if (!g_dump && hipMalloc((void **)&g_dump, sizeof(float) * kDumpFloats) == hipSuccess)
        (void)hipMemset(g_dump, 0xFF, sizeof(float) * kDumpFloats);
    return g_dump;
}
extern "C" int ps_debug_row_dump(float *out, int reset) {
    float *b = ps_row_dump_buffer();
    if (!b || hipDeviceSynchronize() != hipSuccess) return PS_ERR_HIP;
    if (hipMemcpy(out, b, sizeof(float) * kDumpFloats, hipMemcpyDeviceToHost) != hipSuccess) return PS_ERR_HIP;
    if (reset && hipMemset(b, 0xFF, sizeof(float) * kDumpFloats) != hipSuccess) return PS_ERR_HIP;
    return PS_OK;
}
#endif

// ------------------------------------------------------------------- C ABI
extern "C" {

int ps_abi_version(void) { return PS_ABI_VERSION; }

int ps_default_config(int task, int control, int reward, ps_config *out) {
    if (!out || task < 0 || task >= PS_NUM_TASKS || control < 0 || control > 1 || reward < 0 || reward > 1)
        return PS_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->task = task;
    out->control = control;
    out->reward = reward;
    // Reach/Push/Slide block the gripper (panda_tasks.py:62,78,94)
    out->block_gripper = task == PS_TASK_REACH || task == PS_TASK_PUSH || task == PS_TASK_SLIDE;
    out->has_table = 1;
    out->has_plane = 1;
    out->n_objects = task_nobj(task);
    out->object_shape = task == PS_TASK_SLIDE ? PS_SHAPE_CYLINDER : PS_SHAPE_BOX;
    out->base[0] = (float)PM_BASE_X;
    if (task == PS_TASK_SLIDE) {
        out->object_half[0] = out->object_half[1] = (float)(PM_SLIDE_OBJECT_SIZE / 2);
        out->object_half[2] = (float)(PM_SLIDE_OBJECT_SIZE / 2 / 2);
        out->object_friction = (float)PM_SLIDE_FRICTION;
        out->table_cx = (float)PM_SLIDE_TABLE_CX;
        out->table_hx = (float)PM_SLIDE_TABLE_HX;
    } else {
        out->object_half[0] = out->object_half[1] = out->object_half[2] = (float)(PM_OBJECT_SIZE / 2);
        out->object_friction = (float)PM_DEFAULT_FRICTION;
        out->table_cx = (float)PM_TABLE_CX;
        out->table_hx = (float)PM_TABLE_HX;
    }
    out->table_hy = (float)PM_TABLE_HY;
    out->object_mass = (float)(task == PS_TASK_STACK ? PM_STACK_MASS1 : PM_CUBE_MASS);
    out->object2_mass = (float)PM_STACK_MASS2;
    return PS_OK;
}

int ps_state_layout(int64_t num_envs, ps_layout *out) {
    if (!out || num_envs <= 0 || num_envs > PS_MAX_ENVS) return PS_ERR_ARG;
    int64_t stride = (num_envs + 63) & ~(int64_t)63;
    out->num_envs = num_envs;
    out->stride = stride;
    out->float_offset = 0;
    out->goal_offset = out->float_offset + (int64_t)PS_NUM_FLOAT_ROWS * stride * 4;
    out->rng_offset = out->goal_offset + (int64_t)PS_MAX_GOAL_DIM * stride * 8;
    out->elapsed_offset = out->rng_offset + (int64_t)PS_NUM_RNG_ROWS * stride * 8;
    out->total_bytes = out->elapsed_offset + stride * 4;
    return PS_OK;
}

int ps_create(const ps_config *cfg, int64_t num_envs, int device, ps_ctx **out) {
    if (!cfg || !out || num_envs <= 0 || num_envs > PS_MAX_ENVS) return PS_ERR_ARG;
    if (cfg->task < 0 || cfg->task >= PS_NUM_TASKS || cfg->control < 0 || cfg->control > 1 || cfg->reward < 0 ||
        cfg->reward > 1 || cfg->n_objects < 0 || cfg->n_objects > 2 || cfg->object_shape < 0 || cfg->object_shape > 1)
        return PS_ERR_ARG;
    if (cfg->n_objects > 0) {
        // compiled-in shapes: cubes (isotropic), one upright z cylinder
        if (cfg->object_shape == PS_SHAPE_BOX &&
            (cfg->object_half[0] != cfg->object_half[1] || cfg->object_half[1] != cfg->object_half[2]))
            return PS_ERR_UNSUPPORTED;
        if (cfg->object_shape == PS_SHAPE_CYLINDER &&
            (cfg->n_objects != 1 || cfg->object_half[0] != cfg->object_half[1]))
            return PS_ERR_UNSUPPORTED;
        if (!(cfg->object_mass > 0.0f) || (cfg->n_objects == 2 && !(cfg->object2_mass > 0.0f))) return PS_ERR_ARG;
    }
    ps_ctx *c = new (std::nothrow) ps_ctx;
    if (!c) return PS_ERR_ARG;
    memset(c, 0, sizeof *c);
    c->cfg = *cfg;
    c->num_envs = num_envs;
    c->device = device;
    c->gains_dirty = 1;
    ps_state_layout(num_envs, &c->lay);
    *out = c;
    return PS_OK;
}

void ps_destroy(ps_ctx *ctx) {
    if (ctx && ctx->render_prims) (void)hipFree(ctx->render_prims);
    if (ctx && ctx->gstash) (void)hipFree(ctx->gstash);
    delete ctx;
}

const char *ps_last_error(const ps_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int ps_obs_dim(const ps_ctx *c) { return (c->cfg.block_gripper ? 6 : 7) + task_obs_dim(c->cfg.task); }

int ps_action_dim(const ps_ctx *c) {
    return (c->cfg.control == PS_CONTROL_EE ? 3 : 7) + (c->cfg.block_gripper ? 0 : 1);
}

int ps_goal_dim(const ps_ctx *c) { return task_goal_dim(c->cfg.task); }

int ps_max_episode_steps(const ps_ctx *c) {
    return c->cfg.task == PS_TASK_STACK ? PM_STACK_MAX_EPISODE_STEPS : PM_MAX_EPISODE_STEPS;
}

int ps_mark_motor_rows_dirty(ps_ctx *c) {
    if (!c) return PS_ERR_ARG;
    c->gains_dirty = 1;
    return PS_OK;
}

// ps_step and ps_step_oriented (io.orn != NULL: ee control, checked by the
// caller): one stash, lanes-per-env choice and gain-row bookkeeping
static int step_with(ps_ctx *c, void *state, const ps_step_io &io, void *stream) {
    if (!c || !state || !io.actions || !io.reward || !io.terminated || !io.truncated)
        return fail(c, PS_ERR_ARG, "null argument");
    if (!scene_matches_task(c->cfg)) return fail(c, PS_ERR_UNSUPPORTED, "scene does not match the task");
    hipStream_t st = (hipStream_t)stream;
    if (ensure_stash(c, st) != PS_OK) return fail(c, PS_ERR_HIP, "hipMalloc of the Stack stash failed");
    const int lanes = ps_step_lanes(c);
    const bool ee = c->cfg.control == PS_CONTROL_EE;
    int rc;
#define PS_STEP_TASK_CASE(T)                                                                              \
    case T:                                                                                               \
        rc = io.orn ? PS_STEP_ORI_LAUNCHER_NAME(T)(c, state, io, lanes, st)                               \
             : ee   ? PS_STEP_LAUNCHER_NAME(T, 0)(c, state, io, lanes, st)                                \
                    : PS_STEP_LAUNCHER_NAME(T, 1)(c, state, io, lanes, st);                               \
        break;
    switch (c->cfg.task) {
        PS_FOR_EACH_TASK(PS_STEP_TASK_CASE)
        default: return fail(c, PS_ERR_ARG, "bad task");
    }
#undef PS_STEP_TASK_CASE
    if (rc == PS_OK) {
        c->gains_dirty = 0;
        c->gains_state = state;
    }
    return rc;
}

int ps_step(ps_ctx *c, void *state, const float *actions, float *obs, float *ag, float *dg, float *reward,
            uint8_t *terminated, uint8_t *truncated, int autoreset, float *final_obs, float *final_ag,
            void *stream) {
    const ps_step_io io{actions, obs, ag, dg, reward, terminated, truncated, final_obs, final_ag, autoreset, nullptr};
    return step_with(c, state, io, stream);
}

int ps_step_oriented(ps_ctx *c, void *state, const float *actions, const float *orn, float *obs, float *ag,
                     float *dg, float *reward, uint8_t *terminated, uint8_t *truncated, int autoreset,
                     float *final_obs, float *final_ag, void *stream) {
    if (!c || !orn) return fail(c, PS_ERR_ARG, "null argument");
    if (c->cfg.control != PS_CONTROL_EE)
        return fail(c, PS_ERR_UNSUPPORTED, "a target orientation needs ee control (joints control ignores it: ps_step)");
    const ps_step_io io{actions, obs, ag, dg, reward, terminated, truncated, final_obs, final_ag, autoreset, orn};
    return step_with(c, state, io, stream);
}

int ps_set_lanes_per_env(ps_ctx *c, int lanes) {
    if (!c || !(lanes == 0 || lanes == 1 || lanes == 8 || lanes == 16)) return PS_ERR_ARG;
    if (lanes > 1 && c->cfg.n_objects > 1) return fail(c, PS_ERR_UNSUPPORTED, "8 or 16 lanes per env: one object at most");
    c->lanes_per_env = lanes;
    return PS_OK;
}

int ps_step_lanes(const ps_ctx *c) {
    if (!c) return PS_ERR_ARG;
    if (c->lanes_per_env) return c->lanes_per_env;
    if (c->cfg.n_objects > 1) return 1;
    if (c->num_envs <= PS_GROUP16_AUTO_MAX_ENVS) return 16;
    return c->num_envs <= PS_GROUP8_AUTO_MAX_ENVS ? 8 : 1;
}

int ps_set_episode_stats(ps_ctx *c, float *stats) {
    if (!c) return PS_ERR_ARG;
    c->epstats = stats;
    return PS_OK;
}

int ps_set_nonfinite_guard(ps_ctx *c, uint8_t *flags, int reset_nonfinite) {
    if (!c) return PS_ERR_ARG;
    c->nonfinite = flags;
    c->reset_nonfinite = reset_nonfinite ? 1 : 0;
    return PS_OK;
}

// the launcher of the context's scene: the object count, and with objects
// their shape (ps_create admits the cylinder with one object only)
#define PS_SCENE_CASE(NOBJ, SHAPE) \
    if (c->cfg.n_objects == NOBJ && (NOBJ == 0 || c->cfg.object_shape == SHAPE)) return PS_SCENE_LAUNCH(NOBJ, SHAPE);

int ps_sim_step(ps_ctx *c, void *state, int n_substeps, void *stream) {
    if (!c || !state || n_substeps < 0) return fail(c, PS_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (ensure_stash(c, st) != PS_OK) return fail(c, PS_ERR_HIP, "hipMalloc of the Stack stash failed");
#define PS_SCENE_LAUNCH(NOBJ, SHAPE) PS_SIM_LAUNCHER_NAME(NOBJ, SHAPE)(c, state, n_substeps, st)
    PS_FOR_EACH_SCENE(PS_SCENE_CASE)
#undef PS_SCENE_LAUNCH
    return fail(c, PS_ERR_UNSUPPORTED, "no kernel of this scene");
}

int ps_motion_run(ps_ctx *c, void *state, void *plan, int max_steps, void *stream) {
    if (!c || !state || !plan || max_steps < 1) return fail(c, PS_ERR_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (ensure_stash(c, st) != PS_OK) return fail(c, PS_ERR_HIP, "hipMalloc of the Stack stash failed");
#define PS_SCENE_LAUNCH(NOBJ, SHAPE) PS_MOTION_LAUNCHER_NAME(NOBJ, SHAPE)(c, state, plan, max_steps, st)
    PS_FOR_EACH_SCENE(PS_SCENE_CASE)
#undef PS_SCENE_LAUNCH
    return fail(c, PS_ERR_UNSUPPORTED, "no kernel of this scene");
}

// every check before anything is enqueued (the Stack stash's memset
// included); the host arrays are packed into the kernel's by-value argument,
// the blocked flag of each segment as the sequence of Panda calls leaves it
int ps_motion_program(ps_ctx *c, void *state, void *plan, int num_segments, const int32_t *kinds,
                      const int32_t *wait_steps, int blocked0, const float *goal_pos, const float *goal_quat,
                      const float *width, const uint8_t *mask, int32_t *completed, int32_t *steps, void *stream) {
    if (!c || !state || !plan || !kinds) return fail(c, PS_ERR_ARG, "null argument");
    if (num_segments < 1 || num_segments > PS_PROGRAM_MAX_SEGMENTS)
        return fail(c, PS_ERR_ARG, "num_segments out of range");
    ps_program_args prog;
    memset(&prog, 0, sizeof prog);
    prog.num_segments = num_segments;
    bool blocked = blocked0 != 0;
    for (int s = 0; s < num_segments; s++) {
        const int k = kinds[s];
        if (k == PS_SEG_MOVE) {
            if (!goal_pos || !goal_quat) return fail(c, PS_ERR_ARG, "a move segment needs goal_pos and goal_quat");
        } else if (k == PS_SEG_GRASP) {
            blocked = true;
        } else if (k == PS_SEG_RELEASE) {
            blocked = false;
        } else if (k == PS_SEG_WAIT) {
            if (!wait_steps || wait_steps[s] < 1 || wait_steps[s] > PS_PROGRAM_MAX_WAIT)
                return fail(c, PS_ERR_ARG, "a wait segment's count is out of range");
            prog.wait[s] = (uint16_t)wait_steps[s];
        } else {
            return fail(c, PS_ERR_ARG, "unknown segment kind");
        }
        prog.kinds |= (uint64_t)k << (2 * s);
        prog.blocked |= (uint32_t)blocked << s;
    }
    prog.goal_pos = goal_pos;
    prog.goal_quat = goal_quat;
    prog.width = width;
    prog.mask = mask;
    prog.completed = completed;
    prog.steps = steps;
    hipStream_t st = (hipStream_t)stream;
    if (ensure_stash(c, st) != PS_OK) return fail(c, PS_ERR_HIP, "hipMalloc of the Stack stash failed");
#define PS_SCENE_LAUNCH(NOBJ, SHAPE) PS_PROGRAM_LAUNCHER_NAME(NOBJ, SHAPE)(c, state, plan, prog, st)
    PS_FOR_EACH_SCENE(PS_SCENE_CASE)
#undef PS_SCENE_LAUNCH
    return fail(c, PS_ERR_UNSUPPORTED, "no kernel of this scene");
}
#undef PS_SCENE_CASE

}  // extern "C"
