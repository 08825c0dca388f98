// plan_kernels.hip — the motion primitives' plan kernels (the plan of move,
// grasp and release from the state, on ps_motion.h's plan view and fp64
// helpers) and the C ABI entry points that launch them: ps_motion_plan_bytes,
// ps_plan_move, ps_plan_grasp, ps_plan_release.  Compiled once, unlike
// motion_kernels.hip (k_motion, once per scene); ps_motion_run is pandasim.hip's.
#include "ps_motion.h"

namespace {

// ------------------------------------------------------ motion primitives
// Panda.move up to its loop (panda_cartesian.py:98-114): the plan of env i
// from its state and goal (plan_move_rows, ps_motion.h)
__global__ __launch_bounds__(kBlock) void k_plan_move(KParams P, PlanView pl, const float *goal_pos,
                                                      const float *goal_quat, const uint8_t *mask) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    pl.I(PS_PLAN_DONE, i) = 0;
    if (mask && !mask[i]) {
        pl.I(PS_PLAN_NUM_STEPS, i) = 0;
        return;
    }
    float q[9], qd[9];
    load_robot(P.s, i, q, qd);
    plan_move_rows(P.sc, pl, i, q, goal_pos, goal_quat);
}

// Panda.grasp / release up to their loops (panda_cartesian.py:124-126,
// 139-141; plan_hold_rows, ps_motion.h)
__global__ __launch_bounds__(kBlock) void k_plan_hold(KParams P, PlanView pl, const float *width, int blocked,
                                                      const uint8_t *mask) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    pl.I(PS_PLAN_DONE, i) = 0;
    if (mask && !mask[i]) {
        pl.I(PS_PLAN_NUM_STEPS, i) = 0;
        return;
    }
    float q[9], qd[9];
    load_robot(P.s, i, q, qd);
    plan_hold_rows(P.sc, pl, i, q, width, blocked);
}

}  // namespace

// ------------------------------------------------------------------- C ABI
extern "C" {

int64_t ps_motion_plan_bytes(int64_t num_envs) {
    ps_layout lay;
    if (ps_state_layout(num_envs, &lay) != PS_OK) return PS_ERR_ARG;
    return lay.stride * ((int64_t)PS_PLAN_NUM_F64_ROWS * 8 + (int64_t)PS_PLAN_NUM_I32_ROWS * 4);
}

int ps_plan_move(ps_ctx *c, const void *state, void *plan, const float *goal_pos, const float *goal_quat,
                 const uint8_t *mask, void *stream) {
    if (!c || !state || !plan || !goal_pos || !goal_quat) return fail(c, PS_ERR_ARG, "null argument");
    KParams P = params_of(c, (void *)state);
    hipLaunchKernelGGL(k_plan_move, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, plan_view(c, plan),
                       goal_pos, goal_quat, mask);
    return check_launch(c);
}

static int plan_hold(ps_ctx *c, const void *state, void *plan, const float *width, int blocked, const uint8_t *mask,
                     void *stream) {
    if (!c || !state || !plan) return fail(c, PS_ERR_ARG, "null argument");
    KParams P = params_of(c, (void *)state);
    hipLaunchKernelGGL(k_plan_hold, grid_of(P.n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, P, plan_view(c, plan),
                       width, blocked, mask);
    return check_launch(c);
}

int ps_plan_grasp(ps_ctx *c, const void *state, void *plan, const uint8_t *mask, void *stream) {
    return plan_hold(c, state, plan, nullptr, 1, mask, stream);
}

int ps_plan_release(ps_ctx *c, const void *state, void *plan, const float *width, const uint8_t *mask,
                    void *stream) {
    return plan_hold(c, state, plan, width, 0, mask, stream);
}

}  // extern "C"
