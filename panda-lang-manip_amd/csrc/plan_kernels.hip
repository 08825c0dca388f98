// plan_kernels.hip — the motion primitives' plan kernels (the plan of move,
// grasp and release from the state, on ps_motion.h's plan view and fp64
// helpers) and the C ABI entry points that launch them: ps_motion_plan_bytes,
// ps_plan_move, ps_plan_grasp, ps_plan_release.  Compiled once, unlike
// motion_kernels.hip (k_motion, once per scene); ps_motion_run is pandasim.hip's.
#include "ps_motion.h"

namespace {

// ------------------------------------------------------ motion primitives
// Panda.move up to its loop (panda_cartesian.py:98-114): the plan of env i
// from its state and goal, fp64 on the f32 state (FK of link 11 and the
// rotation-matrix -> quaternion step as k_link_state)
__global__ __launch_bounds__(kBlock) void k_plan_move(KParams P, PlanView pl, const float *goal_pos,
                                                      const float *goal_quat, const uint8_t *mask) {
#pragma clang fp contract(off)
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    pl.I(PS_PLAN_DONE, i) = 0;
    if (mask && !mask[i]) {
        pl.I(PS_PLAN_NUM_STEPS, i) = 0;
        return;
    }
    float q[9], qd[9];
    load_robot(P.s, i, q, qd);
    Kin k;
    fk(q, k);
    const V3 pf = k.f[11].o + P.sc.base;
    const Q4 qf = mat_to_quat(k.f[11].R);
    const double start[3] = {(double)pf.x, (double)pf.y, (double)pf.z};
    double tot[3], d2 = 0.0;
    for (int c = 0; c < 3; c++) {
        tot[c] = (double)goal_pos[i * 3 + c] - start[c];
        d2 += tot[c] * tot[c];
    }
    const int num = move_num_steps(sqrt(d2));
    for (int c = 0; c < 3; c++) {
        pl.D(PS_PLAN_START + c, i) = start[c];
        pl.D(PS_PLAN_DELTA + c, i) = tot[c] / (double)num;
    }
    pl.D(PS_PLAN_WIDTH, i) = (double)q[7] + (double)q[8];
    const Q4d q0 = unit(Q4d{(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w});
    const Q4d q1 = unit(Q4d{(double)goal_quat[i * 4], (double)goal_quat[i * 4 + 1], (double)goal_quat[i * 4 + 2],
                            (double)goal_quat[i * 4 + 3]});
    double rv[3];
    relative_rotvec(q0, q1, rv);
    pl.D(PS_PLAN_Q0, i) = q0.x;
    pl.D(PS_PLAN_Q0 + 1, i) = q0.y;
    pl.D(PS_PLAN_Q0 + 2, i) = q0.z;
    pl.D(PS_PLAN_Q0 + 3, i) = q0.w;
    for (int c = 0; c < 3; c++) pl.D(PS_PLAN_ROTVEC + c, i) = rv[c];
    pl.I(PS_PLAN_NUM_STEPS, i) = num;
    pl.I(PS_PLAN_KIND, i) = PS_PLAN_KIND_MOVE;
}

// Panda.grasp / release up to their loops (panda_cartesian.py:124-126,
// 139-141): 30 control steps of action (0, 0, 0, width) and the gripper's
// blocked flag
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
    Kin k;
    fk(q, k);
    const V3 pf = k.f[11].o + P.sc.base;
    const Q4 qf = mat_to_quat(k.f[11].R);
    const Q4d q0 = unit(Q4d{(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w});
    pl.D(PS_PLAN_START, i) = (double)pf.x;
    pl.D(PS_PLAN_START + 1, i) = (double)pf.y;
    pl.D(PS_PLAN_START + 2, i) = (double)pf.z;
    for (int c = 0; c < 3; c++) {
        pl.D(PS_PLAN_DELTA + c, i) = 0.0;
        pl.D(PS_PLAN_ROTVEC + c, i) = 0.0;
    }
    pl.D(PS_PLAN_WIDTH, i) = width ? (double)width[i] : 1.0;
    pl.D(PS_PLAN_Q0, i) = q0.x;
    pl.D(PS_PLAN_Q0 + 1, i) = q0.y;
    pl.D(PS_PLAN_Q0 + 2, i) = q0.z;
    pl.D(PS_PLAN_Q0 + 3, i) = q0.w;
    pl.I(PS_PLAN_NUM_STEPS, i) = PS_PLAN_HOLD_STEPS;
    pl.I(PS_PLAN_BLOCKED, i) = blocked;
    pl.I(PS_PLAN_KIND, i) = PS_PLAN_KIND_HOLD;
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
