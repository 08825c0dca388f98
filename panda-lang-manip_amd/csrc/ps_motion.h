// ps_motion.h — the Cartesian motion primitives of panda_cartesian.py:53-145
// (move / grasp / release): the plan buffer's view, the plans of one env
// (plan_move_rows, plan_hold_rows), the arithmetic of one control step
// (motion_control_step) and the fused run kernel k_motion.  motion_kernels.hip
// instantiates k_motion once per scene, as sim_kernels.hip does k_sim_step
// (its launchers are declared with the others, ps_ctx.h); plan_kernels.hip
// holds the plan kernels and their entry points, pandasim.hip ps_motion_run.
// ps_motion_program.h runs a whole sequence of primitives on the same pieces.
#pragma once

#include "ps_env.h"

namespace {

// the plan buffer (ps_motion_plan_bytes): f64 rows, then i32 rows, of the
// state's stride; addressed as the state is (StateView::at)
struct PlanView {
    double *d;
    int32_t *n;
    int64_t stride;
    PS_D double &D(int row, int64_t i) const { return StateView::at(d + row * stride, i); }
    PS_D int32_t &I(int row, int64_t i) const { return StateView::at(n + row * stride, i); }
};

inline PlanView plan_view(const ps_ctx *c, void *plan) {
    PlanView v;
    v.stride = c->lay.stride;
    v.d = (double *)plan;
    v.n = (int32_t *)((char *)plan + (int64_t)PS_PLAN_NUM_F64_ROWS * v.stride * 8);
    return v;
}

struct Q4d {
    double x, y, z, w;
};
PS_D Q4d qmuld(Q4d a, Q4d b) {
    return Q4d{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
               a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
PS_D Q4d unit(Q4d q) {
    const double inv = 1.0 / sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Q4d{q.x * inv, q.y * inv, q.z * inv, q.w * inv};
}

// (R_start^-1 R_goal).as_rotvec() of scipy's Slerp (panda_cartesian.py:87-89):
// the relative rotation by its shortest arc (w >= 0: angle <= pi), whatever
// the two quaternions' signs
PS_D void relative_rotvec(Q4d q0, Q4d q1, double rv[3]) {
    Q4d r = qmuld(Q4d{-q0.x, -q0.y, -q0.z, q0.w}, q1);
    if (r.w < 0.0) r = Q4d{-r.x, -r.y, -r.z, -r.w};
    const double vn = sqrt(r.x * r.x + r.y * r.y + r.z * r.z);
    // angle / sin(angle / 2) -> 2 as the angle -> 0
    const double s = vn > 1e-150 ? 2.0 * atan2(vn, r.w) / vn : 2.0;
    rv[0] = r.x * s;
    rv[1] = r.y * s;
    rv[2] = r.z * s;
}

// Slerp([1, n], [R_start, R_goal])(i) = R_start exp(t rotvec), t = (i - 1) / (n - 1)
// (panda_cartesian.py:87-95, 118)
PS_D Q4d slerp_at(Q4d q0, const double rv[3], int i, int n) {
    const double t = n > 1 ? (double)(i - 1) / (double)(n - 1) : 0.0;
    const double ang = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    double sh, ch;
    sincos(0.5 * t * ang, &sh, &ch);
    const double s = ang > 1e-150 ? sh / ang : 0.5 * t;
    return qmuld(q0, Q4d{rv[0] * s, rv[1] * s, rv[2] * s, ch});
}

// num_steps of move (panda_cartesian.py:74-85, 105-114): 20 below 3 cm, else
// d // 0.015 (+ 1 when d % 0.015 > 1e-3) with numpy's float floor division
// and remainder (npy_divmod)
PS_D int move_num_steps(double d) {
    if (d < 0.03) return 20;
    const double b = 0.015;
    const double mod = fmod(d, b);
    const double div = (d - mod) / b;
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return (int)fl + (mod > 1e-3 ? 1 : 0);
}

// Panda.move up to its loop (panda_cartesian.py:98-114): the plan of env i
// from its joint positions q and its goal (goal_pos[i * 3 ..], goal_quat[i * 4
// ..]), fp64 on the f32 state (FK of link 11 and the rotation-matrix ->
// quaternion step as k_link_state); every row but done and blocked.  Returns
// num_steps.  k_plan_move and k_motion_program plan with it.
PS_D int plan_move_rows(const Scene &sc, const PlanView &pl, int64_t i, const float q[9], const float *goal_pos,
                        const float *goal_quat) {
#pragma clang fp contract(off)
    Kin k;
    fk(q, k);
    const V3 pf = k.f[11].o + sc.base;
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
    return num;
}

// Panda.grasp / release up to their loops (panda_cartesian.py:124-126,
// 139-141): 30 control steps of action (0, 0, 0, width) and the gripper's
// blocked flag; every row but done.  k_plan_hold's and k_motion_program's.
PS_D void plan_hold_rows(const Scene &sc, const PlanView &pl, int64_t i, const float q[9], const float *width,
                         int blocked) {
    Kin k;
    fk(q, k);
    const V3 pf = k.f[11].o + sc.base;
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

// The action and target orientation of control step `istep` (1-based) of env
// i's plan, from the joint positions q: move's waypoint and slerp
// (panda_cartesian.py:116-120) or grasp/release's hold with the ee link's
// current orientation (:124-145); then Cartesian set_action (:53-72, 147-176):
// the action clipped to [-1, 1], target = ee position + action[:3] with z >= 0
// (fp64, rounded once to f32 for IK), the fingers' target 0 when blocked, else
// the current width + action[3], POSITION_CONTROL defaults as set_action of
// ps_task.h.
PS_D void motion_step_target(const Scene &sc, const PlanView &pl, int64_t i, int istep, int num, int kind,
                             const Kin &k, V3 &target, Q4 &orn, float &a_width) {
#pragma clang fp contract(off)
    const V3 pf = k.f[11].o + sc.base;
    const double p[3] = {(double)pf.x, (double)pf.y, (double)pf.z};
    double a[3] = {0.0, 0.0, 0.0};
    const double w = pl.D(PS_PLAN_WIDTH, i);
    if (kind == PS_PLAN_KIND_MOVE) {
        const double m = (double)(istep < num ? istep : num);
#pragma unroll
        for (int c = 0; c < 3; c++) a[c] = (pl.D(PS_PLAN_START + c, i) + pl.D(PS_PLAN_DELTA + c, i) * m) - p[c];
        const Q4d q0 = Q4d{pl.D(PS_PLAN_Q0, i), pl.D(PS_PLAN_Q0 + 1, i), pl.D(PS_PLAN_Q0 + 2, i), pl.D(PS_PLAN_Q0 + 3, i)};
        const double rv[3] = {pl.D(PS_PLAN_ROTVEC, i), pl.D(PS_PLAN_ROTVEC + 1, i), pl.D(PS_PLAN_ROTVEC + 2, i)};
        const Q4d o = slerp_at(q0, rv, istep, num);
        orn = Q4{(float)o.x, (float)o.y, (float)o.z, (float)o.w};
    } else {
        orn = mat_to_quat(k.f[11].R);
    }
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = p[c] + fmin(fmax(a[c], -1.0), 1.0);
    if (t[2] < 0.0) t[2] = 0.0;
    target = mk((float)t[0], (float)t[1], (float)t[2]);
    a_width = (float)fmin(fmax(w, -1.0), 1.0);
}

// One control step of env i, k_motion's and k_motion_program's: the plan's
// target for step `istep` (1-based) of `num`, IK, the motor targets (kept in
// tgt), then PM_SUBSTEPS substeps (run_substeps, which carries the contact
// cache).  The plan rows are read here, at every control step (the index goes
// through an empty asm so the loads stay in the caller's loop), instead of
// occupying 28 registers through the solver.  HOLD_TARGETS (k_motion_program's
// wait segments): with `hold` the targets in tgt stand as they are, no IK.
template <int NOBJ, int SHAPE, bool HOLD_TARGETS>
PS_D void motion_control_step(const KParams &P, const PlanView &pl, int64_t i, int istep, int num, int kind,
                              bool blocked, bool hold, float q[9], float qd[9], Body *bd, const MJStore &lds,
                              float tgt[9] PS_PROF_PARAM) {
    int64_t ii = i;
    asm volatile("" : "+v"(ii));
    if (!HOLD_TARGETS || !hold) {
        Kin k;
        fk(q, k);
        V3 t;
        Q4 orn;
        float aw;
        motion_step_target(P.sc, pl, ii, istep, num, kind, k, t, orn, aw);
        float qik[9];
        inverse_kinematics<11>(q, t - P.sc.base, orn, qik);
#pragma unroll
        for (int d = 0; d < 7; d++) tgt[d] = qik[d];
        const float width = blocked ? 0.0f : (q[7] + q[8]) + aw;
        tgt[7] = tgt[8] = width * 0.5f;
    }
    run_substeps<NOBJ, SHAPE, true>(P, i, PM_SUBSTEPS, q, qd, bd, lds, true, tgt PS_PROF_ARG);
}

// What a motion kernel leaves in the state: robot, bodies, the motor targets
// of its last control step and ps_step's gains
template <int NOBJ>
PS_D void store_motion_state(const StateView &s, int64_t i, const float q[9], const float qd[9], const Body *bd,
                             const float tgt[9]) {
    {
        Motors m;
#pragma unroll
        for (int d = 0; d < 9; d++) {
            m.target[d] = tgt[d];
            m.kp[d] = (float)PM_MOTOR_KP;
            m.kd[d] = (float)PM_MOTOR_KD;
            m.vel[d] = 0.0f;
            m.imp[d] = (float)(joint_force(d) * PM_TIMESTEP);
        }
        store_motor_targets(s, i, m);
        store_motor_gains(s, i, m);
    }
    store_robot(s, i, q, qd);
#pragma unroll
    for (int b = 0; b < NOBJ; b++) store_body(s, i, b, bd[b]);
}

// ps_motion_run: up to max_steps control steps of every env whose plan has
// steps left, one env per lane.  Robot and objects are loaded once and stored
// once; per control step the plan's target, IK, the motor targets and
// PM_SUBSTEPS substeps (run_substeps, which carries the contact cache).  The
// control-step loop's trip count is the lane's own: a lane without steps left
// returns before it touches its env, and a lane that finishes early leaves the
// loop, so the wave-level numbering of the substep (robot_candidates' ballot
// of the lanes still executing, the solver's gates) sees exactly the lanes
// that still step, as it sees the lanes of a ragged last wave.
template <int NOBJ, int SHAPE>
__global__ __launch_bounds__(kBlock, 1) void k_motion(KParams P, PlanView pl, int max_steps) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int num = pl.I(PS_PLAN_NUM_STEPS, i), done = pl.I(PS_PLAN_DONE, i);
    const int left = num - done;
    const int todo = left < max_steps ? left : max_steps;
    if (todo <= 0) return;
    const int kind = pl.I(PS_PLAN_KIND, i);
    const bool blocked = pl.I(PS_PLAN_BLOCKED, i) != 0;
    const StateView &s = P.s;
    float q[9], qd[9];
    load_robot(s, i, q, qd);
    Body bd[NOBJ > 0 ? NOBJ : 1];
#pragma unroll
    for (int b = 0; b < NOBJ; b++) load_body(s, i, b, bd[b]);
    __shared__ float smem[lds_floats<NOBJ>() * kBlock];
    MJStore lds{(lds_float *)(smem + threadIdx.x), kBlock};
    lds.cwo = lds.base + CW_OUT * kBlock;
    if constexpr (NOBJ == 2) bind_stack(lds, P, i);
#ifdef PS_PROFILE_PHASES
    PhaseTimer pt;
    pt.last = (uint32_t)__builtin_amdgcn_s_memtime();
    for (int k = 0; k < PS_NUM_PROF_SLOTS; k++) pt.acc[k] = 0;
    for (int k = 0; k < PS_ITP_WORDS; k++) pt.itp[k] = 0;
#endif
    float tgt[9];
    for (int st = 0; st < todo; st++)
        motion_control_step<NOBJ, SHAPE, false>(P, pl, i, done + 1 + st, num, kind, blocked, false, q, qd, bd, lds,
                                                tgt PS_PROF_ARG);
    store_motion_state<NOBJ>(s, i, q, qd, bd, tgt);
    pl.I(PS_PLAN_DONE, i) = done + todo;
#ifdef PS_PROFILE_PHASES
    // the diagnostic build's phase counters, as k_step adds them (lane 0 of
    // the wave, when it ran steps)
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < PS_NUM_PROF_SLOTS; k++) atomicAdd(&P.prof[k], (unsigned long long)pt.acc[k]);
#endif
}

}  // namespace
