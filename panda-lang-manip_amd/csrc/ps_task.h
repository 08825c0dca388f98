// ps_task.h — device restatement of the task layer (panda_gym tasks/*.py,
// envs/core.py, envs/robots/panda.py) on the state view: the per-task
// constants, the observation and achieved goal, the fp64 distance / success /
// reward (utils.py:4-15), the goal and object draws of a reset with Flip's
// splitmix64 goal stream, and Panda.set_action.  The random stream itself is
// ps_task_rng.h.
#pragma once

#include "ps_dynamics.h"
#include "ps_state.h"

namespace {

// Per-task constants (panda_gym/__init__.py:8-54, envs/panda_tasks.py:14-113,
// tasks/*.py): objects, shape, goal size, TimeLimit and success threshold.
template <int TASK>
struct TaskTraits {
    static constexpr int NOBJ = TASK == PS_TASK_REACH ? 0 : (TASK == PS_TASK_STACK ? 2 : 1);
    static constexpr int SHAPE = TASK == PS_TASK_SLIDE ? PS_SHAPE_CYLINDER : PS_SHAPE_BOX;
    static constexpr int GOAL = TASK == PS_TASK_STACK ? 6 : (TASK == PS_TASK_FLIP ? 4 : 3);
    static constexpr int STEPS = TASK == PS_TASK_STACK ? PM_STACK_MAX_EPISODE_STEPS : PM_MAX_EPISODE_STEPS;
    static constexpr double THRESHOLD = TASK == PS_TASK_STACK ? PM_STACK_DISTANCE_THRESHOLD
                                        : TASK == PS_TASK_FLIP ? PM_FLIP_DISTANCE_THRESHOLD
                                                               : PM_DISTANCE_THRESHOLD;
};

// ------------------------------------------------------- task layer pieces
// ee = grasptarget (link 11; COM == link frame): position and COM velocity
PS_D void ee_state(const Scene &sc, const float q[9], const float qd[9], V3 &pos, V3 &vel) {
    Kin k;
    fk(q, k);
    V3 p = k.f[11].o;
    V3 v = mk(0, 0, 0);
#pragma unroll
    for (int d = 0; d < 7; d++) v = v + cross(col(k.f[d].R, 2), p - k.f[d].o) * qd[d];
    pos = p + sc.base;
    vel = v;
}

// RobotTaskEnv._get_obs (core.py:229-238): robot obs (panda.py:109-119), the
// task obs (push.py:49-63; stack.py:65-91 both objects; flip.py:53-60 with the
// quaternion in place of Euler angles) and the achieved goal
template <int TASK>
PS_D void write_obs(const KParams &P, int64_t i, const float q[9], const float qd[9], const Body *bd,
                    const double g[6], float *obs, float *ag, float *dg) {
    using T = TaskTraits<TASK>;
    V3 p, v;
    ee_state(P.sc, q, qd, p, v);
    float o[31];
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    o[3] = v.x; o[4] = v.y; o[5] = v.z;
    int k = 6;
    if (!P.block_gripper) o[k++] = q[7] + q[8];
#pragma unroll
    for (int b = 0; b < T::NOBJ; b++) {
        const Body &cb = bd[b];
        o[k] = cb.pos.x; o[k + 1] = cb.pos.y; o[k + 2] = cb.pos.z;
        k += 3;
        if constexpr (TASK == PS_TASK_FLIP) {
            o[k] = cb.quat.x; o[k + 1] = cb.quat.y; o[k + 2] = cb.quat.z; o[k + 3] = cb.quat.w;
            k += 4;
        } else {
            V3 e = euler_from_quat(cb.quat);
            o[k] = e.x; o[k + 1] = e.y; o[k + 2] = e.z;
            k += 3;
        }
        o[k] = cb.vel.x; o[k + 1] = cb.vel.y; o[k + 2] = cb.vel.z;
        o[k + 3] = cb.omg.x; o[k + 4] = cb.omg.y; o[k + 5] = cb.omg.z;
        k += 6;
    }
    float a[6];
    if constexpr (TASK == PS_TASK_REACH) {
        a[0] = p.x; a[1] = p.y; a[2] = p.z;
    } else if constexpr (TASK == PS_TASK_FLIP) {
        a[0] = bd[0].quat.x; a[1] = bd[0].quat.y; a[2] = bd[0].quat.z; a[3] = bd[0].quat.w;
    } else {
        a[0] = bd[0].pos.x; a[1] = bd[0].pos.y; a[2] = bd[0].pos.z;
        if constexpr (T::NOBJ == 2) { a[3] = bd[1].pos.x; a[4] = bd[1].pos.y; a[5] = bd[1].pos.z; }
    }
    if (obs) {
#pragma unroll
        for (int j = 0; j < 31; j++)
            if (j < P.obs_dim) obs[i * P.obs_dim + j] = o[j];
    }
    if (ag) {
#pragma unroll
        for (int j = 0; j < T::GOAL; j++) ag[i * T::GOAL + j] = a[j];
    }
    if (dg) {
#pragma unroll
        for (int j = 0; j < T::GOAL; j++) dg[i * T::GOAL + j] = __double2float_rn(g[j]);
    }
}

// achieved goal of the stepped state (float32, as _get_obs casts it)
template <int TASK>
PS_D void achieved(const KParams &P, const float q[9], const float qd[9], const Body *bd, float a[6]) {
    if constexpr (TASK == PS_TASK_REACH) {
        V3 p, v;
        ee_state(P.sc, q, qd, p, v);
        a[0] = p.x; a[1] = p.y; a[2] = p.z;
    } else if constexpr (TASK == PS_TASK_FLIP) {
        a[0] = bd[0].quat.x; a[1] = bd[0].quat.y; a[2] = bd[0].quat.z; a[3] = bd[0].quat.w;
    } else {
        a[0] = bd[0].pos.x; a[1] = bd[0].pos.y; a[2] = bd[0].pos.z;
        if constexpr (TaskTraits<TASK>::NOBJ == 2) { a[3] = bd[1].pos.x; a[4] = bd[1].pos.y; a[5] = bd[1].pos.z; }
    }
}

// utils.distance (3 or 6 values) / utils.angle_distance (Flip) of float32
// achieved vs float64 desired, in float64 as numpy promotes
template <int TASK>
PS_D double goal_metric(const float a[6], const double g[6]) {
#pragma clang fp contract(off)
    if constexpr (TASK == PS_TASK_FLIP) {
        double dot = opaque(__dmul_rn((double)a[0], g[0]));
#pragma unroll
        for (int k = 1; k < 4; k++) dot = __dadd_rn(dot, opaque(__dmul_rn((double)a[k], g[k])));
        return __dsub_rn(1.0, opaque(__dmul_rn(dot, dot)));
    } else {
        constexpr int N = TaskTraits<TASK>::GOAL;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            double e = __dsub_rn((double)a[k], g[k]);
            double e2 = opaque(__dmul_rn(e, e));
            s = k == 0 ? e2 : __dadd_rn(s, e2);
        }
        return __dsqrt_rn(s);
    }
}

PS_D float reward_for(int reward_type, double d, double thr) {
    if (reward_type == 0) return d > thr ? -1.0f : -0.0f;
    return -__double2float_rn(d);
}

// splitmix64 stream of Flip's goal (oracle po_flip_goal): R.random()
// (flip.py:70-72) as a uniform unit quaternion by Marsaglia's method -- two
// rejection-sampled points of the unit disc, q = (x1, x2, x3 t, x4 t),
// t = sqrt((1 - s1) / s2).  Only correctly rounded +, *, / and sqrt, kept
// uncontracted, so the oracle's draws are reproduced bit for bit.
PS_D uint64_t splitmix64(uint64_t &st) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
PS_D uint64_t aux_seed(uint64_t seed) { return seed ^ 0x5851F42D4C957F2DULL; }
PS_D double aux_signed_unit(uint64_t &st) {
#pragma clang fp contract(off)
    return __dsub_rn(opaque(__dmul_rn((double)(splitmix64(st) >> 11), 2.0 / 9007199254740992.0)), 1.0);
}
PS_D double disc_point(uint64_t &st, double &x, double &y) {
#pragma clang fp contract(off)
    for (;;) {
        x = aux_signed_unit(st);
        y = aux_signed_unit(st);
        double s = __dadd_rn(opaque(__dmul_rn(x, x)), opaque(__dmul_rn(y, y)));
        if (s < 1.0 && s > 0.0) return s;
    }
}
PS_D void random_rotation(uint64_t &st, double q[4]) {
#pragma clang fp contract(off)
    double x1, x2, x3, x4;
    double s1 = disc_point(st, x1, x2);
    double s2 = disc_point(st, x3, x4);
    double t = __dsqrt_rn(__ddiv_rn(__dsub_rn(1.0, s1), s2));
    q[0] = x1;
    q[1] = x2;
    q[2] = __dmul_rn(x3, t);
    q[3] = __dmul_rn(x4, t);
}

// set_base_pose -> resetBasePositionAndOrientation (pybullet.py:427-439):
// PyBullet's init-pose command sets the base pose and, with it, zero base
// linear and angular velocity
PS_D void place(Body &b, double x, double y, double z) {
    b.pos = mk((float)x, (float)y, (float)z);
    b.quat = Q4{0.0f, 0.0f, 0.0f, 1.0f};
    b.vel = mk(0.0f, 0.0f, 0.0f);
    b.omg = mk(0.0f, 0.0f, 0.0f);
}

// Panda.reset + Task.reset (core.py:245-247): goal then object draws in the
// reference's order (reach.py:47-54, push.py:69-87, pick_and_place.py:65-85,
// slide.py:69-87, stack.py:103-116, flip.py:66-78)
template <int TASK>
PS_D void reset_env(float q[9], float qd[9], Body *bd, double g[6], Pcg &r, uint64_t &aux) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        q[d] = (float)neutral_q(d);
        qd[d] = 0.0f;
    }
    constexpr double xy = 0.3 / 2;  // goal_xy_range / 2 = obj_xy_range / 2
    if constexpr (TASK == PS_TASK_REACH) {
        g[0] = uniform(r, -xy, xy);
        g[1] = uniform(r, -xy, xy);
        g[2] = uniform(r, 0.0, 0.3);
    } else if constexpr (TASK == PS_TASK_STACK) {
        constexpr double size = PM_OBJECT_SIZE;
        double n0 = uniform(r, -xy, xy), n1 = uniform(r, -xy, xy), n2 = uniform(r, 0.0, 0.0);
        g[0] = __dadd_rn(0.0, n0);
        g[1] = __dadd_rn(0.0, n1);
        g[2] = __dadd_rn(size / 2, n2);
        g[3] = __dadd_rn(0.0, n0);
        g[4] = __dadd_rn(0.0, n1);
        g[5] = __dadd_rn(3 * size / 2, n2);
        double a0 = uniform(r, -xy, xy), a1 = uniform(r, -xy, xy), a2 = uniform(r, 0.0, 0.0);
        double b0 = uniform(r, -xy, xy), b1 = uniform(r, -xy, xy), b2 = uniform(r, 0.0, 0.0);
        place(bd[0], __dadd_rn(0.0, a0), __dadd_rn(0.0, a1), __dadd_rn(size / 2, a2));
        place(bd[1], __dadd_rn(0.0, b0), __dadd_rn(0.0, b1), __dadd_rn(3 * size / 2, b2));
    } else if constexpr (TASK == PS_TASK_FLIP) {
        random_rotation(aux, g);
        double o0 = uniform(r, -xy, xy), o1 = uniform(r, -xy, xy), o2 = uniform(r, 0.0, 0.0);
        place(bd[0], __dadd_rn(0.0, o0), __dadd_rn(0.0, o1), __dadd_rn(PM_OBJECT_SIZE / 2, o2));
    } else {
        // Push, PickAndPlace, Slide
        constexpr double size = TASK == PS_TASK_SLIDE ? PM_SLIDE_OBJECT_SIZE : PM_OBJECT_SIZE;
        constexpr double gx = TASK == PS_TASK_SLIDE ? PM_SLIDE_GOAL_X_OFFSET : 0.0;
        constexpr double zr = TASK == PS_TASK_PICK_AND_PLACE ? 0.2 : 0.0;
        double n0 = uniform(r, -xy + gx, xy + gx), n1 = uniform(r, -xy, xy), n2 = uniform(r, 0.0, zr);
        if (TASK == PS_TASK_PICK_AND_PLACE && pcg_double(r) < 0.3) n2 = 0.0;
        g[0] = __dadd_rn(0.0, n0);
        g[1] = __dadd_rn(0.0, n1);
        g[2] = __dadd_rn(size / 2, n2);
        double o0 = uniform(r, -xy, xy), o1 = uniform(r, -xy, xy), o2 = uniform(r, 0.0, 0.0);
        place(bd[0], __dadd_rn(0.0, o0), __dadd_rn(0.0, o1), __dadd_rn(size / 2, o2));
    }
}

// Panda.set_action (panda.py:52-107) -> motor targets (control_joints).
// ORI (ee control; panda_ori.py:52-99): the IK target's orientation is the
// env's quaternion orn[4] (x, y, z, w; inverse_kinematics normalises it) in
// place of the standard one, which stays a compile-time constant otherwise.
template <int CONTROL, bool ORI = false>
PS_D void set_action(const KParams &P, const float *act, const float q[9], Motors &m, const float *orn = nullptr) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = j < P.action_dim ? fminf(fmaxf(act[j], -1.0f), 1.0f) : 0.0f;
    float tq[9];
    if constexpr (CONTROL == PS_CONTROL_EE) {
        V3 p, v;
        float zero[9];
#pragma unroll
        for (int d = 0; d < 9; d++) zero[d] = 0.0f;
        ee_state(P.sc, q, zero, p, v);
        V3 t = p + mk(a[0] * 0.05f, a[1] * 0.05f, a[2] * 0.05f);
        t.z = fmaxf(0.0f, t.z);
        float qik[9];
        if constexpr (ORI)
            inverse_kinematics<11>(q, t - P.sc.base, Q4{orn[0], orn[1], orn[2], orn[3]}, qik);
        else
            inverse_kinematics<11>(q, t - P.sc.base, Q4{1.0f, 0.0f, 0.0f, 0.0f}, qik);
#pragma unroll
        for (int d = 0; d < 7; d++) tq[d] = qik[d];
    } else {
#pragma unroll
        for (int d = 0; d < 7; d++) tq[d] = q[d] + a[d] * 0.05f;
    }
    float width = 0.0f;
    if (!P.block_gripper) width = (q[7] + q[8]) + a[P.action_dim - 1] * 0.2f;
    tq[7] = tq[8] = width * 0.5f;
#pragma unroll
    for (int d = 0; d < 9; d++) {
        m.target[d] = tq[d];
        m.kp[d] = (float)PM_MOTOR_KP;
        m.kd[d] = (float)PM_MOTOR_KD;
        m.vel[d] = 0.0f;
        m.imp[d] = (float)(joint_force(d) * PM_TIMESTEP);
    }
}

}  // namespace
