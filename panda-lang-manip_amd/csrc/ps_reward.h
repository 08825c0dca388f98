// ps_reward.h — compute_reward / is_success of one goal pair (core.py:226,
// utils.py:4-30) as ps_compute_reward evaluates it: f64 arithmetic when either
// side is f64 (numpy's promotion), f32 otherwise (the threshold rounded to
// f32).  One device function per arithmetic, shared by k_compute_reward
// (state_kernels.hip) and the replay sampler's relabelling
// (replay_kernels.hip), so a relabelled reward is ps_compute_reward's bit for
// bit.  Every operation is an explicit round-to-nearest intrinsic behind
// opaque() (ps_task_rng.h): nothing is contracted.
#pragma once

#include "ps_task_rng.h"

namespace ps {

PS_D int goal_pair_dim(int task) { return task == PS_TASK_STACK ? 6 : (task == PS_TASK_FLIP ? 4 : 3); }

PS_D double goal_pair_threshold(int task) {
    return task == PS_TASK_STACK ? PM_STACK_DISTANCE_THRESHOLD
           : task == PS_TASK_FLIP ? PM_FLIP_DISTANCE_THRESHOLD
                                  : PM_DISTANCE_THRESHOLD;
}

// the pair (a, g) of goal_pair_dim(task) values each, either side f32 or f64
PS_D void goal_pair_reward_f64(int task, int reward_type, const void *a_, int a_dbl, const void *g_, int g_dbl,
                               float &reward, bool &success) {
#pragma clang fp contract(off)
    const int gd = goal_pair_dim(task);
    const bool angle = task == PS_TASK_FLIP;
    const double thr = goal_pair_threshold(task);
    double m = 0.0;
    for (int k = 0; k < gd; k++) {
        double a = a_dbl ? ((const double *)a_)[k] : (double)((const float *)a_)[k];
        double g = g_dbl ? ((const double *)g_)[k] : (double)((const float *)g_)[k];
        double e = __dsub_rn(a, g);
        double t = angle ? opaque(__dmul_rn(a, g)) : opaque(__dmul_rn(e, e));
        m = k == 0 ? t : __dadd_rn(m, t);
    }
    double d = angle ? __dsub_rn(1.0, opaque(__dmul_rn(m, m))) : __dsqrt_rn(m);
    reward = reward_type == 0 ? (d > thr ? -1.0f : -0.0f) : -__double2float_rn(d);  // ps_task.h reward_for
    success = d < thr;
}

// both sides f32
PS_D void goal_pair_reward_f32(int task, int reward_type, const float *a, const float *g, float &reward,
                               bool &success) {
#pragma clang fp contract(off)
    const int gd = goal_pair_dim(task);
    const bool angle = task == PS_TASK_FLIP;
    const double thr = goal_pair_threshold(task);
    float m = 0.0f;
    for (int k = 0; k < gd; k++) {
        float av = a[k], gv = g[k];
        float e = __fsub_rn(av, gv);
        float t = angle ? opaque(__fmul_rn(av, gv)) : opaque(__fmul_rn(e, e));
        m = k == 0 ? t : __fadd_rn(m, t);
    }
    // correctly rounded f32 root: the f64 root rounded once
    float d = angle ? __fsub_rn(1.0f, opaque(__fmul_rn(m, m))) : __double2float_rn(__dsqrt_rn((double)m));
    float tf = (float)thr;
    reward = reward_type == 0 ? (d > tf ? -1.0f : -0.0f) : -d;
    success = d < tf;
}

}  // namespace ps
