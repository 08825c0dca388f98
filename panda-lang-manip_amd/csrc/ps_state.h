// ps_state.h — the structure-of-arrays state as the kernels see it: the
// state view (StateView), the kernel parameter block (KParams), Stack's stash
// binding and the load / store of robot, motor, body and rng rows.  Needs the
// scene records (ps_scene.h) and the rng (ps_task_rng.h), not the substep:
// the query and render units include this and nothing of the solver.
#pragma once

#include <hip/hip_runtime.h>

#include "pandasim.h"
#include "ps_scene.h"
#include "ps_task_rng.h"

using namespace ps;

namespace {

constexpr int kBlock = 64;

struct StateView {
    float *f;  // [PS_NUM_FLOAT_ROWS][stride]
    double *goal;
    uint64_t *rng;
    int32_t *elapsed;
    int64_t stride;
    // Row r of env i = a wave-uniform row base (SGPRs, rebuilt from the kernel
    // arguments by two scalar ops) plus the lane's 32-bit byte offset, which
    // the loads and stores take as `global_* v_off, s[base]`.  With a 64-bit
    // per-lane address per row the compiler kept 26 of them live from the
    // state loads at entry to the stores at exit: 208 B per lane of scratch
    // (spilled and written back to HBM every step) and AGPR copies through the
    // solver.  ps_create caps num_envs at PS_MAX_ENVS so i * 8 fits 32 bits.
    // The row base goes through an empty asm pinned to SGPRs: otherwise the
    // compiler reassociates (f + off) + row * stride back into one 64-bit
    // per-lane pointer per row.
    PS_D static uint32_t off(int64_t i, uint32_t size) { return (uint32_t)i * size; }
    // (readfirstlane first: the group kernels' divergence analysis does not
    // always see the base as uniform, and an SGPR operand needs one)
    template <class T>
    PS_D static T *pin(T *p) {
        const uint64_t u = (uint64_t)p;
        uint64_t r = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
        asm("" : "+s"(r));
        return (T *)r;
    }
    template <class T>
    PS_D static T &at(T *row_base, int64_t i) {
        return *(T *)((char *)pin(row_base) + off(i, sizeof(T)));
    }
    PS_D float &F(int row, int64_t i) const { return at(f + row * stride, i); }
    PS_D double &G(int k, int64_t i) const { return at(goal + k * stride, i); }
    PS_D uint64_t &R(int k, int64_t i) const { return at(rng + k * stride, i); }
    PS_D int32_t &E(int64_t i) const { return at(elapsed, i); }
};

struct KParams {
    StateView s;
    int64_t n;
    Scene sc;
    int reward_type, block_gripper, obs_dim, action_dim, autoreset;
    uint8_t *nonfinite;  // NaN/Inf guard output (ps_set_nonfinite_guard), NULL = off
    int reset_nonfinite;
    float *gstash;  // Stack: GSTASH_FLOATS x stride per-substep stash and pair rows (ctx scratch)
    int write_gains;  // k_step also stores the motor gain rows (ps_ctx::gains_dirty)
    float *epstats;   // ps_set_episode_stats: [4][epstride] running return, last return, last success, episodes
    int64_t epstride;
#ifdef PS_PROFILE_PHASES
    unsigned long long *prof;  // phase counters (ps_prof_buffer)
    uint32_t *itdump;          // per-env PGS iterations of the last step (ps_iter_dump_buffer)
#endif
#ifdef PS_DEBUG_ROW_DUMP
    float *dbg;  // row dump (ps_row_dump_buffer)
#endif
};

// Stack: env i's views of the global stash (ensure_stash): the stash rows
// env-minor, then its pair and gripper rows env-major, then the shared zero block
PS_D void bind_stack(MJStore &lds, const KParams &P, int64_t i) {
    const int64_t stride = P.s.stride;
    lds.gst = P.gstash;
    lds.gst_stride = stride;
    lds.goff = StateView::off(i, 4);
    lds.gpair = (__attribute__((address_space(1))) float *)(P.gstash + (int64_t)GSTASH_PAIR_OFFSET * stride +
                                                             i * (NP * PAIR_FLOATS));
    lds.ggrip = (__attribute__((address_space(1))) float *)(P.gstash + (int64_t)GSTASH_GRIP_OFFSET * stride +
                                                             i * GRIP_FLOATS);
    lds.gzero = (__attribute__((address_space(1))) float *)(P.gstash + (int64_t)GSTASH_FLOATS * stride);
}

// ------------------------------------------------------------ state I/O
PS_D void load_robot(const StateView &s, int64_t i, float q[9], float qd[9]) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        q[d] = s.F(PS_F_Q + d, i);
        qd[d] = s.F(PS_F_QD + d, i);
    }
}
PS_D void store_robot(const StateView &s, int64_t i, const float q[9], const float qd[9]) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        s.F(PS_F_Q + d, i) = q[d];
        s.F(PS_F_QD + d, i) = qd[d];
    }
}
PS_D void load_motors(const StateView &s, int64_t i, Motors &m) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        m.target[d] = s.F(PS_F_MTARGET + d, i);
        m.kp[d] = s.F(PS_F_MKP + d, i);
        m.kd[d] = s.F(PS_F_MKD + d, i);
        m.vel[d] = s.F(PS_F_MVEL + d, i);
        m.imp[d] = s.F(PS_F_MIMP + d, i);
    }
}
// The fused step's motors are POSITION_CONTROL with PyBullet's gains (kp 0.1,
// kd 1, target velocity 0) on all nine joints.  It stores the targets and max
// impulses every step (72 B per env) and the three gain rows (108 B) only when
// they may hold something else: on the first step after ps_create /
// ps_init_state, or after ps_mark_motor_rows_dirty (the plugin path's
// control_joints, a restored snapshot).  Until then they hold PyBullet's
// default velocity motors (kp 0, kd 1, k_init_state).
PS_D void store_motor_targets(const StateView &s, int64_t i, const Motors &m) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        s.F(PS_F_MTARGET + d, i) = m.target[d];
        s.F(PS_F_MIMP + d, i) = m.imp[d];
    }
}
PS_D void store_motor_gains(const StateView &s, int64_t i, const Motors &m) {
#pragma unroll
    for (int d = 0; d < 9; d++) {
        s.F(PS_F_MKP + d, i) = m.kp[d];
        s.F(PS_F_MKD + d, i) = m.kd[d];
        s.F(PS_F_MVEL + d, i) = m.vel[d];
    }
}
PS_D int body_row(int b) { return b == 0 ? PS_F_CPOS : PS_F_C2POS; }
PS_D void load_body(const StateView &s, int64_t i, int b, Body &c) {
    int r = body_row(b);
    c.pos = mk(s.F(r, i), s.F(r + 1, i), s.F(r + 2, i));
    c.quat = Q4{s.F(r + 3, i), s.F(r + 4, i), s.F(r + 5, i), s.F(r + 6, i)};
    c.vel = mk(s.F(r + 7, i), s.F(r + 8, i), s.F(r + 9, i));
    c.omg = mk(s.F(r + 10, i), s.F(r + 11, i), s.F(r + 12, i));
}
PS_D void store_body(const StateView &s, int64_t i, int b, const Body &c) {
    int r = body_row(b);
    s.F(r, i) = c.pos.x; s.F(r + 1, i) = c.pos.y; s.F(r + 2, i) = c.pos.z;
    s.F(r + 3, i) = c.quat.x; s.F(r + 4, i) = c.quat.y; s.F(r + 5, i) = c.quat.z; s.F(r + 6, i) = c.quat.w;
    s.F(r + 7, i) = c.vel.x; s.F(r + 8, i) = c.vel.y; s.F(r + 9, i) = c.vel.z;
    s.F(r + 10, i) = c.omg.x; s.F(r + 11, i) = c.omg.y; s.F(r + 12, i) = c.omg.z;
}
PS_D Pcg load_rng(const StateView &s, int64_t i) {
    return Pcg{s.R(0, i), s.R(1, i), s.R(2, i), s.R(3, i)};
}
PS_D void store_rng(const StateView &s, int64_t i, const Pcg &r) {
    s.R(0, i) = r.sh; s.R(1, i) = r.sl; s.R(2, i) = r.ih; s.R(3, i) = r.il;
}
PS_D uint64_t &aux_rng(const StateView &s, int64_t i) { return s.R(4, i); }

// a reset teleports the robot and the objects: every cached contact breaks
// (its points drift beyond the breaking threshold)
PS_D void clear_contact_cache(const StateView &s, int64_t i) {
#pragma unroll
    for (int r = PS_F_WG0; r < PS_NUM_FLOAT_ROWS; r++) s.F(r, i) = 0.0f;
}

}  // namespace
