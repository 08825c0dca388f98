// ps_motion_program.h — a whole sequence of motion primitives in one launch
// (ps_motion_program): k_motion_program, on ps_motion.h's plans and control
// step.  program_kernels.hip instantiates it once per scene, as
// motion_kernels.hip does k_motion; pandasim.hip checks and packs the program.
#pragma once

#include "ps_motion.h"

namespace {

// the first segment from `from` on that env i runs (num_segments: none)
PS_D int next_segment(const ps_program_args &A, int64_t n, int64_t i, int from) {
    int s = from;
    if (A.mask)
        while (s < A.num_segments && !A.mask[(int64_t)s * n + i]) s++;
    return s;
}

// whether a move's goal can be planned: seven finite numbers, the quaternion
// not zero (its squares cannot vanish in fp64 unless every component is 0)
PS_D bool move_goal_ok(const float *goal_pos, const float *goal_quat, int64_t i) {
    bool ok = true;
    double n2 = 0.0;
    for (int c = 0; c < 3; c++) ok = ok && isfinite(goal_pos[i * 3 + c]);
    for (int c = 0; c < 4; c++) {
        const float v = goal_quat[i * 4 + c];
        ok = ok && isfinite(v);
        n2 += (double)v * (double)v;
    }
    return ok && n2 > 0.0;
}

// ps_motion_program: env i (one per lane) runs its segments one after the
// other.  One flat loop over control steps: at the top of an iteration a lane
// whose segment is exhausted starts its next one under a short divergent
// branch (it plans from the q it holds, as the plan kernels do from the
// state, or leaves the loop), then every lane still in the loop executes the
// one control-step body, motion_control_step, together.  run_substeps is
// reached from that one place only, so its wave-level numbering
// (robot_candidates' ballot of the lanes executing, the solver's gates) sees
// exactly the lanes that still step, as in k_motion; with a loop over
// segments around a loop over steps the lanes of different segments would
// pass through the substep apart.  A wave takes the largest sum of steps over
// its lanes, not the sum over segments of the largest count.
//
// A lane without a segment to run returns before it touches its env; one that
// stops before its first control step stores only completed and steps.
template <int NOBJ, int SHAPE>
__global__ __launch_bounds__(kBlock, 1) void k_motion_program(KParams P, PlanView pl, ps_program_args A) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int S = A.num_segments;
    int next = next_segment(A, P.n, i, 0);  // the segment to start when the current one is exhausted
    if (next >= S) {
        if (A.completed) A.completed[i] = S;
        if (A.steps) A.steps[i] = 0;
        return;
    }
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
    // a wait before the lane's first planned step holds the state's targets
    float tgt[9];
#pragma unroll
    for (int d = 0; d < 9; d++) tgt[d] = s.F(PS_F_MTARGET + d, i);
    int num = 0, istep = 0, steps = 0, completed = S;
    int kind = PS_PLAN_KIND_HOLD;
    bool blocked = false, hold = false;
    for (;;) {
        if (istep >= num) {
            if (next >= S) break;
            const int seg = next;
            const int sk = (int)(A.kinds >> (2 * seg)) & 3;
            blocked = (A.blocked >> seg) & 1;
            hold = sk == PS_SEG_WAIT;
            if (sk == PS_SEG_WAIT) {
                num = A.wait[seg];
            } else if (sk == PS_SEG_MOVE) {
                const float *gp = A.goal_pos + (int64_t)seg * P.n * 3, *gq = A.goal_quat + (int64_t)seg * P.n * 4;
                if (!move_goal_ok(gp, gq, i)) {
                    completed = seg;
                    break;
                }
                kind = PS_PLAN_KIND_MOVE;
                num = plan_move_rows(P.sc, pl, i, q, gp, gq);
                pl.I(PS_PLAN_BLOCKED, i) = blocked;
                pl.I(PS_PLAN_DONE, i) = num;  // the segment runs to its end in this launch
            } else {
                const float *w = sk == PS_SEG_RELEASE && A.width ? A.width + (int64_t)seg * P.n : nullptr;
                kind = PS_PLAN_KIND_HOLD;
                num = PS_PLAN_HOLD_STEPS;
                plan_hold_rows(P.sc, pl, i, q, w, blocked);
                pl.I(PS_PLAN_DONE, i) = num;
            }
            istep = 0;
            next = next_segment(A, P.n, i, seg + 1);
        }
        istep++;
        steps++;
        motion_control_step<NOBJ, SHAPE, true>(P, pl, i, istep, num, kind, blocked, hold, q, qd, bd, lds,
                                               tgt PS_PROF_ARG);
    }
    if (A.completed) A.completed[i] = completed;
    if (A.steps) A.steps[i] = steps;
    if (steps > 0) store_motion_state<NOBJ>(s, i, q, qd, bd, tgt);
#ifdef PS_PROFILE_PHASES
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < PS_NUM_PROF_SLOTS; k++) atomicAdd(&P.prof[k], (unsigned long long)pt.acc[k]);
#endif
}

}  // namespace
