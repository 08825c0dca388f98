// ps_step.h — the kernels that run the substep on the state: run_substeps
// (the substep loop with the contact cache, also k_motion's: ps_motion.h),
// the fused env step k_step and the plugin path's k_sim_step.  The only env
// header that needs the whole physics (ps_physics.h).  step_kernels.hip
// instantiates k_step once per (task, control) pair and sim_kernels.hip
// k_sim_step once per scene.
#pragma once

#include "ps_physics.h"
#include "ps_ctx.h"
#include "ps_task.h"

namespace {

static_assert(kBlock == CW_LANES, "robot_candidates: the work lists' output rows are kBlock lanes wide");

// The motor rows are constant over a control step.  The fused step's targets
// (its gains are PyBullet's defaults, STD_MOTORS) stay in 9 registers across
// the substeps; the plugin path's full rows (45 floats) are re-read from the
// state at every substep instead of occupying registers through the solver
// (the index goes through an empty asm so the loads stay in the loop).
// STD_MOTORS: `tgt` holds the targets set_action computed in this lane.
template <int NOBJ, int SHAPE, bool STD_MOTORS, int G = 1>
PS_D void run_substeps(const KParams &P, int64_t i, int n, float q[9], float qd[9], Body *bd,
                       const MJStore &lds, bool live, const float *tgt PS_PROF_PARAM) {
    static_assert(kBlock == 64, "WarmCache: one wave per workgroup");
    const WarmCache<G, NOBJ> wc{P.s.f + PS_F_WG0 * P.s.stride, P.s.stride, live, lds};
    wc.to_lds();
    // G > 1: the targets come back from the state rows, which every lane of
    // the group wrote with the same values (k_step); held in registers across
    // the substeps the 8-lane Slide kernel drifted from the one-lane kernel by
    // 2 cm (the lanes' dumped targets were identical: a codegen effect, not a
    // per-lane difference), through memory it is bit-identical to it
    float tgt_mem[9];
    if constexpr (G > 1) {
#pragma unroll
        for (int d = 0; d < 9; d++) tgt_mem[d] = STD_MOTORS ? P.s.F(PS_F_MTARGET + d, i) : 0.0f;
        tgt = tgt_mem;
    }
    for (int st = 0; st < n; st++) {
        int64_t ii = i;
        asm volatile("" : "+v"(ii));
        Motors m;
        if constexpr (STD_MOTORS) {
#pragma unroll
            for (int d = 0; d < 9; d++) m.target[d] = tgt[d];
        } else {
            load_motors(P.s, ii, m);
        }
#ifdef PS_DEBUG_ROW_DUMP
        // by logical block (step_block: the group kernels' XCD remap), so
        // dump lane l holds env l / G as scripts/row_dump.py reads it
        const uint64_t dl = (uint64_t)step_block<G>() * 64 + __lane_id();
        float *dump = (P.dbg && st < 2 && dl < PS_DUMP_LANES) ? P.dbg + (dl * 2 + st) * PS_DUMP_ROWS : nullptr;
#endif
        substep<NOBJ, SHAPE, STD_MOTORS, G>(P.sc, q, qd, m, bd, lds, wc PS_PROF_ARG PS_DUMP_ARG);
    }
    wc.from_lds();
}

// The fused env step: G lanes = one env = one full RobotTaskEnv.step().
// G = 1: one env per lane (large batches).  G = 16 (small batches, NOBJ <= 1):
// the 16 lanes of a group run the same setup and share the solver
// (group_pgs); lane 0 of the group writes the env's results, and the groups
// of the last wave past the batch end compute a copy of the last env and
// write nothing.  ORI: ps_step_oriented's kernel, whose IK target takes env
// i's orientation from orn [B, 4] (every lane of a group reads the same four
// floats, as it does the action); ps_step's kernels never read orn.
template <int TASK, int CONTROL, int G = 1, bool ORI = false>
__global__ __launch_bounds__(kBlock, 1) void k_step(KParams P, const float *actions, float *obs, float *ag, float *dg,
                                                    float *reward, uint8_t *terminated, uint8_t *truncated,
                                                    float *final_obs, float *final_ag, const float *orn) {
    static_assert(!ORI || CONTROL == PS_CONTROL_EE, "a target orientation exists with ee control only");
    using T = TaskTraits<TASK>;
    const int64_t gi = ((int64_t)step_block<G>() * blockDim.x + threadIdx.x) / G;
    if (G == 1 && gi >= P.n) return;
    const bool live = gi < P.n;
    const int64_t i = live ? gi : P.n - 1;
    const bool writer = G == 1 || (live && (threadIdx.x % G) == 0);
    const StateView &s = P.s;
#ifdef PS_PROFILE_PHASES
    PhaseTimer pt;
    pt.last = (uint32_t)__builtin_amdgcn_s_memtime();
    for (int k = 0; k < PS_NUM_PROF_SLOTS; k++) pt.acc[k] = 0;
    for (int k = 0; k < PS_ITP_WORDS; k++) pt.itp[k] = 0;
#endif
    float q[9], qd[9];
    load_robot(s, i, q, qd);
    Body bd[T::NOBJ > 0 ? T::NOBJ : 1];
#pragma unroll
    for (int b = 0; b < T::NOBJ; b++) load_body(s, i, b, bd[b]);
    float tgt[9];
    {
        Motors m;
        if constexpr (ORI) set_action<CONTROL, true>(P, actions + i * P.action_dim, q, m, orn + i * 4);
        else set_action<CONTROL>(P, actions + i * P.action_dim, q, m);
        // every lane of a group stores the same targets (no lane reads a value
        // only another lane wrote; run_substeps reads them back for G > 1)
        if (G > 1 || writer) store_motor_targets(s, i, m);
        if (writer && P.write_gains) store_motor_gains(s, i, m);
#pragma unroll
        for (int d = 0; d < 9; d++) tgt[d] = m.target[d];
    }
    PS_PHASE(6);
    // LDS columns: one per lane, or one per env when the group's lanes share it
    // (shared_lds<G>, then the work lists' per-lane output rows after them)
    constexpr bool SHARED = shared_lds<G>();
    constexpr int NCOL = SHARED ? kBlock / G : kBlock;
    __shared__ float smem[lds_floats<T::NOBJ>() * NCOL + (SHARED ? CW_OUT_FLOATS * kBlock : 0)];
    MJStore lds{(lds_float *)(smem + (SHARED ? threadIdx.x / G : threadIdx.x)), NCOL};
    lds.cwo = SHARED ? (lds_float *)(smem + lds_floats<T::NOBJ>() * NCOL + threadIdx.x) : lds.base + CW_OUT * kBlock;
    if constexpr (T::NOBJ == 2) bind_stack(lds, P, i);
    run_substeps<T::NOBJ, T::SHAPE, true, G>(P, i, PM_SUBSTEPS, q, qd, bd, lds, live, tgt PS_PROF_ARG);
    double g[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int d = 0; d < T::GOAL; d++) g[d] = s.G(d, i);
    float a[6];
    achieved<TASK>(P, q, qd, bd, a);
    double dist = goal_metric<TASK>(a, g);
    bool term = dist < T::THRESHOLD;
    int el = s.E(i) + 1;
    bool trunc = el >= T::STEPS;
    const float rew = reward_for(P.reward_type, dist, T::THRESHOLD);
    if (writer) {
        reward[i] = rew;
        terminated[i] = term;
        truncated[i] = trunc;
    }
    // NaN/Inf guard: a non-finite joint or object state is
    // flagged, and with reset_nonfinite the env is reset and reported truncated
    bool reset_bad = false;
    if (P.nonfinite || P.reset_nonfinite) {
        bool ok = true;
#pragma unroll
        for (int d = 0; d < 9; d++) ok = ok && isfinite(q[d]) && isfinite(qd[d]);
#pragma unroll
        for (int b = 0; b < T::NOBJ; b++)
            ok = ok && isfinite(bd[b].pos.x + bd[b].pos.y + bd[b].pos.z + bd[b].quat.x + bd[b].quat.y + bd[b].quat.z +
                                bd[b].quat.w + bd[b].vel.x + bd[b].vel.y + bd[b].vel.z + bd[b].omg.x + bd[b].omg.y +
                                bd[b].omg.z);
        if (P.nonfinite && writer) P.nonfinite[i] = !ok;
        if (!ok && P.reset_nonfinite) {
            trunc = true;
            if (writer) truncated[i] = 1;
            reset_bad = true;
        }
    }
    if ((P.autoreset && (term || trunc)) || reset_bad) {
        if (writer && (final_obs || final_ag)) write_obs<TASK>(P, i, q, qd, bd, g, final_obs, final_ag, nullptr);
        Pcg r = load_rng(s, i);
        uint64_t aux = aux_rng(s, i);
        reset_env<TASK>(q, qd, bd, g, r, aux);
        if (writer) {
            store_rng(s, i, r);
            aux_rng(s, i) = aux;
            for (int d = 0; d < T::GOAL; d++) s.G(d, i) = g[d];
            clear_contact_cache(s, i);
        }
        el = 0;
    } else if (writer && (final_obs || final_ag)) {
        write_obs<TASK>(P, i, q, qd, bd, g, final_obs, final_ag, nullptr);
    }
    if (writer && P.epstats) {
        // RecordEpisodeStatistics, fused (ps_set_episode_stats): the running
        // return of the episode, and at its end (terminated or truncated,
        // incl. the guard's reset) the finished episode's return and success
        float *e = P.epstats + i;
        const int64_t w = P.epstride;
        const float run = e[0] + rew;
        if (term || trunc) {
            e[w] = run;
            e[2 * w] = term ? 1.0f : 0.0f;
            e[3 * w] += 1.0f;
            e[0] = 0.0f;
        } else {
            e[0] = run;
        }
    }
    if (writer) {
        s.E(i) = el;
        store_robot(s, i, q, qd);
#pragma unroll
        for (int b = 0; b < T::NOBJ; b++) store_body(s, i, b, bd[b]);
        write_obs<TASK>(P, i, q, qd, bd, g, obs, ag, dg);
    }
#ifdef PS_PROFILE_PHASES
    PS_PHASE(7);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < PS_NUM_PROF_SLOTS; k++)
            atomicAdd(&P.prof[k], (unsigned long long)pt.acc[k]);
    if (G == 1 && P.itdump && i < PS_ITER_DUMP_ENVS)
        for (int k = 0; k < PS_ITP_WORDS; k++) P.itdump[(int64_t)k * PS_ITER_DUMP_ENVS + i] = pt.itp[k];
#endif
}

template <int NOBJ, int SHAPE>
__global__ __launch_bounds__(kBlock) void k_sim_step(KParams P, int n_substeps) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
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
#endif
    run_substeps<NOBJ, SHAPE, false>(P, i, n_substeps, q, qd, bd, lds, true, nullptr PS_PROF_ARG);
    store_robot(s, i, q, qd);
#pragma unroll
    for (int b = 0; b < NOBJ; b++) store_body(s, i, b, bd[b]);
}

}  // namespace
