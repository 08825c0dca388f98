// ps_substep.h — substep(): one btMultiBodyDynamicsWorld::stepSimulation(1/500 s)
// of an env, still one function: geometry and M, free velocities, row setup
// (joint rows, ground / pair / gripper contacts), the one-lane solve (or
// group_pgs), cache write-back, integration.
#pragma once

#include "ps_collide.h"
#include "ps_dynamics.h"
#include "ps_solver.h"
#include "ps_solver_group.h"

namespace ps {

// ---- substep's macros, undefined at the end of this header.  They expand to
// locals of substep(): PS_COUNT_IT to prof_it (diagnostic build), PS_REGATE to
// the gates gate_lim, gate_pair, gate_robot, gate_ground[] and the extent NB.
// PGS iterations run, for the diagnostic build's counters
#ifdef PS_PROFILE_PHASES
#define PS_COUNT_IT() prof_it++
#else
#define PS_COUNT_IT() do {} while (0)
#endif
// The gates are wave-uniform SGPR values.  Hoisted out of the PGS loop,
// whose exit is per lane, their bit tests become lane masks that are
// rebuilt against exec at every gated row (a v_cndmask + v_cmp pair
// each); redefining them at the top of each half-iteration (an empty asm
// with an "s" operand) keeps the tests scalar, inside the loop.
#define PS_REGATE()                                                                        \
    do {                                                                                   \
        asm volatile("" : "+s"(gate_lim), "+s"(gate_pair), "+s"(gate_robot));              \
        for (int b_ = 0; b_ < NB; b_++) asm volatile("" : "+s"(gate_ground[b_]));         \
    } while (0)

// Joint d's limit on one side (0: lower, 1: upper) at coordinate qd_: the
// penetration, the row's sign, whether the row is on, and whether it takes
// its position error in the velocity row (combined) or as a split impulse.
struct LimitSide {
    float pen, sgn;
    bool on, combined;
    // the split-impulse position correction of a row that is on and not combined
    PS_D float split() const { return sgn * (-pen) * (float)PM_SPLIT_LIMIT_ERP; }
};
PS_D LimitSide limit_side(int d, int side, float qd_) {
    // the limit as fp32 head + tail (lo = lo_h + lo_t): q - lo_h is
    // exact near the limit, so the row switches where the fp64 limit
    // puts it (a joint pressed onto -3.0718 by its motor sits exactly
    // at fp32(-3.0718) = -3.0717999935, 6.5e-9 inside the double
    // limit: on with the fp32 constant, off in Bullet and the oracle)
    // (folded to constants: the callers' loops are unrolled)
    const double LO = dof_def(d).lo, HI = dof_def(d).hi;
    const float lo_h = (float)LO, lo_t = (float)(LO - (double)lo_h);
    const float hi_h = (float)HI, hi_t = (float)(HI - (double)hi_h);
    LimitSide s;
    s.pen = side ? (hi_h - qd_) + hi_t : (qd_ - lo_h) - lo_t;
    s.sgn = side ? -1.0f : 1.0f;
    s.on = s.pen <= 0.0f;
    s.combined = s.pen > (float)PM_SPLIT_PENETRATION_THRESHOLD;
    return s;
}

// The split-impulse position correction of joint d's limit rows: a function
// of q alone, so Stack rebuilds it after the solve instead of keeping 9 stash
// rows per substep.
PS_D float split_of(int d, float qd_) {
    float split = 0.0f;
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const LimitSide s = limit_side(d, side, qd_);
        if (s.on && !s.combined) split += s.split();
    }
    return split;
}

// ----------------------------------------------------------------- substep
// One btMultiBodyDynamicsWorld::stepSimulation(1/500 s): see the oracle's
// po_substep for the row-by-row restatement this mirrors.
// STD_MOTORS: the motors are the ones RobotTaskEnv.step sets (POSITION_CONTROL
// on all nine joints with the fixed Panda gains and forces, panda.py:40-56), so
// only the targets are per-env; otherwise every gain comes from `mt`.
template <int NOBJ, int SHAPE, bool STD_MOTORS, int G = 1>
PS_D void substep(const Scene &sc, float q[9], float qd[9], const Motors &mt, Body *bd, const MJStore &lds,
                  const WarmCache<G, NOBJ> &wc PS_PROF_PARAM PS_DUMP_PARAM) {
    static_assert(NOBJ >= 0 && NOBJ <= 2, "objects");
    static_assert(NOBJ < 2 || SHAPE == SHAPE_BOX, "Stack stacks cubes");
    constexpr int NB = NOBJ > 0 ? NOBJ : 1;  // array extents
    constexpr bool ANISO = SHAPE == SHAPE_CYL;
    constexpr bool CHUNKED = chunked_lds<NOBJ, G>();  // the gripper rows' M^-1 J^T as 16-byte chunks
    const float dt = (float)PM_TIMESTEP;
    float Mi[45], hb[9];
    Geo geo;
    // phases are fenced so the scheduler does not interleave them (each one's
    // transient state is large; overlapping them is what spilled to scratch)
    bias_forces(q, qd, hb);
    PS_PHASE(0);
    __builtin_amdgcn_sched_barrier(0);
    {
        Kin k;
        fk(q, k);
        static_for<0, 9>([&](auto D) {
            constexpr int d = decltype(D)::value;
            geo.ax[d] = dof_axis<d>(k);
            if constexpr (d < 7) geo.org[d] = k.f[d].o;
        });
        geo.hR = k.f[8].R;  // links 9 and 10 carry the hand's rotation
        static_for<0, PM_NUM_BOXES>([&](auto BB) {
            constexpr int B = decltype(BB)::value;
            constexpr BoxDef b = box_def(B);
            geo.bc[B] = k.f[b.link].o + mul(k.f[b.link].R, mk((float)b.c[0], (float)b.c[1], (float)b.c[2])) + sc.base;
        });
        {
            constexpr SphereDef w = wrist_def();
            geo.wc = k.f[w.link].o + mul(k.f[w.link].R, mk((float)w.c[0], (float)w.c[1], (float)w.c[2])) + sc.base;
        }
        mass_matrix(k, Mi);
    }
#ifdef PS_PROFILE_PHASES
    // (diagnostic build: M and M^-1 are forced out where their phases end;
    // the product sinks them into the candidate code)
#pragma unroll
    for (int k = 0; k < 45; k++) asm volatile("" ::"v"(Mi[k]));
#endif
    PS_PHASE(1);
    __builtin_amdgcn_sched_barrier(0);
    spd_inverse(Mi);
#ifdef PS_PROFILE_PHASES
#pragma unroll
    for (int k = 0; k < 45; k++) asm volatile("" ::"v"(Mi[k]));
#endif
    PS_PHASE(2);
    __builtin_amdgcn_sched_barrier(0);
    // gripper contact candidates: geometry only, so they are found here, where
    // few registers are live, and wait in LDS (robot_candidates)
    int nr;
    {
        M3 oR[NB];
#pragma unroll
        for (int b = 0; b < NB; b++) oR[b] = NOBJ > 0 ? quat_to_mat(bd[b].quat) : M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
        nr = robot_candidates<NOBJ, SHAPE, G>(sc, geo, bd, oR, lds PS_PROF_ARG);
    }
    PS_PHASE(17);
    __builtin_amdgcn_sched_barrier(0);
    // M^-1 for the joint rows stays in registers: re-reading it from LDS in
    // every PGS iteration exposed the LDS latency once per motor row (Push
    // 4.56 -> 3.99 ms, Reach 2.97 -> 1.98 ms per step of 65 536 envs).
    float v1[9];
#pragma unroll
    for (int a = 0; a < 9; a++) {
        float s = 0.0f;
#pragma unroll
        for (int b = 0; b < 9; b++) s -= Mi[sidx(a, b)] * hb[b];
        v1[a] = qd[a] + dt * s;
    }
    // objects: gravity + btMultiBody base damping, plus the gyroscopic torque
    // -w x (I w) for the (anisotropic) cylinder
    V3 cw1[NB], cv1[NB];
    BodyDyn<SHAPE> od[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        cw1[b] = mk(0, 0, 0);
        cv1[b] = mk(0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < NOBJ; b++) {
        od[b] = body_dyn<SHAPE>(sc, bd[b], b == 0 ? sc.mass : sc.mass2);
        float cl = (float)PM_LINEAR_DAMPING + (float)PM_LINEAR_DAMPING * norm(bd[b].vel);
        float ca = (float)PM_ANGULAR_DAMPING + (float)PM_ANGULAR_DAMPING * norm(bd[b].omg);
        cv1[b] = bd[b].vel + (mk(0, 0, (float)PM_GRAVITY_Z) - bd[b].vel * cl) * dt;
        cw1[b] = bd[b].omg - bd[b].omg * (ca * dt);
        if constexpr (ANISO) {
            V3 I = local_inertia<SHAPE>(sc, b == 0 ? sc.mass : sc.mass2);
            S3 Iw = rotate_diag(od[b].R, I.x, I.y, I.z);
            V3 gyro = od[b].inv_inertia(cross(bd[b].omg, mul(Iw, bd[b].omg)));
            cw1[b] = cw1[b] - gyro * dt;
        }
    }

    // ---- joint-space rows: limits and motors.  A joint can be beyond at most
    // one of its limits, so each joint carries one limit row whose side is a
    // bit of lim_up; rows that are off have bounds [0, 0] and are exact no-ops.
    float dinvj[9];
    float lim_rhs[9], lim_lam[9];
    unsigned lim_on = 0u, lim_up = 0u;
    float split_dq[9];
    float mot_rhs[9], mot_lam[9];
#pragma unroll
    for (int d = 0; d < 9; d++) {
        float den = Mi[sidx(d, d)];
        dinvj[d] = safe_inv(den);
        split_dq[d] = 0.0f;
        lim_rhs[d] = 0.0f;
        lim_lam[d] = 0.0f;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const LimitSide s = limit_side(d, side, q[d]);
            float velerr = -s.sgn * v1[d];
            float poserr = -s.pen * (float)PM_ERP * PS_INV_DT;
            if (s.on) {
                lim_on |= 1u << d;
                lim_up |= side ? 1u << d : 0u;
                lim_rhs[d] = (s.combined ? poserr + velerr : velerr) * dinvj[d];
                if (!s.combined) split_dq[d] += s.split();
            }
        }
        float kp = STD_MOTORS ? (float)PM_MOTOR_KP : mt.kp[d], kd = STD_MOTORS ? (float)PM_MOTOR_KD : mt.kd[d];
        float vel = STD_MOTORS ? 0.0f : mt.vel[d];
        float target = kp * (mt.target[d] - q[d]) * PS_INV_DT + v1[d] + kd * (vel - v1[d]);
        mot_rhs[d] = (target - v1[d]) * dinvj[d];
        mot_lam[d] = 0.0f;
    }

    PS_PHASE(16);
    // ---- contacts (oracle gen_contacts order: ground per object, pairs, gripper)
    GroundContact gc[NB][NG];
    int ng[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        ng[b] = 0;
#pragma unroll
        for (int s = 0; s < NG; s++)
            gc[b][s] = GroundContact{mk(0, 0, 0), {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, 0};
    }
    const float gmu = sc.fric * (float)PM_DEFAULT_FRICTION;
    if constexpr (NOBJ == 2) {
        // unused LDS ground rows must be all-zero no-ops
#pragma unroll
        for (int c = 0; c < 2 * NG; c++)
#pragma unroll
            for (int k = 0; k < LDS_GND_FLOATS; k++) lds.gnd(c, k) = 0.0f;
    }
    const float warm = (float)PM_WARMSTART_FACTOR;
#pragma unroll
    for (int b = 0; b < NOBJ; b++) {
        // the previous substep's ground contacts of this object (ids = 1 +
        // support point, packed 5 bits per slot)
        const int grow = b == 0 ? PS_F_WG0 : PS_F_WG1;
        float plam[NG];
#pragma unroll
        for (int k = 0; k < NG; k++) plam[k] = wc.load(grow + k);
        const unsigned pid = (unsigned)wc.load(grow + NG);
        static_for<0, num_support<SHAPE>()>([&](auto VV) {
            constexpr int V = decltype(VV)::value;
            V3 pw = bd[b].pos + mul(od[b].R, support_point<SHAPE, V>(sc));
            float top;
            if (ng[b] < NG && ground_top(sc, pw.x, pw.y, top)) {
                float dist = pw.z - top;
                if (dist < (float)PM_CONTACT_MARGIN_GROUND) {
                    V3 r = pw - bd[b].pos;
                    // normal (0,0,1), t1 (0,-1,0), t2 (1,0,0)
                    V3 dirs[3] = {mk(0, 0, 1), mk(0, -1, 0), mk(1, 0, 0)};
                    GroundContact g;
                    g.r = r;
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        V3 rn = cross(r, dirs[j]);
                        V3 w = od[b].inv_inertia(rn);
                        float den = dot(rn, w) + dot(dirs[j], dirs[j]) * od[b].inv_m;
                        g.dinv[j] = NOBJ == 2 ? cube_ground_dinv(r, j, od[b].iI, od[b].inv_m) : safe_inv(den);
                        float rel = dot(rn, cw1[b]) + dot(dirs[j], cv1[b]);
                        g.lam[j] = 0.0f;
                        g.rhs[j] = j == 0 ? normal_rhs(dist, rel, g.dinv[0]) : -rel * g.dinv[j];
                    }
                    g.lam[0] = warm * cache_lookup(plam, pid, V + 1);
                    g.id = V + 1;
                    if (NOBJ == 2) {
                        // Stack: the cubes' read-only ground-row data live in LDS
                        const int at = b * NG + ng[b];
                        lds.gnd(at, 0) = g.r.x; lds.gnd(at, 1) = g.r.y; lds.gnd(at, 2) = g.r.z;
#pragma unroll
                        for (int j = 0; j < 3; j++) lds.gnd(at, 3 + j) = g.rhs[j];
#pragma unroll
                        for (int s = 0; s < NG; s++)
                            if (s == ng[b]) {
                                gc[b][s].lam[0] = g.lam[0];
                                gc[b][s].id = g.id;
                            }
                    } else {
#pragma unroll
                        for (int s = 0; s < NG; s++)
                            if (s == ng[b]) gc[b][s] = g;
                    }
                    ng[b]++;
                }
            }
        });
        // the new ids are packed from the slots after the loop (packing inside
        // it, by a shift of 5 * ng[b], turned the select into compile-time
        // slots into a dynamic index and gc[][] into scratch)
        unsigned nid = 0u;
#pragma unroll
        for (int k = 0; k < NG; k++) nid |= (unsigned)gc[b][k].id << (5 * k);
        wc.store(grow + NG, (float)nid);
    }
    PairContact pc[NP];
    int np = 0;
    if constexpr (NOBJ == 2) {
        PairCand cand[NP];
        np = box_box(sc, bd[0], bd[1], od[0].R, od[1].R, cand);
        // the previous substep's pair contacts: points in object 1's frame,
        // matched by distance (btPersistentManifold::getCacheEntry)
        float pl[NP];
        V3 ppt[NP];
        const int pn = (int)wc.load(PS_F_WPN);
#pragma unroll
        for (int k = 0; k < NP; k++) {
            pl[k] = wc.load(PS_F_WP + k);
            ppt[k] = mk(wc.load(PS_F_WPPT + 3 * k), wc.load(PS_F_WPPT + 3 * k + 1), wc.load(PS_F_WPPT + 3 * k + 2));
        }
#pragma unroll
        for (int c = 0; c < NP; c++) {
            PairContact &p = pc[c];
            if (c < np) {
                const PairCand &cd = cand[c];
                int A = cd.a0 ? 0 : 1;
                V3 dirs[3];
                dirs[0] = cd.n;
                plane_space(cd.n, dirs[1], dirs[2]);
                V3 rA = cd.pA - (A == 0 ? bd[0].pos : bd[1].pos), rB = cd.pB - (A == 0 ? bd[1].pos : bd[0].pos);
                p.a0 = cd.a0;
                p.rA = A == 0 ? rA : rB;  // stored by object index: offset from object 0's COM
                p.rB = A == 0 ? rB : rA;  // and from object 1's
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    V3 dj = dirs[j];
                    p.dir[j] = dj;
                    const V3 rnA = cross(rA, dj), rnB = cross(rB, dj);
                    float iIA = A == 0 ? od[0].iI : od[1].iI, iIB = A == 0 ? od[1].iI : od[0].iI;
                    float imA = A == 0 ? od[0].inv_m : od[1].inv_m, imB = A == 0 ? od[1].inv_m : od[0].inv_m;
                    float den = dot(rnA, rnA) * iIA + dot(rnB, rnB) * iIB + dot(dj, dj) * (imA + imB);
                    p.dinv[j] = safe_inv(den);
                    V3 wA = A == 0 ? cw1[0] : cw1[1], vA = A == 0 ? cv1[0] : cv1[1];
                    V3 wB = A == 0 ? cw1[1] : cw1[0], vB = A == 0 ? cv1[1] : cv1[0];
                    float rel = dot(rnA, wA) + dot(dj, vA) - dot(rnB, wB) - dot(dj, vB);
                    p.lam[j] = 0.0f;
                    p.rhs[j] = j == 0 ? normal_rhs(cd.dist, rel, p.dinv[0]) : -rel * p.dinv[j];
                }
                V3 lp = tmul(od[0].R, cd.pB - bd[0].pos);
                float best = (float)(PM_CONTACT_BREAKING_THRESHOLD * PM_CONTACT_BREAKING_THRESHOLD), l0 = 0.0f;
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    V3 d = ppt[k] - lp;
                    float d2 = dot(d, d);
                    bool hit = k < pn && d2 < best;
                    best = hit ? d2 : best;
                    l0 = hit ? pl[k] : l0;
                }
                p.lam[0] = warm * l0;
                wc.store(PS_F_WPPT + 3 * c, lp.x);
                wc.store(PS_F_WPPT + 3 * c + 1, lp.y);
                wc.store(PS_F_WPPT + 3 * c + 2, lp.z);
            } else {
                p.a0 = true;
                p.rA = p.rB = mk(0, 0, 0);
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    p.dir[j] = mk(0, 0, 0);
                    p.rhs[j] = p.lam[j] = p.dinv[j] = 0.0f;
                }
            }
            // the read-only part of the row goes to the global stash
            // (PAIR_FLOATS); the slots this env does not use are not written
            // (the solver reads the zero block for them: MJStore::pair_rows)
            if (c < np) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    lds.pair(c, 3 * j + 0) = p.dir[j].x; lds.pair(c, 3 * j + 1) = p.dir[j].y; lds.pair(c, 3 * j + 2) = p.dir[j].z;
                    lds.pair(c, 15 + j) = p.rhs[j];
                    lds.pair(c, 18 + j) = p.dinv[j];
                }
                lds.pair(c, 9) = p.rA.x; lds.pair(c, 10) = p.rA.y; lds.pair(c, 11) = p.rA.z;
                lds.pair(c, 12) = p.rB.x; lds.pair(c, 13) = p.rB.y; lds.pair(c, 14) = p.rB.z;
            }
        }
        wc.store(PS_F_WPN, (float)np);
    }
    RobotContact rc[NR];
    {
        PS_PHASE(18);
        // 2) rows of each used slot: J (registers), M^-1 J^T (LDS), rhs, bounds;
        //    the normal starts from the cached impulse of the same feature
        float prl[NR];
#pragma unroll
        for (int k = 0; k < NR; k++) prl[k] = wc.load(PS_F_WR + k);
        const unsigned prid = (unsigned)wc.load(PS_F_WRID);
        unsigned nrid = 0u;
#pragma unroll
        for (int sl = 0; sl < NR; sl++) {
            RobotContact &c = rc[sl];
            // Chunked rows (MJStore::chunk) land in other lanes' columns, in rows
            // [28 sl, 28 sl + 28): below every record still unread (slot s's
            // record starts at row 52 + 14 s), but slot 2's rows cover its own
            // record's first rows.  So every lane reads the slot's record before
            // any lane writes the slot's rows, whichever side of the branch
            // below the wave runs first (one wave: its LDS accesses keep the
            // program's order)
            RobotCand cd0{};
            if constexpr (CHUNKED) {
                cd0 = RobotCand::load(lds, sl);
                __builtin_amdgcn_wave_barrier();
            }
            float mjc[LDS_CHUNK_FLOATS] = {};
            if (sl < nr) {
                const RobotCand cd = CHUNKED ? cd0 : RobotCand::load(lds, sl);
                V3 dirs[3];
                dirs[0] = cd.n;
                plane_space(cd.n, dirs[1], dirs[2]);
                c.mu = cd.mu;
                c.o1 = cd.obj == 1;
                bool on_obj = NOBJ > 0 && cd.obj >= 0;
                V3 p = cd.pA - sc.base;
                V3 opos = NOBJ == 2 && cd.obj == 1 ? bd[NB - 1].pos : bd[0].pos;
                V3 rB = cd.pB - opos;
                V3 ow = NOBJ == 2 && cd.obj == 1 ? cw1[NB - 1] : cw1[0];
                V3 ov = NOBJ == 2 && cd.obj == 1 ? cv1[NB - 1] : cv1[0];
                float oim = NOBJ == 2 && cd.obj == 1 ? od[NB - 1].inv_m : od[0].inv_m;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    V3 dj = dirs[j];
#pragma unroll
                    for (int D = 0; D < 7; D++) c.J[j][D] = dot(geo.ax[D], cross(p - geo.org[D], dj));
                    c.J[j][7] = cd.link == 9 ? dot(geo.ax[7], dj) : 0.0f;
                    c.J[j][8] = cd.link == 10 ? dot(geo.ax[8], dj) : 0.0f;
                    float den = 0.0f;
#pragma unroll
                    for (int a = 0; a < 9; a++) {
                        float s = 0.0f;
#pragma unroll
                        for (int b = 0; b < 9; b++) s += Mi[sidx(a, b)] * c.J[j][b];
                        if constexpr (CHUNKED) mjc[a < 8 ? 8 * j + a : 24 + j] = s;
                        else lds.at(sl, j, a) = NOBJ == 2 ? c.J[j][a] : s;  // Stack: J (M^-1 J^T rebuilt in the loop)
                        if constexpr (NOBJ == 2)
                            if (j == 0) lds.grip(sl, a) = s;
                        den += c.J[j][a] * s;
                    }
                    if constexpr (CHUNKED) {
                        // the row's DoFs 0..7, 16 bytes at a time (DoF 8 goes with chunk 6)
                        lds.chunk(sl, 2 * j) = (f32x4){mjc[8 * j], mjc[8 * j + 1], mjc[8 * j + 2], mjc[8 * j + 3]};
                        lds.chunk(sl, 2 * j + 1) = (f32x4){mjc[8 * j + 4], mjc[8 * j + 5], mjc[8 * j + 6], mjc[8 * j + 7]};
                    }
                    float rel = jrow_dot(c.J[j], v1);
                    c.rn[j] = on_obj ? cross(rB, dj) : mk(0, 0, 0);
                    c.dir[j] = on_obj ? dj : mk(0, 0, 0);  // object side only
                    if constexpr (NOBJ > 0) {
                        V3 w = ANISO ? od[0].inv_inertia(c.rn[j])
                                     : c.rn[j] * (NOBJ == 2 && cd.obj == 1 ? od[NB - 1].iI : od[0].iI);
                        if (on_obj) {
                            den += dot(c.rn[j], w) + dot(dj, dj) * oim;
                            rel -= dot(c.rn[j], ow) + dot(dj, ov);
                        }
                    }
                    c.dinv[j] = safe_inv(den);
                    c.lam[j] = 0.0f;
                    c.rhs[j] = j == 0 ? normal_rhs(cd.dist, rel, c.dinv[0]) : -rel * c.dinv[j];
                }
                if constexpr (CHUNKED) lds.chunk(sl, 6) = (f32x4){mjc[24], mjc[25], mjc[26], 0.0f};
                c.lam[0] = warm * cache_lookup(prl, prid, (unsigned)cd.id);
                nrid |= (unsigned)cd.id << (5 * sl);
            } else {
                // unused slot: all-zero rows (finite M^-1 J^T too) are no-ops in PGS
                c.mu = 0.0f;
                c.o1 = false;
#pragma unroll
                for (int j = 0; j < 3; j++) {
#pragma unroll
                    for (int a = 0; a < 9; a++) {
                        c.J[j][a] = 0.0f;
                        if constexpr (!CHUNKED)
                            lds.at(sl, j, a) = 0.0f;  // (Stack's grip rows: MJStore::grip_rows reads the zero block)
                    }
                    c.dir[j] = c.rn[j] = mk(0, 0, 0);
                    c.rhs[j] = c.lam[j] = c.dinv[j] = 0.0f;
                }
                if constexpr (CHUNKED) {
#pragma unroll
                    for (int k = 0; k < LDS_CHUNKS; k++) lds.chunk(sl, k) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                }
            }
        }
        wc.store(PS_F_WRID, (float)nrid);
    }
    PS_PHASE(3);
    __builtin_amdgcn_sched_barrier(0);
    // per-substep values the solver never reads wait outside the registers:
    // in LDS, or (Stack, whose LDS holds its ground rows) in the global stash
    // (Stack's global stash and the chunked layout's LDS stash have no
    // split-impulse rows, 18..26: split_of rebuilds them from q after the
    // solve, and the rows above shift down)
    constexpr bool SPLIT_REBUILT = NOBJ == 2 || CHUNKED;
    auto gk = [](int k) { return SPLIT_REBUILT && k >= 27 ? k - 9 : k; };
    auto put = [&](int k, float v) {
        if constexpr (NOBJ == 2) lds.gstash(gk(k)) = v;
        else if constexpr (CHUNKED) lds.stash1(gk(k)) = v;
        else lds.stash(k) = v;
    };
    auto get = [&](const MJStore &S, int k) -> float {
        if constexpr (NOBJ == 2) return S.gstash(gk(k));
        else if constexpr (CHUNKED) return S.stash1(gk(k));
        else return S.stash(k);
    };
#pragma unroll
    for (int d = 0; d < 9; d++) {
        put(d, q[d]);
        put(9 + d, v1[d]);
        if constexpr (!SPLIT_REBUILT) put(18 + d, split_dq[d]);
    }
    if constexpr (NOBJ > 0) {
        put(27, cw1[0].x); put(28, cw1[0].y); put(29, cw1[0].z);
        put(30, cv1[0].x); put(31, cv1[0].y); put(32, cv1[0].z);
        put(33, bd[0].pos.x); put(34, bd[0].pos.y); put(35, bd[0].pos.z);
        put(36, bd[0].quat.x); put(37, bd[0].quat.y); put(38, bd[0].quat.z); put(39, bd[0].quat.w);
    }
    if constexpr (NOBJ == 2) {
        put(40, cw1[1].x); put(41, cw1[1].y); put(42, cw1[1].z);
        put(43, cv1[1].x); put(44, cv1[1].y); put(45, cv1[1].z);
        put(46, bd[1].pos.x); put(47, bd[1].pos.y); put(48, bd[1].pos.z);
        put(49, bd[1].quat.x); put(50, bd[1].quat.y); put(51, bd[1].quat.z); put(52, bd[1].quat.w);
    }

    // ---- projected Gauss-Seidel
    // Every row kind is gated by a wave-uniform ballot (a scalar branch: the
    // block runs if any lane of the wave needs it); inside, lanes without the
    // row hold all-zero data or [0, 0] bounds, which leave every impulse and
    // velocity untouched, so no per-lane exec masking or phi copies remain.
    float dv[9];
#pragma unroll
    for (int d = 0; d < 9; d++) dv[d] = 0.0f;
    V3 dw[NB], dvl[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        dw[b] = mk(0, 0, 0);
        dvl[b] = mk(0, 0, 0);
    }
    float res;
    MJStore L = lds;

    // Row-family gates, fixed for the whole solve: bit k is set when some lane
    // of the wave has that row.  Taken at the solver's entry (full exec) and
    // made wave-uniform, so each gate in the loop is a scalar test and branch;
    // a ballot inside the loop is re-masked by the lanes still iterating and
    // costs two VALU instructions per row.  Lanes that have converged are
    // masked off inside a block either way, so the results do not change.
    auto wave_bits = [&](auto pred, int n) {
        unsigned m = 0u;
        for (int k = 0; k < n; k++) m |= __builtin_amdgcn_ballot_w64(pred(k)) ? 1u << k : 0u;
        return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
    };
    unsigned gate_lim = wave_bits([&](int d) { return ((lim_on >> d) & 1u) != 0u; }, 9);
    unsigned gate_ground[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) gate_ground[b] = wave_bits([&](int c) { return c < ng[b]; }, NG);
    unsigned gate_pair = wave_bits([&](int c) { return c < np; }, NP);
    unsigned gate_robot = wave_bits([&](int c) { return c < nr; }, NR);

#ifdef PS_PROFILE_PHASES
    int prof_it = 0;
#endif
    // the solver stops when every row's violation (row_viol, joint_viol) is <= 0
    static_assert(PM_SOLVER_ITERATIONS % 2 == 0, "iteration pairs");
    if constexpr (G == 1) {
        VelChange dvv;
#pragma unroll
        for (int k = 0; k < 4; k++) dvv.p[k] = (f32x2){0.0f, 0.0f};
        dvv.z = 0.0f;
        // dv += M^-1 e_d f: rows a >= d of column d (its lower part, which no
        // other column pairs) as v_pk_fma_f32 over the aligned dv pairs (2k,
        // 2k + 1), the rest as v_fma_f32 -- the same fused products
        auto mcol_apply = [&](int d, float f) {
            const int a0 = (d + 1) & ~1;  // first even row >= d
#pragma unroll
            for (int a = 0; a < 9; a++)
                if (a < a0 || a == 8) dvv.s(a, fmaf(Mi[sidx(a, d)], f, dvv.g(a)));
#pragma unroll
            for (int a = a0; a < 8; a += 2)
                dvv.p[a >> 1] = __builtin_elementwise_fma((f32x2){Mi[sidx(a, d)], Mi[sidx(a + 1, d)]}, (f32x2){f, f},
                                                          dvv.p[a >> 1]);
        };
        auto joint_row = [&](int d, float sgn, float rhs, float &lam, float lo, float hi) {
            float dl = rhs - dinvj[d] * (sgn * dvv.g(d));
            float nl = clamp_impulse(lam + dl, lo, hi);
            dl = nl - lam;
            lam = nl;
            mcol_apply(d, sgn * dl);
            res = res_max(res, joint_viol(dl, Mi[sidx(d, d)]));
        };
        auto limit_row = [&](int d) {
            if (PS_GATE(gate_lim & (1u << d), 0)) {
                float sgn = (lim_up >> d) & 1u ? -1.0f : 1.0f;
                float hi = (lim_on >> d) & 1u ? (float)PM_LIMIT_MAX_IMPULSE : 0.0f;
                joint_row(d, sgn, lim_rhs[d], lim_lam[d], 0.0f, hi);
            }
        };
        auto motor_row = [&](int d) {
            float imp = STD_MOTORS ? (float)(joint_force(d) * PM_TIMESTEP) : mt.imp[d];
            joint_row(d, 1.0f, mot_rhs[d], mot_lam[d], -imp, imp);
        };
        // body-side velocity change of object `o1 ? 1 : 0` (Stack selects; the
        // other scenes have one object and the select folds away)
        auto obj_add = [&](bool o1, V3 ddw, V3 ddv) {
            if constexpr (NOBJ == 2) {
                // a 0/1 weight per object: one FMA per component instead of a
                // select and an add
                const float s1 = o1 ? 1.0f : 0.0f, s0 = o1 ? 0.0f : 1.0f;
                dw[0] = fma3(ddw, s0, dw[0]);
                dvl[0] = fma3(ddv, s0, dvl[0]);
                dw[NB - 1] = fma3(ddw, s1, dw[NB - 1]);
                dvl[NB - 1] = fma3(ddv, s1, dvl[NB - 1]);
            } else {
                dw[0] = dw[0] + ddw;
                dvl[0] = dvl[0] + ddv;
            }
        };
        auto obj_dw = [&](bool o1) { return NOBJ == 2 && o1 ? dw[NB - 1] : dw[0]; };
        auto obj_dv = [&](bool o1) { return NOBJ == 2 && o1 ? dvl[NB - 1] : dvl[0]; };
        // Stack pair rows in the objects' own frame: with rn0 = r0 x d, rn1 = r1 x d
        // the row velocity is sg * pair_rel (sg = +1 when body A is object 0), and
        // an impulse dl on A moves object 0 by +sg dl and object 1 by -sg dl
        auto pair_rel = [&](V3 rn0, V3 rn1, V3 d) {
            return dot(rn0, dw[0]) + dot(d, dvl[0]) - dot(rn1, dw[NB - 1]) - dot(d, dvl[NB - 1]);
        };
        auto pair_apply = [&](V3 rn0, V3 rn1, V3 d, float sdl) {
            dw[0] = pk_fma3(rn0, sdl * od[0].iI, dw[0]);
            dvl[0] = pk_fma3(d, sdl * od[0].inv_m, dvl[0]);
            dw[NB - 1] = pk_fma3(rn1, -sdl * od[NB - 1].iI, dw[NB - 1]);
            dvl[NB - 1] = pk_fma3(d, -sdl * od[NB - 1].inv_m, dvl[NB - 1]);
        };

        // Stack keeps the gripper rows' J, not M^-1 J^T, in LDS: the warm start and
        // the friction rows apply dv += M^-1 g for the generalized impulse g (J^T
        // dl, or both friction rows' J^T dl summed: one product with the M^-1
        // registers per contact and sweep); the normal rows read their M^-1 J^T
        // from the global stash (GRIP_MJ_SLOTS)
        auto mi_apply = [&](const float g[9]) {
            // column by column: each dv[a] still takes b = 0..8 in order (the
            // same bits as a row-by-row product), with the columns' lower parts
            // packed (mcol_apply)
#pragma unroll
            for (int b = 0; b < 9; b++) mcol_apply(b, g[b]);
        };

        // ---- warm start: the normals that matched a cached contact start from
        // 0.85 x its impulse, applied to the velocity change before the first
        // iteration (btMultiBodyConstraintSolver::setupMultiBodyContactConstraint);
        // lanes without a cache hit carry lam = 0, a no-op
        {
            MJStore W = lds.opaque();
#pragma unroll
            for (int b = 0; b < NOBJ; b++)
#pragma unroll
                for (int c = 0; c < NG; c++)
                    if (PS_GATE(gate_ground[b] & (1u << c), 1)) {
                        const float l0 = gc[b][c].lam[0];
                        V3 gr = gc[b][c].r;
                        if (NOBJ == 2) {
                            const int at = b * NG + c;
                            gr = mk(W.gnd(at, 0), W.gnd(at, 1), W.gnd(at, 2));
                        }
                        dw[b] = dw[b] + od[b].inv_inertia(mk(gr.y * l0, -gr.x * l0, 0.0f));
                        dvl[b].z = fmaf(l0, od[b].inv_m, dvl[b].z);
                    }
            if constexpr (NOBJ == 2) {
#pragma unroll
                for (int c = 0; c < NP; c++)
                    if (gate_pair & (1u << c)) {
                        const auto *pr = W.pair_rows(c, np);
                        auto pv = [&](int k) { return mk(pr[k], pr[k + 1], pr[k + 2]); };
                        const float sl = pc[c].a0 ? pc[c].lam[0] : -pc[c].lam[0];
                        const V3 d0 = pv(0);
                        pair_apply(cross(pv(9), d0), cross(pv(12), d0), d0, sl);
                    }
            }
#pragma unroll
            for (int c = 0; c < NR; c++)
                if (PS_GATE(gate_robot & (1u << c), c < 2)) {
                    const RobotContact &r = rc[c];
                    const float l0 = r.lam[0];
                    float Jl[9];
#pragma unroll
                    for (int a = 0; a < 9; a++) Jl[a] = NOBJ == 2 ? (float)W.at(c, 0, a) : r.J[0][a];
                    if constexpr (NOBJ == 2) {
                        float g[9];
#pragma unroll
                        for (int a = 0; a < 9; a++) g[a] = Jl[a] * l0;
                        mi_apply(g);
                    } else {
                        float w[9];
                        if constexpr (CHUNKED) W.chunk_row(c, 0, w);
                        else {
#pragma unroll
                            for (int a = 0; a < 9; a++) w[a] = W.at(c, 0, a);
                        }
#pragma unroll
                        for (int a = 0; a < 9; a++) dvv.s(a, fmaf(w[a], l0, dvv.g(a)));
                    }
                    if constexpr (NOBJ > 0) {
                        float im = NOBJ == 2 && r.o1 ? od[NB - 1].inv_m : od[0].inv_m;
                        V3 ddw = ANISO ? od[0].inv_inertia(r.rn[0] * -l0)
                                       : r.rn[0] * (-l0 * (NOBJ == 2 && r.o1 ? od[NB - 1].iI : od[0].iI));
                        obj_add(r.o1, ddw, r.dir[0] * (-l0 * im));
                    }
                }
        }

        float gmj[GRIP_MJ_SLOTS][9];  // Stack: see object_normals
        auto object_normals = [&]() {
            if constexpr (NOBJ == 2) {
                // Stack: the cubes' ground normals and the pair normals touch only
                // the cubes' DoFs, so they commute with the joint rows and run right
                // after the motor rows, ungated for the ground (a slot a lane lacks
                // has 1/den = 0: an exact no-op).  The pair rows' read-only data come from the global stash
                // (PAIR_FLOATS).  Every slot's loads are issued here, before the
                // ground rows, so their L2 latency runs under those rows and the wave
                // waits once per sweep, not once per contact (unused slots hold
                // all-zero rows).
                float pf[NP][11];
                if constexpr (NOBJ == 2) {
                    if (gate_pair) {
#pragma unroll
                        for (int c = 0; c < NP; c++) {
                            const auto *pr = L.pair_rows(c, np);
#pragma unroll
                            for (int k = 0; k < 3; k++) {
                                pf[c][k] = pr[k];
                                pf[c][3 + k] = pr[9 + k];
                                pf[c][6 + k] = pr[12 + k];
                            }
                            pf[c][9] = pr[15];
                            pf[c][10] = pr[18];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    {
                        // the gripper normal rows' M^-1 J^T, loaded here so the L2
                        // latency runs under the ground rows
#pragma unroll
                        for (int c = 0; c < GRIP_MJ_SLOTS; c++)
                            if (gate_robot & (1u << c)) {
                                const auto *gr = L.grip_rows(c, nr);
#pragma unroll
                                for (int k = 0; k < 9; k++) gmj[c][k] = gr[k];
                            }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
                for (int b = 0; b < NOBJ; b++) {
                    const float inv_m = od[b].inv_m;
#pragma unroll
                    for (int c = 0; c < NG; c++) {
                        GroundContact &g = gc[b][c];
                        V3 gr = g.r;
                        float grhs = g.rhs[0], gdinv = g.dinv[0];
                        if (NOBJ == 2) {  // Stack: row data in LDS
                            const int at = b * NG + c;
                            gr = mk(L.gnd(at, 0), L.gnd(at, 1), L.gnd(at, 2));
                            grhs = L.gnd(at, 3);
                            // a slot this env does not have (the gate is the wave's) gets
                            // 1/den = 0, so its rows stay exact no-ops: with the zeroed
                            // offset alone, 1/den would be the cube's mass and the row
                            // would push back on any downward velocity change
                            gdinv = c < ng[b] ? cube_ground_dinv(gr, 0, od[b].iI, inv_m) : 0.0f;
                        }
                        V3 rn = mk(gr.y, -gr.x, 0.0f);  // r x (0,0,1); zero terms dropped below
                        float dl = grhs - gdinv * (rn.x * dw[b].x + rn.y * dw[b].y + dvl[b].z);
                        float nl = clamp_impulse(g.lam[0] + dl, 0.0f, (float)PM_CONTACT_UPPER);
                        dl = nl - g.lam[0];
                        g.lam[0] = nl;
                        if constexpr (ANISO) {
                            // I^-1 (r x n) dl rebuilt here: 9 FMAs instead of 3 registers per row
                            dw[b] = dw[b] + od[b].inv_inertia(mk(rn.x * dl, rn.y * dl, 0.0f));
                        } else {
                            float dI = dl * od[b].iI;
                            dw[b].x = fmaf(rn.x, dI, dw[b].x);
                            dw[b].y = fmaf(rn.y, dI, dw[b].y);
                        }
                        dvl[b].z = fmaf(dl, inv_m, dvl[b].z);
                        res = res_max(res, row_viol(dl, gdinv));
                    }
                }
                if constexpr (NOBJ == 2) {
                    if (gate_pair) {
#pragma unroll
                        for (int c = 0; c < NP; c++)
                            if (gate_pair & (1u << c)) {
                                PairContact &p = pc[c];
                                const float sg = p.a0 ? 1.0f : -1.0f;  // A = object 0: +1
                                const V3 d0 = mk(pf[c][0], pf[c][1], pf[c][2]);
                                const V3 rn0 = cross(mk(pf[c][3], pf[c][4], pf[c][5]), d0);
                                const V3 rn1 = cross(mk(pf[c][6], pf[c][7], pf[c][8]), d0);
                                float jv = sg * pair_rel(rn0, rn1, d0);
                                float dl = pf[c][9] - pf[c][10] * jv;
                                float nl = clamp_impulse(p.lam[0] + dl, 0.0f, (float)PM_CONTACT_UPPER);
                                dl = nl - p.lam[0];
                                p.lam[0] = nl;
                                pair_apply(rn0, rn1, d0, sg * dl);
                                res = res_max(res, row_viol(dl, pf[c][10]));
                            }
                    }
                }
            }
        };
        auto contacts = [&]() {
            // normals: the gripper contacts (the objects' ground and pair
            // normals ran with the motor rows: ground_normals, object_normals)
#pragma unroll
            for (int c = 0; c < NR; c++)
                if (PS_GATE(gate_robot & (1u << c), c < 2)) {
                    RobotContact &r = rc[c];
                    // M^-1 J^T column first: its LDS latency hides under the dot
                    float mj[9], Jl[9];
#pragma unroll
                    for (int a = 0; a < 9; a++) Jl[a] = NOBJ == 2 ? (float)L.at(c, 0, a) : r.J[0][a];
                    if constexpr (CHUNKED) {
                        L.chunk_row(c, 0, mj);  // three ds_read_b128
                    } else if constexpr (NOBJ != 2) {
#pragma unroll
                        for (int a = 0; a < 9; a++) mj[a] = L.at(c, 0, a);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    float jv = dvv.dot(Jl);
                    if (NOBJ > 0) jv -= dot(r.rn[0], obj_dw(r.o1)) + dot(r.dir[0], obj_dv(r.o1));
                    float dl = r.rhs[0] - r.dinv[0] * jv;
                    float nl = clamp_impulse(r.lam[0] + dl, 0.0f, (float)PM_CONTACT_UPPER);
                    dl = nl - r.lam[0];
                    r.lam[0] = nl;
                    if constexpr (NOBJ == 2) {
                        dvv.apply(gmj[c], dl);
                    } else {
                        dvv.apply(mj, dl);
                    }
                    if constexpr (NOBJ == 1) {
                        // one object: fma straight into its velocity change
                        dw[0] = ANISO ? dw[0] + od[0].inv_inertia_pk(r.rn[0] * -dl) : pk_fma3(r.rn[0], -dl * od[0].iI, dw[0]);
                        dvl[0] = pk_fma3(r.dir[0], -dl * od[0].inv_m, dvl[0]);
                    } else if constexpr (NOBJ == 2) {
                        float im = r.o1 ? od[NB - 1].inv_m : od[0].inv_m;
                        float iI = r.o1 ? od[NB - 1].iI : od[0].iI;
                        obj_add(r.o1, r.rn[0] * (-dl * iI), r.dir[0] * (-dl * im));
                    }
                    res = res_max(res, row_viol(dl, r.dinv[0]));
                }
            // friction cones (Stack: the pair rows' loads first, as above)
            float pq[NP][16];
            if constexpr (NOBJ == 2) {
                if (gate_pair) {
#pragma unroll
                    for (int c = 0; c < NP; c++) {
                        const auto *pr = L.pair_rows(c, np);
#pragma unroll
                        for (int k = 0; k < 12; k++) pq[c][k] = pr[3 + k];  // d1, d2, r0, r1
                        pq[c][12] = pr[16];
                        pq[c][13] = pr[17];
                        pq[c][14] = pr[19];
                        pq[c][15] = pr[20];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

#pragma unroll
            for (int b = 0; b < NOBJ; b++) {
                const float inv_m = od[b].inv_m;
#pragma unroll
                for (int c = 0; c < NG; c++)
                    if (PS_GATE(gate_ground[b] & (1u << c), 1)) {
                        GroundContact &g = gc[b][c];
                        V3 gr = g.r;
                        float grhs1 = g.rhs[1], grhs2 = g.rhs[2], gdinv1 = g.dinv[1], gdinv2 = g.dinv[2];
                        if (NOBJ == 2) {  // Stack: row data in LDS
                            const int at = b * NG + c;
                            gr = mk(L.gnd(at, 0), L.gnd(at, 1), L.gnd(at, 2));
                            grhs1 = L.gnd(at, 4);
                            grhs2 = L.gnd(at, 5);
                            const bool on = c < ng[b];  // as in the normal sweep
                            gdinv1 = on ? cube_ground_dinv(gr, 1, od[b].iI, inv_m) : 0.0f;
                            gdinv2 = on ? cube_ground_dinv(gr, 2, od[b].iI, inv_m) : 0.0f;
                        }
                        // The two friction rows (directions (0,-1,0) and (1,0,0), so
                        // r x dir = (r.z, 0, -r.x) and (0, r.z, -r.y)) side by side
                        // as f32x2 (v_pk_mul/fma/add_f32): the operations the scalar
                        // rows compiled to, fused where they were fused, so the same
                        // bits; x = row a, y = row b.
                        float dla, dlb;
                        {
#pragma clang fp contract(off)
                            const f32x2 gz = {gr.z, gr.z};
                            const f32x2 t = (f32x2){gr.x, gr.y} * (f32x2){dw[b].z, dw[b].z};
                            const f32x2 u = __builtin_elementwise_fma(gz, (f32x2){dw[b].x, dw[b].y}, -t);
                            const f32x2 w = u + (f32x2){-dvl[b].y, dvl[b].x};
                            const f32x2 lam12 = {g.lam[1], g.lam[2]};
                            const f32x2 s2 = lam12 + __builtin_elementwise_fma(-(f32x2){gdinv1, gdinv2}, w,
                                                                               (f32x2){grhs1, grhs2});
                            const float lim = gmu * g.lam[0];  // >= 0: the normal row's clamp
                            // |f|^2 as each kernel's scalar rows contracted it (the
                            // one-object kernels fused row b's square, Stack's row a's);
                            // |f| > mu N: project onto the cone (lim * rsq(m2) <= 1 there)
                            const float m2 = NOBJ == 2 ? fmaf(s2.x, s2.x, s2.y * s2.y) : fmaf(s2.y, s2.y, s2.x * s2.x);
                            const float sc2 = cone_scale(m2, lim);
                            const f32x2 dl2 = __builtin_elementwise_fma(s2, (f32x2){sc2, sc2}, -lam12);
                            const f32x2 nl2 = s2 * (f32x2){sc2, sc2};
                            g.lam[1] = nl2.x;
                            g.lam[2] = nl2.y;
                            dla = dl2.x;
                            dlb = dl2.y;
                            if constexpr (ANISO) {
                                // I^-1 (r1 dla + r2 dlb)
                                const f32x2 zab = gz * dl2;
                                dw[b] = dw[b] + od[b].inv_inertia_pk_unfused(mk(zab.x, zab.y, fmaf(-gr.x, dla, -gr.y * dlb)));
                            } else {
                                const f32x2 ab = dl2 * (f32x2){od[b].iI, od[b].iI};
                                const f32x2 wxy = __builtin_elementwise_fma(gz, ab, (f32x2){dw[b].x, dw[b].y});
                                dw[b].z = fmaf(-gr.y, ab.y, fmaf(-gr.x, ab.x, dw[b].z));
                                dw[b].x = wxy.x;
                                dw[b].y = wxy.y;
                            }
                            const f32x2 vxy = __builtin_elementwise_fma((f32x2){dlb, -dla}, (f32x2){inv_m, inv_m},
                                                                        (f32x2){dvl[b].x, dvl[b].y});
                            dvl[b].x = vxy.x;
                            dvl[b].y = vxy.y;
                        }
                        res = res_max(res, res_max(row_viol(dla, gdinv1), row_viol(dlb, gdinv2)));
                    }
            }
            if constexpr (NOBJ == 2) {
                const float pmu = sc.fric * sc.fric;
                if (gate_pair) {
#pragma unroll
                    for (int c = 0; c < NP; c++)
                        if (gate_pair & (1u << c)) {
                            PairContact &p = pc[c];
                            auto pv = [&](int k) { return mk(pq[c][k], pq[c][k + 1], pq[c][k + 2]); };
                            const float sg = p.a0 ? 1.0f : -1.0f;
                            const V3 d1 = pv(0), d2 = pv(3), r0 = pv(6), r1 = pv(9);
                            const V3 rn01 = cross(r0, d1), rn02 = cross(r0, d2), rn11 = cross(r1, d1), rn12 = cross(r1, d2);
                            float ja = sg * pair_rel(rn01, rn11, d1);
                            float jb = sg * pair_rel(rn02, rn12, d2);
                            float dla = pq[c][12] - pq[c][14] * ja, dlb = pq[c][13] - pq[c][15] * jb;
                            float sa = p.lam[1] + dla, sb = p.lam[2] + dlb;
                            float lim = pmu * p.lam[0];
                            float m2 = sa * sa + sb * sb;
                            float s = cone_scale(m2, lim);
                            sa *= s;
                            sb *= s;
                            dla = sa - p.lam[1];
                            dlb = sb - p.lam[2];
                            p.lam[1] = sa;
                            p.lam[2] = sb;
                            pair_apply(rn01, rn11, d1, sg * dla);
                            pair_apply(rn02, rn12, d2, sg * dlb);
                            res = res_max(res, res_max(row_viol(dla, pq[c][14]), row_viol(dlb, pq[c][15])));
                        }
                }
            }
#pragma unroll
            for (int c = 0; c < NR; c++)
                if (PS_GATE(gate_robot & (1u << c), c < 2)) {
                    RobotContact &r = rc[c];
                    float mj1[9], mj2[9], J1[9], J2[9];
#pragma unroll
                    for (int a = 0; a < 9; a++) {
                        J1[a] = NOBJ == 2 ? (float)L.at(c, 1, a) : r.J[1][a];
                        J2[a] = NOBJ == 2 ? (float)L.at(c, 2, a) : r.J[2][a];
                    }
                    if constexpr (CHUNKED) {
                        L.chunk_rows12(c, mj1, mj2);  // five ds_read_b128
                    } else if constexpr (NOBJ != 2) {
#pragma unroll
                        for (int a = 0; a < 9; a++) {
                            mj1[a] = L.at(c, 1, a);
                            mj2[a] = L.at(c, 2, a);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    float ja, jb;
                    if constexpr (NOBJ != 2) {
                        // the two rows' dot products side by side: (J1_a, J2_a) x
                        // (dv_a, dv_a), each lane the scalar chain's FMAs
#pragma clang fp contract(off)
                        f32x2 j2 = {0.0f, 0.0f};
#pragma unroll
                        for (int a = 0; a < 9; a++) j2 = __builtin_elementwise_fma((f32x2){J1[a], J2[a]}, dvv.bc(a), j2);
                        ja = j2.x;
                        jb = j2.y;
                    } else {
                        ja = dvv.dot(J1);
                        jb = dvv.dot(J2);
                    }
                    if (NOBJ > 0) {
                        V3 ow = obj_dw(r.o1), ov = obj_dv(r.o1);
                        ja -= dot(r.rn[1], ow) + dot(r.dir[1], ov);
                        jb -= dot(r.rn[2], ow) + dot(r.dir[2], ov);
                    }
                    float dla, dlb;
                    if constexpr (NOBJ != 2) {
                        // from the two rows' velocities on, the rows side by side as
                        // f32x2 (v_pk_*) with the scalar rows' operations and
                        // fusions (the same bits); the object's dot products above
                        // stay scalar (pairing rn[1] with rn[2] would fight
                        // pk_fma3's (x, y) pairs of the same registers)
#pragma clang fp contract(off)
                        const f32x2 lam12 = {r.lam[1], r.lam[2]};
                        const f32x2 s2 = lam12 + __builtin_elementwise_fma(-(f32x2){r.dinv[1], r.dinv[2]}, (f32x2){ja, jb},
                                                                           (f32x2){r.rhs[1], r.rhs[2]});
                        const float lim = r.mu * r.lam[0];  // >= 0: the normal row's clamp
                        const float sc2 = cone_scale(fmaf(s2.x, s2.x, s2.y * s2.y), lim);
                        const f32x2 dl2 = __builtin_elementwise_fma(s2, (f32x2){sc2, sc2}, -lam12);
                        const f32x2 nl2 = s2 * (f32x2){sc2, sc2};
                        r.lam[1] = nl2.x;
                        r.lam[2] = nl2.y;
                        dla = dl2.x;
                        dlb = dl2.y;
                    } else {
                        dla = r.rhs[1] - r.dinv[1] * ja;
                        dlb = r.rhs[2] - r.dinv[2] * jb;
                        float sa = r.lam[1] + dla, sb = r.lam[2] + dlb;
                        const float lim = r.mu * r.lam[0];  // >= 0: the normal row's clamp
                        const float m2 = sa * sa + sb * sb;
                        const float s = cone_scale(m2, lim);
                        sa *= s;
                        sb *= s;
                        dla = sa - r.lam[1];
                        dlb = sb - r.lam[2];
                        r.lam[1] = sa;
                        r.lam[2] = sb;
                    }
                    if constexpr (NOBJ == 2) {
                        float g[9];
#pragma unroll
                        for (int a = 0; a < 9; a++) g[a] = fmaf(J2[a], dlb, J1[a] * dla);
                        mi_apply(g);
                    } else {
                        dvv.apply(mj1, dla);
                        dvv.apply(mj2, dlb);
                    }
                    if constexpr (NOBJ == 1) {
                        if constexpr (ANISO) {
                            dw[0] = dw[0] + od[0].inv_inertia_pk(fma3(r.rn[2], -dlb, r.rn[1] * -dla));
                        } else {
                            float aI = -dla * od[0].iI, bI = -dlb * od[0].iI;
                            dw[0] = pk_fma3(r.rn[2], bI, pk_fma3(r.rn[1], aI, dw[0]));
                        }
                        float am = -dla * od[0].inv_m, bm = -dlb * od[0].inv_m;
                        dvl[0] = pk_fma3(r.dir[2], bm, pk_fma3(r.dir[1], am, dvl[0]));
                    } else if constexpr (NOBJ == 2) {
                        float im = r.o1 ? od[NB - 1].inv_m : od[0].inv_m;
                        // two objects are cubes (isotropic inverse inertia)
                        float iI = r.o1 ? od[NB - 1].iI : od[0].iI;
                        float aI = -dla * iI, bI = -dlb * iI;
                        V3 ddw = mk(fmaf(r.rn[2].x, bI, r.rn[1].x * aI), fmaf(r.rn[2].y, bI, r.rn[1].y * aI),
                                    fmaf(r.rn[2].z, bI, r.rn[1].z * aI));
                        float am = -dla * im, bm = -dlb * im;
                        V3 ddv = mk(fmaf(r.dir[2].x, bm, r.dir[1].x * am), fmaf(r.dir[2].y, bm, r.dir[1].y * am),
                                    fmaf(r.dir[2].z, bm, r.dir[1].z * am));
                        obj_add(r.o1, ddw, ddv);
                    }
                    res = res_max(res, res_max(row_viol(dla, r.dinv[1]), row_viol(dlb, r.dinv[2])));
                }
        };

        // One object (not Stack): its ground normals touch only the object's
        // DoFs and commute with the joint rows, so they run ungated in the motor
        // rows' block (a slot a lane lacks is an all-zero no-op) -- Bullet's
        // order up to commuting rows
        auto ground_normals = [&]() {
            if constexpr (NOBJ == 1) {
#pragma unroll
                for (int c = 0; c < NG; c++) {
                    GroundContact &g = gc[0][c];
                    const V3 rn = mk(g.r.y, -g.r.x, 0.0f);  // r x (0,0,1)
                    float dl = g.rhs[0] - g.dinv[0] * (rn.x * dw[0].x + rn.y * dw[0].y + dvl[0].z);
                    const float nl = clamp_impulse(g.lam[0] + dl, 0.0f, (float)PM_CONTACT_UPPER);
                    dl = nl - g.lam[0];
                    g.lam[0] = nl;
                    if constexpr (ANISO) {
                        dw[0] = dw[0] + od[0].inv_inertia_pk(mk(rn.x * dl, rn.y * dl, 0.0f));
                    } else {
                        const float dI = dl * od[0].iI;
                        dw[0].x = fmaf(rn.x, dI, dw[0].x);
                        dw[0].y = fmaf(rn.y, dI, dw[0].y);
                    }
                    dvl[0].z = fmaf(dl, od[0].inv_m, dvl[0].z);
                    res = res_max(res, row_viol(dl, g.dinv[0]));
                }
            }
        };

        // btSequentialImpulseConstraintSolver alternates the order of the
        // non-contact rows by iteration parity: even iterations run them in
        // reverse (motors 8..0, then limits 8..0), odd ones forward (limits 0..8,
        // then motors 0..8).  The loop is unrolled by two so both orders are
        // straight-line code; each env still stops at its own residual.
        for (int it = 0; it < PM_SOLVER_ITERATIONS; it += 2) {
            PS_COUNT_IT();
            L = lds.opaque();
            res = 0.0f;
            PS_REGATE();
            // one object: M^-1 enters each iteration pair in VGPRs (an empty asm
            // with a "v" operand), else the allocator parks it in AGPRs and
            // every motor row reads its column back (v_accvgpr_read): the PGS
            // loop's AGPR reads 442 -> 340 per iteration pair, Push 3.03 ->
            // 3.01 ms (profiles/r03h_variants_pin.log; Reach, no object, got
            // slower and keeps the allocator's choice)
            if constexpr (NOBJ == 1) {
#pragma unroll
                for (int k = 0; k < 45; k++) asm volatile("" : "+v"(Mi[k]));
            }
#pragma unroll
            for (int d = 8; d >= 0; d--) motor_row(d);
            ground_normals();
            object_normals();
            if (PS_GATE(gate_lim != 0u, 0)) {
#pragma unroll
                for (int d = 8; d >= 0; d--) limit_row(d);
            }
            contacts();
            if (res <= 0.0f) break;
            PS_COUNT_IT();
            L = lds.opaque();
            res = 0.0f;
            PS_REGATE();
            if (PS_GATE(gate_lim != 0u, 0)) {
#pragma unroll
                for (int d = 0; d < 9; d++) limit_row(d);
            }
#pragma unroll
            for (int d = 0; d < 9; d++) motor_row(d);
            ground_normals();
            object_normals();
            contacts();
            if (res <= 0.0f) break;
        }
#pragma unroll
        for (int a = 0; a < 9; a++) dv[a] = dvv.g(a);
    } else {
        group_pgs<NOBJ, SHAPE, STD_MOTORS, G>(mt, Mi, lds, gate_lim, lim_up, lim_on, gate_ground[0], gate_robot,
                                              dinvj, lim_rhs, lim_lam, mot_rhs, mot_lam, gc[0], rc, od[0], gmu,
                                              dv, dw[0], dvl[0] PS_PROF_COUNT_ARG PS_DUMP_ARG);
    }

    // the contacts' final normal impulses become the cache of the next
    // substep (solveGroupCacheFriendlyFinish writes m_appliedImpulse back)
#pragma unroll
    for (int b = 0; b < NOBJ; b++)
#pragma unroll
        for (int c = 0; c < NG; c++) wc.store((b == 0 ? PS_F_WG0 : PS_F_WG1) + c, gc[b][c].lam[0]);
    if constexpr (NOBJ == 2) {
#pragma unroll
        for (int c = 0; c < NP; c++) wc.store(PS_F_WP + c, pc[c].lam[0]);
    }
#pragma unroll
    for (int c = 0; c < NR; c++) wc.store(PS_F_WR + c, rc[c].lam[0]);

    PS_PHASE(4);
#ifdef PS_PROFILE_PHASES
    {
        int wmax = prof_it, wnr = nr;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            wmax = max(wmax, __shfl_xor(wmax, o));
            wnr = max(wnr, __shfl_xor(wnr, o));
        }
        pt.acc[8] += prof_it;
        pt.acc[9] += wmax;
#pragma unroll
        for (int k = PS_ITP_WORDS - 1; k > 0; k--) pt.itp[k] = (pt.itp[k] << 16) | (pt.itp[k - 1] >> 16);
        pt.itp[0] = (pt.itp[0] << 16) | (uint32_t)min(prof_it, 255) | ((uint32_t)nr << 8) | ((uint32_t)np << 11);
        pt.acc[10] += 1;
        pt.acc[11] += wnr;
        // the wave's open row gates (wave-uniform: every lane adds the same)
        unsigned ngnd = 0;
        for (int b = 0; b < NB; b++) ngnd += __builtin_popcount(gate_ground[b]);
        pt.acc[12] += __builtin_popcount(gate_pair);
        pt.acc[13] += ngnd;
        pt.acc[14] += __builtin_popcount(gate_robot);
        pt.acc[15] += gate_lim != 0u;
    }
#endif
    {
        // reload through an opaque address: no store-to-load forwarding, so
        // the registers really were free during the solve
        MJStore S = lds.opaque();
#pragma unroll
        for (int d = 0; d < 9; d++) {
            q[d] = get(S, d);
            v1[d] = get(S, 9 + d);
            split_dq[d] = SPLIT_REBUILT ? split_of(d, q[d]) : get(S, 18 + d);
        }
        if constexpr (NOBJ > 0) {
            cw1[0] = mk(get(S, 27), get(S, 28), get(S, 29));
            cv1[0] = mk(get(S, 30), get(S, 31), get(S, 32));
            bd[0].pos = mk(get(S, 33), get(S, 34), get(S, 35));
            bd[0].quat = Q4{get(S, 36), get(S, 37), get(S, 38), get(S, 39)};
        }
        if constexpr (NOBJ == 2) {
            cw1[1] = mk(get(S, 40), get(S, 41), get(S, 42));
            cv1[1] = mk(get(S, 43), get(S, 44), get(S, 45));
            bd[1].pos = mk(get(S, 46), get(S, 47), get(S, 48));
            bd[1].quat = Q4{get(S, 49), get(S, 50), get(S, 51), get(S, 52)};
        }
    }
    // ---- integrate (btMultiBody::stepPositionsMultiDof)
#pragma unroll
    for (int d = 0; d < 9; d++) {
        qd[d] = v1[d] + dv[d];
        q[d] += dt * qd[d] + split_dq[d];
    }
#pragma unroll
    for (int b = 0; b < NOBJ; b++) {
        Body &cb = bd[b];
        cb.omg = cw1[b] + dw[b];
        cb.vel = cv1[b] + dvl[b];
        cb.pos = cb.pos + cb.vel * dt;
        float ang = norm(cb.omg);
        if (ang * dt > 0.5f * 1.5707963267948966f) ang = 0.5f * 1.5707963267948966f / dt;
        float f = ang < 0.001f ? (0.5f * dt - (dt * dt * dt) * 0.020833333333f * ang * ang) : sinf(0.5f * ang * dt) / ang;
        Q4 dq = Q4{cb.omg.x * f, cb.omg.y * f, cb.omg.z * f, cosf(0.5f * ang * dt)};
        Q4 nq = qmul(dq, cb.quat);
        float nn = rsqrtf(nq.x * nq.x + nq.y * nq.y + nq.z * nq.z + nq.w * nq.w);
        cb.quat = Q4{nq.x * nn, nq.y * nn, nq.z * nn, nq.w * nn};
    }
    PS_PHASE(5);
}

#undef PS_COUNT_IT
#undef PS_REGATE

}  // namespace ps
